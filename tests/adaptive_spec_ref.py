"""Speculative adaptive passes restated in numpy (include/srr_capi.h
srr_adaptive_speculate): the schedule in Python integers, and the resume loop with
passes of several batches over a CPU-oracle render's per-path radiance -- fresh (from
a zero state) and resumed.  It returns the state the call must leave and a log of its
passes.  Built on tests/adaptive_ref.py's rule and tests/adaptive_resume_ref.py's
retirement.  Shared by tests/test_adaptive_spec.py (CPU) and
tests/test_gpu_adaptive_spec.py."""
from __future__ import annotations

import functools

import numpy as np

import adaptive_ref as ar
import adaptive_resume_ref as rr

F = np.float32

HUGE = 1 << 40  # a fill_paths no frame of the tests reaches: every pass as wide as pass_spp_max allows
# The mixed-k case on the parity frame (1,073 slots, batch 4): pass_spp_max = 12 allows three
# batches, and 6,000 paths are fewer than two batches of the whole frame (8,584) but more
# than two batches of the slots still active after the first decision at 8 samples
# (tests/test_adaptive_spec.py checks that passes of one batch and of several both occur).
MIXED_PASS_SPP, MIXED_FILL = 12, 6000


def pass_width(n_active: int, n: int, budget: int, batch_spp: int, pass_spp_max: int, fill_paths: int,
               fill_default: int) -> int:
    """kmax = max(1, pass_spp_max // batch_spp); k = clamp(fill_paths // (n_active * batch_spp), 1, kmax);
    w = min(k * batch_spp, budget - n).  fill_paths = 0 stands for fill_default."""
    fill = fill_paths if fill_paths else fill_default
    kmax = max(1, pass_spp_max // batch_spp)
    k = min(kmax, max(1, fill // (n_active * batch_spp)))
    return min(k * batch_spp, budget - n)


def boundaries(n: int, w: int, batch_spp: int):
    """The counts at which a pass at level n of width w asks the rule."""
    return sorted(set(range(n + batch_spp, n + w, batch_spp)) | {n + w})


def resume(paths: np.ndarray, state: dict, budget: int, batch_spp: int, min_spp: int, rel_tol: float,
           abs_eps: float, pass_spp_max: int, fill_paths: int, fill_default: int = 1 << 20):
    """adaptive_resume_ref.resume with speculative passes: returns (state, log), one log
    entry per pass: dict(level, w, k (batches the schedule chose), active (slot indices),
    stop (the count each active slot holds after the pass), discarded (samples traced past
    the stops))."""
    y = ar.luminance(paths)
    count, s1, s2 = state["count"].copy(), state["s1"].copy(), state["s2"].copy()
    fresh = count == 0  # a slot without samples starts from zero, whatever the state holds
    s1[fresh] = 0
    s2[fresh] = 0
    st = dict(count=count, s1=s1, s2=s2)
    log = []
    with np.errstate(all="ignore"):
        while True:
            live = ~rr.retired(st, budget, min_spp, rel_tol, abs_eps)
            if not live.any():
                break
            n = int(count[live].min())
            act = live & (count == n)
            w = pass_width(int(act.sum()), n, budget, batch_spp, pass_spp_max, fill_paths, fill_default)
            asks = set(boundaries(n, w, batch_spp))
            going = act.copy()
            for s in range(n, n + w):  # folded in sample order, float32; nothing past a stop
                s1[going] = s1[going] + y[going, s]
                s2[going] = s2[going] + y[going, s] * y[going, s]
                c = s + 1
                if c not in asks:
                    continue
                if c >= budget:
                    stop = going.copy()
                elif c >= min_spp and rel_tol > 0:
                    stop = np.zeros_like(going)
                    stop[going] = ar.converged_many(c, s1[going], s2[going], rel_tol, abs_eps)
                else:
                    continue
                count[stop] = c
                going &= ~stop
            count[going] = n + w
            log.append(dict(level=n, w=w, k=-(-w // batch_spp), active=np.flatnonzero(act), stop=count[act].copy(),
                            discarded=int((n + w - count[act]).sum())))
    return st, log


def traced_of(log) -> int:
    return int(sum(e["active"].size * e["w"] for e in log))


def discarded_of(log) -> int:
    return int(sum(e["discarded"] for e in log))


def _frozen(st, log):
    for a in st.values():
        a.setflags(write=False)
    return st, log


@functools.lru_cache(maxsize=None)
def fresh(pass_spp_max: int, fill_paths: int, rel_tol: float = ar.REL_TOL, budget: int = ar.BUDGET,
          batch_spp: int = ar.BATCH, fill_default: int = 1 << 20):
    """The parity frame from nothing with speculative passes: (state, log), read-only."""
    paths = ar.oracle_frame()["paths"]
    return _frozen(*resume(paths, rr.zero_state(paths.shape[0]), budget, batch_spp, ar.MIN_SPP, rel_tol, ar.ABS_EPS,
                           pass_spp_max, fill_paths, fill_default))


@functools.lru_cache(maxsize=None)
def tightened(pass_spp_max: int, fill_paths: int, batch_spp: int = ar.BATCH, fill_default: int = 1 << 20):
    """adaptive_resume_ref.stage_one() resumed at TOL_TIGHT with speculative passes."""
    paths = ar.oracle_frame()["paths"]
    return _frozen(*resume(paths, rr.stage_one()[0], ar.BUDGET, batch_spp, ar.MIN_SPP, rr.TOL_TIGHT, ar.ABS_EPS,
                           pass_spp_max, fill_paths, fill_default))


def same_state(a: dict, b: dict) -> None:
    np.testing.assert_array_equal(a["count"], b["count"])
    for k in ("s1", "s2"):
        np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=k)


def check_one_pass(log, budget: int = ar.BUDGET) -> None:
    """The one-pass case's preconditions, from the restatement alone: one pass over every
    slot; slots stop at three or more interior boundaries, some at the first one at or
    above min_spp, some run to the budget, and samples are thrown away."""
    assert len(log) == 1 and log[0]["level"] == 0 and log[0]["w"] == budget
    stop = log[0]["stop"]
    first = min(c for c in boundaries(0, budget, ar.BATCH) if c >= ar.MIN_SPP)
    interior = np.unique(stop[(stop > first) & (stop < budget)])
    assert interior.size >= 3, interior
    assert (stop == first).any() and (stop == budget).any()
    assert stop.min() >= ar.MIN_SPP
    assert log[0]["discarded"] > 0


def check_mixed(log) -> None:
    """The mixed-k case: passes of one batch and passes of several."""
    assert any(e["k"] == 1 for e in log) and any(e["k"] > 1 for e in log), [e["k"] for e in log]
    assert discarded_of(log) > 0
