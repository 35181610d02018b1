"""The resume loop of an adaptive frame restated in numpy (include/srr_capi.h
srr_render_adaptive_resume), over a CPU-oracle render's per-path radiance: it takes
a state (count, s1, s2 per slot) and returns the state the call must leave, with a
log of its passes.  Built on tests/adaptive_ref.py's rule and luminance.  Shared by
tests/test_adaptive_resume.py (CPU) and tests/test_gpu_adaptive_resume.py."""
from __future__ import annotations

import functools

import numpy as np

import adaptive_ref as ar

F = np.float32

# The tightening case on adaptive_ref's parity frame: a frame at TOL_LOOSE, resumed at
# TOL_TIGHT.  Chosen on the CPU from the oracle's paths alone, as adaptive_ref.REL_TOL
# was (tests/test_adaptive_resume.py checks the conditions): the resume reactivates
# slots that retired at three or more different counts, levels merge as the lower
# ones catch up, and some slots stay retired throughout.
TOL_LOOSE, TOL_TIGHT = 0.1, 0.05
# The batch-change case: a frame at batch 4, resumed at batch 6 with the tighter
# tolerance; levels 4 apart never meet in steps of 6 before the budget.
BATCH2 = 6


def zero_state(npix: int) -> dict:
    return dict(count=np.zeros(npix, np.int32), s1=np.zeros(npix, F), s2=np.zeros(npix, F))


def retired(state: dict, budget: int, min_spp: int, rel_tol: float, abs_eps: float) -> np.ndarray:
    """n >= budget, or n >= min_spp, rel_tol > 0 and the rule holds: per slot."""
    n, s1, s2 = state["count"], state["s1"], state["s2"]
    out = n >= budget
    if rel_tol > 0:
        for c in np.unique(n[(n >= min_spp) & ~out]):
            sel = n == c
            out[sel] |= ar.converged_many(int(c), s1[sel], s2[sel], rel_tol, abs_eps)
    return out


def resume(paths: np.ndarray, state: dict, budget: int, batch_spp: int, min_spp: int, rel_tol: float,
           abs_eps: float):
    """The resume loop over paths[npix, >= the samples it reaches, 3]: returns
    (state, log) with one log entry per pass: dict(level, w, active (slot indices),
    from_counts (the distinct counts the active slots held when the call began))."""
    y = ar.luminance(paths)
    count, s1, s2 = state["count"].copy(), state["s1"].copy(), state["s2"].copy()
    fresh = count == 0  # a slot without samples starts from zero, whatever the state holds
    s1[fresh] = 0
    s2[fresh] = 0
    begin = count.copy()
    st = dict(count=count, s1=s1, s2=s2)
    log = []
    with np.errstate(all="ignore"):
        while True:
            live = ~retired(st, budget, min_spp, rel_tol, abs_eps)
            if not live.any():
                break
            n = int(count[live].min())
            act = live & (count == n)
            w = min(batch_spp, budget - n)
            for s in range(n, n + w):  # folded in sample order, float32
                s1[act] = s1[act] + y[act, s]
                s2[act] = s2[act] + y[act, s] * y[act, s]
            count[act] = n + w
            log.append(dict(level=n, w=w, active=np.flatnonzero(act), from_counts=np.unique(begin[act])))
    return st, log


def paths_of(log) -> int:
    return int(sum(e["active"].size * e["w"] for e in log))


@functools.lru_cache(maxsize=None)
def stage_one(rel_tol: float = TOL_LOOSE, budget: int = ar.BUDGET):
    """The parity frame rendered from nothing at rel_tol: (state, log), read-only."""
    paths = ar.oracle_frame()["paths"]
    st, log = resume(paths, zero_state(paths.shape[0]), budget, ar.BATCH, ar.MIN_SPP, rel_tol, ar.ABS_EPS)
    for a in st.values():
        a.setflags(write=False)
    return st, log


@functools.lru_cache(maxsize=None)
def tightened(batch_spp: int = ar.BATCH):
    """stage_one() resumed at TOL_TIGHT with batch_spp: (state, log), read-only."""
    paths = ar.oracle_frame()["paths"]
    st, log = resume(paths, stage_one()[0], ar.BUDGET, batch_spp, ar.MIN_SPP, TOL_TIGHT, ar.ABS_EPS)
    for a in st.values():
        a.setflags(write=False)
    return st, log


def check_tightening(first: dict, log) -> None:
    """The tightening case's preconditions, from the restatement alone."""
    reactivated = np.unique(np.concatenate([e["from_counts"] for e in log]))
    assert reactivated.size >= 3, reactivated  # slots retired at three or more counts come back
    assert any(e["from_counts"].size >= 2 for e in log)  # a pass merges two levels
    touched = np.zeros(first["count"].size, bool)
    for e in log:
        touched[e["active"]] = True
    assert (~touched).any() and touched.any()  # some slots stay retired throughout
    assert (first["count"][~touched] < ar.BUDGET).any()  # ... and not only those at the budget


def check_batch_change(log) -> None:
    """Batch 4 -> 6: at least two levels never merge before the budget, i.e. two
    first-stage counts whose slots both run several passes and never share one (8 and
    12: 8, 14, 20, 26 against 12, 18, 24, 30), so the loop has to interleave them."""
    origins = np.unique(np.concatenate([e["from_counts"] for e in log]))
    runs = {int(o): [e for e in log if o in e["from_counts"]] for o in origins}
    apart = [(a, b) for a in runs for b in runs if a < b and len(runs[a]) >= 2 and len(runs[b]) >= 2
             and not any(b in e["from_counts"] for e in runs[a])]
    assert apart, {o: [e["level"] for e in r] for o, r in runs.items()}
    # and their passes alternate: the level of consecutive passes rises by less than a batch
    assert any(y["level"] - x["level"] < x["w"] for x, y in zip(log, log[1:]))
