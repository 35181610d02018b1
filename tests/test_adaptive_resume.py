"""Resumable adaptive frames, host side (include/srr_capi.h
srr_render_adaptive_resume): the exported symbols, the restated resume loop
(tests/adaptive_resume_ref.py) against the restated fresh loop, and the conditions
on the inputs of the GPU cases (tests/test_gpu_adaptive_resume.py) -- none of
which needs a GPU."""
import numpy as np

import adaptive_ref as ar
import adaptive_resume_ref as rr
from srr import capi


def test_symbols():
    L = capi.lib()
    for name in ("srr_render_adaptive_resume", "srr_render_adaptive_resume_host", "srr_adaptive_state_get",
                 "srr_adaptive_state_set"):
        assert hasattr(L, name), name


def test_resume_from_the_zero_state_is_the_fresh_loop():
    paths = ar.oracle_frame()["paths"]
    for tol in (ar.REL_TOL, rr.TOL_LOOSE, 0.0):
        want, passes = ar.pass_loop(paths, ar.BUDGET, ar.BATCH, ar.MIN_SPP, tol, ar.ABS_EPS)
        st, log = rr.resume(paths, rr.zero_state(paths.shape[0]), ar.BUDGET, ar.BATCH, ar.MIN_SPP, tol, ar.ABS_EPS)
        np.testing.assert_array_equal(st["count"], want)
        assert len(log) == passes
        assert rr.paths_of(log) == int(want.sum())
    # garbage moments of a slot without samples are not read
    junk = rr.zero_state(paths.shape[0])
    junk["s1"][:] = 1e30
    junk["s2"][:] = np.nan
    st2, _ = rr.resume(paths, junk, ar.BUDGET, ar.BATCH, ar.MIN_SPP, ar.REL_TOL, ar.ABS_EPS)
    np.testing.assert_array_equal(st2["count"], ar.expected_counts()[0])


def test_two_stages_equal_one():
    paths = ar.oracle_frame()["paths"]
    npix = paths.shape[0]
    kw = (ar.BATCH, ar.MIN_SPP, ar.REL_TOL, ar.ABS_EPS)
    one, log1 = rr.resume(paths, rr.zero_state(npix), ar.BUDGET, *kw)
    half, loga = rr.resume(paths, rr.zero_state(npix), 16, *kw)
    two, logb = rr.resume(paths, half, ar.BUDGET, *kw)
    assert (half["count"] <= 16).all() and (half["count"] == 16).any()
    for k in ("count", "s1", "s2"):
        np.testing.assert_array_equal(two[k].view(np.uint32 if k != "count" else np.int32),
                                      one[k].view(np.uint32 if k != "count" else np.int32), err_msg=k)
    assert rr.paths_of(loga) + rr.paths_of(logb) == rr.paths_of(log1)
    assert rr.paths_of(logb) == int(one["count"].sum()) - int(half["count"].sum())
    # lowering the budget does nothing: every slot is retired
    none, logc = rr.resume(paths, one, 8, *kw)
    assert logc == [] and (none["count"] == one["count"]).all()


def test_tightening_case_meets_its_preconditions():
    """Condition on the inputs of the GPU tightening case, from the restatement alone
    (adaptive_resume_ref.check_tightening)."""
    first, _ = rr.stage_one()
    st, log = rr.tightened()
    rr.check_tightening(first, log)
    print("stage one counts", np.unique(first["count"], return_counts=True))
    print("passes", [(e["level"], e["w"], e["active"].size, e["from_counts"].tolist()) for e in log])
    # and what it reaches is what a fresh frame at the tight tolerance need not reach:
    # samples are never removed, so every slot holds at least its first-stage count
    assert (st["count"] >= first["count"]).all() and (st["count"] > first["count"]).any()
    live = ~rr.retired({k: v.copy() for k, v in st.items()}, ar.BUDGET, ar.MIN_SPP, rr.TOL_TIGHT, ar.ABS_EPS)
    assert not live.any()


def test_batch_change_case_meets_its_preconditions():
    """Batch 4 -> 6 (adaptive_resume_ref.check_batch_change): at least two levels
    never merge before the budget."""
    st, log = rr.tightened(rr.BATCH2)
    rr.check_batch_change(log)
    print("passes", [(e["level"], e["w"], e["active"].size, e["from_counts"].tolist()) for e in log])
    # counts off the batch-4 grid occur, and the last pass of a level is clipped to the budget
    assert ((st["count"] - ar.MIN_SPP) % ar.BATCH != 0).any()
    assert any(e["w"] < rr.BATCH2 for e in log)
