"""Speculative adaptive passes on the GPU (srr_adaptive_speculate): every comparison is
bit for bit -- against the same library's frame without speculation, against the numpy
restatement (tests/adaptive_spec_ref.py, tests/adaptive_resume_ref.py) and against the
CPU oracle's fixed-spp frame of each pixel's own count."""
import numpy as np
import pytest

import adaptive_ref as ar
import adaptive_resume_ref as rr
import adaptive_spec_ref as sr
import oracle_bind as ob
from srr import capi, scenes

pytestmark = pytest.mark.gpu

NPIX = ar.NX * ar.NY
KW = dict(batch_spp=ar.BATCH, min_spp=ar.MIN_SPP, rel_tol=ar.REL_TOL, abs_eps=ar.ABS_EPS)
LOOSE = dict(KW, rel_tol=rr.TOL_LOOSE)
TIGHT = dict(KW, rel_tol=rr.TOL_TIGHT)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    np.testing.assert_array_equal(got["count"], want["count"])
    np.testing.assert_array_equal(_bits(got["mean"]), _bits(want["mean"]))
    np.testing.assert_array_equal(got["img8"], want["img8"])


def _same_moments(r, want):
    st = r.adaptive_state()
    np.testing.assert_array_equal(st["count"], want["count"])
    np.testing.assert_array_equal(_bits(st["mom"][:, 0]), _bits(want["s1"]))
    np.testing.assert_array_equal(_bits(st["mom"][:, 1]), _bits(want["s2"]))


def _assert_fixed_frames(text, nx, ny, mean, count, counts=None):
    """Every pixel is bitwise the CPU oracle's fixed-spp frame at its own count."""
    for c in np.unique(count) if counts is None else counts:
        px = np.flatnonzero(count == c).astype(np.int32)
        img = ob.render(text, nx, ny, int(c), 50, pixels=px, want_paths=False)["img"]
        np.testing.assert_array_equal(_bits(mean[px]), _bits(img), err_msg=f"pixels with {c} samples")


def _spec(text, pass_spp_max, fill=sr.HUGE):
    r = capi.Renderer(text)
    r.adaptive_speculate(pass_spp_max, fill)
    return r


def _check_stats(r, out, log):
    """The call's stats and launches are the restatement's log (a pass is one window here)."""
    st, sp = out["stats"], r.adaptive_spec_stats()
    assert st["passes"] == sp["windows"] == len(log)
    assert sp["paths_traced"] == sr.traced_of(log)
    assert sp["paths_discarded"] == sr.discarded_of(log)
    assert st["paths"] == sp["paths_traced"] - sp["paths_discarded"]


@pytest.fixture(scope="module")
def text():
    return ar.scene_text()


@pytest.fixture(scope="module")
def plain32(text):
    """The parity frame without speculation (read-only)."""
    out = capi.Renderer(text).render_adaptive(ar.NX, ar.NY, ar.BUDGET, 50, **KW)
    for k in ("mean", "count", "img8"):
        out[k].setflags(write=False)
    return out


def test_one_pass(text, plain32):
    want, log = sr.fresh(32, sr.HUGE)
    sr.check_one_pass(log)
    r = _spec(text, 32)
    out = r.render_adaptive(ar.NX, ar.NY, ar.BUDGET, 50, **KW)
    _same(out, plain32)
    _same_moments(r, want)
    st, sp = out["stats"], r.adaptive_spec_stats()
    assert st["passes"] == 1 and sp["windows"] == 1
    assert st["paths"] == int(out["count"].sum())
    assert sp["paths_traced"] == NPIX * 32
    assert sp["paths_discarded"] == sp["paths_traced"] - st["paths"] == log[0]["discarded"] > 0
    assert st["pixels_retired"] == plain32["stats"]["pixels_retired"] == int((out["count"] < ar.BUDGET).sum())
    fixed = capi.Renderer(text).render(ar.NX, ar.NY, 32, 50)
    assert st["world_rays"] == fixed["stats"]["world_rays"]
    _assert_fixed_frames(text, ar.NX, ar.NY, out["mean"], out["count"])


def test_mixed_k(text, plain32):
    want, log = sr.fresh(sr.MIXED_PASS_SPP, sr.MIXED_FILL)
    sr.check_mixed(log)
    r = _spec(text, sr.MIXED_PASS_SPP, sr.MIXED_FILL)
    out = r.render_adaptive(ar.NX, ar.NY, ar.BUDGET, 50, **KW)
    _same(out, plain32)
    _same_moments(r, want)
    _check_stats(r, out, log)
    assert out["stats"]["passes"] < plain32["stats"]["passes"]
    assert out["stats"]["pixels_retired"] == plain32["stats"]["pixels_retired"]


@pytest.mark.parametrize("budget,batch,pass_spp_max,fill", [(30, 4, 10, sr.HUGE), (30, 6, 18, sr.HUGE),
                                                            (30, 6, 18, sr.MIXED_FILL)])
def test_odd_edges(text, budget, batch, pass_spp_max, fill):
    """A budget that is no multiple of 4, a pass_spp_max that floors to two batches, and
    window widths of 6 and 18 (scalar loads) and 12 (16-byte loads)."""
    kw = dict(KW, batch_spp=batch)
    want, log = sr.fresh(pass_spp_max, fill, budget=budget, batch_spp=batch)
    plain = capi.Renderer(text).render_adaptive(ar.NX, ar.NY, budget, 50, **kw)
    r = _spec(text, pass_spp_max, fill)
    out = r.render_adaptive(ar.NX, ar.NY, budget, 50, **kw)
    _same(out, plain)
    _same_moments(r, want)
    _check_stats(r, out, log)
    assert out["stats"]["pixels_retired"] == plain["stats"]["pixels_retired"]


@pytest.mark.parametrize("batch", [ar.BATCH, rr.BATCH2])
def test_resume(text, batch):
    want, plain_log = rr.tightened(batch)
    got, log = sr.tightened(32, sr.HUGE, batch)
    sr.same_state(got, want)
    tight = dict(TIGHT, batch_spp=batch)
    # without speculation
    p = capi.Renderer(text)
    p.render_adaptive(ar.NX, ar.NY, ar.BUDGET, 50, **LOOSE)
    plain = p.render_adaptive_resume(ar.NX, ar.NY, ar.BUDGET, 50, **tight)
    # with it, the first frame too
    r = _spec(text, 32)
    one = r.render_adaptive(ar.NX, ar.NY, ar.BUDGET, 50, **LOOSE)
    np.testing.assert_array_equal(one["count"], rr.stage_one()[0]["count"])
    out = r.render_adaptive_resume(ar.NX, ar.NY, ar.BUDGET, 50, **tight)
    _same(out, plain)
    _same_moments(r, want)
    _check_stats(r, out, log)
    assert out["stats"]["paths"] == plain["stats"]["paths"] == rr.paths_of(plain_log)
    assert out["stats"]["pixels_retired"] == plain["stats"]["pixels_retired"]
    # (each level the first frame left is now one wide pass: never more passes, not always fewer)
    assert out["stats"]["passes"] <= plain["stats"]["passes"] == len(plain_log)
    assert any(e["k"] > 1 for e in log) and r.adaptive_spec_stats()["paths_discarded"] > 0
    np.testing.assert_array_equal(_bits(r.adaptive_variance(out["count"])), _bits(p.adaptive_variance(plain["count"])))


def test_windows_not_aligned_with_batches(monkeypatch):
    """S2 at 96 x 64, batch 8, one pass of 96 samples cut into sample windows by a 1 MiB
    window budget: 1 MiB / (12 B x 6,144 rows) = 14 samples, which is no multiple of the
    batch, so slots stop inside windows and windows begin on and off boundaries."""
    text = scenes.s2_cornell_teapot()[0].text()
    nx, ny, budget = 96, 64, 96
    kw = dict(batch_spp=8, min_spp=8, rel_tol=ar.REL_TOL, abs_eps=ar.ABS_EPS)
    plain = capi.Renderer(text).render_adaptive(nx, ny, budget, 50, **kw)
    r = _spec(text, 96)
    whole = r.render_adaptive(nx, ny, budget, 50, **kw)
    whole_sp = r.adaptive_spec_stats()
    assert whole["stats"]["passes"] == 1 and whole_sp["windows"] == 1
    monkeypatch.setenv("SRR_WINDOW_MB", "1")
    r2 = _spec(text, 96)
    cut = r2.render_adaptive(nx, ny, budget, 50, **kw)
    cut_sp = r2.adaptive_spec_stats()
    monkeypatch.delenv("SRR_WINDOW_MB")
    assert cut["stats"]["passes"] == 1 and cut_sp["windows"] == -(-96 // 14)
    _same(cut, whole)
    _same(cut, plain)
    assert cut_sp["paths_traced"] == whole_sp["paths_traced"] == nx * ny * budget
    assert cut_sp["paths_discarded"] == whole_sp["paths_discarded"] == nx * ny * budget - int(plain["count"].sum())
    assert cut["stats"] == {**whole["stats"], "total_ms": cut["stats"]["total_ms"]}
    for a, b in (("sums", "sums"), ("mom", "mom")):
        np.testing.assert_array_equal(_bits(r2.adaptive_state()[a]), _bits(r.adaptive_state()[b]))
    counts = np.unique(plain["count"])
    assert counts.size >= 3 and (counts % 14 != 0).any()
    # two counts against the oracle: the least, and one that lies inside a window
    inside = [int(c) for c in counts if c % 14 != 0 and c > counts[0]][:1]
    _assert_fixed_frames(text, nx, ny, cut["mean"], cut["count"], [int(counts[0])] + inside)


def test_rel_tol_zero_is_the_fixed_frame(text):
    r = _spec(text, 32)
    out = r.render_adaptive(ar.NX, ar.NY, ar.BUDGET, 50, **dict(KW, rel_tol=0.0))
    fixed = capi.Renderer(text).render(ar.NX, ar.NY, ar.BUDGET, 50)
    np.testing.assert_array_equal(_bits(out["mean"]), _bits(fixed["mean"]))
    assert (out["count"] == ar.BUDGET).all()
    sp = r.adaptive_spec_stats()
    assert out["stats"]["passes"] == 1 and sp["windows"] == 1
    assert sp["paths_discarded"] == 0 and sp["paths_traced"] == out["stats"]["paths"] == NPIX * ar.BUDGET
    assert out["stats"]["world_rays"] == fixed["stats"]["world_rays"] and out["stats"]["pixels_retired"] == 0


def test_partial_last_block_and_two_scan_chunks(text):
    nx, ny = ar.BIG_NX, ar.BIG_NYS[0]
    kw = dict(batch_spp=ar.BIG_BATCH, min_spp=ar.BIG_MIN_SPP, rel_tol=ar.BIG_REL_TOL, abs_eps=ar.ABS_EPS)
    count, passes = ar.big_expected_counts(ny)
    ar.check_big_frame(count, ny)
    r = _spec(text, 12)
    out = r.render_adaptive(nx, ny, ar.BIG_BUDGET, 50, **kw)
    np.testing.assert_array_equal(out["count"], count)
    sp = r.adaptive_spec_stats()
    assert out["stats"]["passes"] == 1 < passes
    assert out["stats"]["paths"] == int(count.sum()) == sp["paths_traced"] - sp["paths_discarded"]
    assert out["stats"]["pixels_retired"] == int((count < ar.BIG_BUDGET).sum())
    # and with a fill that leaves the first pass alone, so that the compaction runs before a wider pass
    r.adaptive_speculate(12, nx * ny * ar.BIG_BATCH)
    two = r.render_adaptive(nx, ny, ar.BIG_BUDGET, 50, **kw)
    _same(two, out)
    assert two["stats"]["passes"] == 2 and two["stats"]["pixels_retired"] == out["stats"]["pixels_retired"]


def test_off_and_refusals(text, plain32):
    r = capi.Renderer(text)
    with pytest.raises(capi.SrrError):  # no adaptive call yet
        r.adaptive_spec_stats()
    for bad in ((-1, 0), (8, -1)):
        with pytest.raises(capi.SrrError):
            r.adaptive_speculate(*bad)
    multi = capi.Renderer(text, devices=[0, 0])  # the one-GPU rehearsal of a multi-device renderer
    with pytest.raises(capi.SrrError):
        multi.adaptive_speculate(32, 0)
    with pytest.raises(capi.SrrError):
        multi.adaptive_spec_stats()
    # switched on, then off again: the frame and its stats are a fresh renderer's
    r.adaptive_speculate(32, sr.HUGE)
    assert r.render_adaptive(ar.NX, ar.NY, ar.BUDGET, 50, **KW)["stats"]["passes"] == 1
    r.adaptive_speculate(0, 0)
    out = r.render_adaptive(ar.NX, ar.NY, ar.BUDGET, 50, **KW)
    _same(out, plain32)
    assert out["stats"] == {**plain32["stats"], "total_ms": out["stats"]["total_ms"]}
    sp = r.adaptive_spec_stats()
    assert sp == dict(windows=out["stats"]["passes"], paths_traced=out["stats"]["paths"], paths_discarded=0)
    # a pass_spp_max below two batches is off as well
    r.adaptive_speculate(2 * ar.BATCH - 1, sr.HUGE)
    out = r.render_adaptive(ar.NX, ar.NY, ar.BUDGET, 50, **KW)
    assert out["stats"] == {**plain32["stats"], "total_ms": out["stats"]["total_ms"]}
