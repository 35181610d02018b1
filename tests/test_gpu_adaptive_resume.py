"""Resumable adaptive frames on the GPU (srr_render_adaptive_resume,
srr_adaptive_state_get / _set, Progressive(adaptive=...)): every comparison is bit
for bit -- against a fresh adaptive frame, against the numpy restatement of the
resume loop (tests/adaptive_resume_ref.py) and against the CPU oracle's fixed-spp
frame of each pixel's own count."""
import ctypes

import numpy as np
import pytest

import adaptive_ref as ar
import adaptive_resume_ref as rr
import oracle_bind as ob
from srr import capi
from srr.progressive import Progressive

pytestmark = pytest.mark.gpu

KW = dict(batch_spp=ar.BATCH, min_spp=ar.MIN_SPP, rel_tol=ar.REL_TOL, abs_eps=ar.ABS_EPS)
LOOSE = dict(KW, rel_tol=rr.TOL_LOOSE)
TIGHT = dict(KW, rel_tol=rr.TOL_TIGHT)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    np.testing.assert_array_equal(got["count"], want["count"])
    np.testing.assert_array_equal(_bits(got["mean"]), _bits(want["mean"]))
    np.testing.assert_array_equal(got["img8"], want["img8"])


def _assert_fixed_frames(text, mean, count):
    """Every pixel is bitwise the CPU oracle's fixed-spp frame at its own count."""
    for c in np.unique(count):
        px = np.flatnonzero(count == c).astype(np.int32)
        img = ob.render(text, ar.NX, ar.NY, int(c), 50, pixels=px, want_paths=False)["img"]
        np.testing.assert_array_equal(_bits(mean[px]), _bits(img), err_msg=f"pixels with {c} samples")


@pytest.fixture(scope="module")
def text():
    return ar.scene_text()


@pytest.fixture(scope="module")
def fresh32(text):
    """The parity frame rendered in one call at the budget (read-only)."""
    out = capi.Renderer(text).render_adaptive(ar.NX, ar.NY, ar.BUDGET, 50, **KW)
    for k in ("mean", "count", "img8"):
        out[k].setflags(write=False)
    return out


def _stage_one(text, budget=16, kw=KW):
    r = capi.Renderer(text)
    return r, r.render_adaptive(ar.NX, ar.NY, budget, 50, **kw)


def test_budget_raised(text, fresh32):
    r, first = _stage_one(text)
    assert (first["count"] <= 16).all() and (first["count"] < 16).any() and (first["count"] == 16).any()
    out = r.render_adaptive_resume(ar.NX, ar.NY, ar.BUDGET, 50, **KW)
    _same(out, fresh32)
    st = out["stats"]
    assert st["paths"] == int(fresh32["count"].sum()) - int(first["count"].sum()) > 0
    assert st["world_rays"] + first["stats"]["world_rays"] == fresh32["stats"]["world_rays"]
    assert st["pixels_retired"] == fresh32["stats"]["pixels_retired"] == int((fresh32["count"] < ar.BUDGET).sum())
    assert st["passes"] == fresh32["stats"]["passes"] - first["stats"]["passes"]


def test_tolerance_tightened(text):
    first, _ = rr.stage_one()
    want, log = rr.tightened()
    rr.check_tightening(first, log)
    r, one = _stage_one(text, ar.BUDGET, LOOSE)
    np.testing.assert_array_equal(one["count"], first["count"])
    out = r.render_adaptive_resume(ar.NX, ar.NY, ar.BUDGET, 50, **TIGHT)
    np.testing.assert_array_equal(out["count"], want["count"])
    _assert_fixed_frames(text, out["mean"], out["count"])
    assert out["stats"]["passes"] == len(log)
    assert out["stats"]["paths"] == rr.paths_of(log)
    assert out["stats"]["pixels_retired"] == int((want["count"] < ar.BUDGET).sum())
    # the moments it leaves are the restatement's
    mom = r.adaptive_state()["mom"]
    np.testing.assert_array_equal(_bits(mom[:, 0]), _bits(want["s1"]))
    np.testing.assert_array_equal(_bits(mom[:, 1]), _bits(want["s2"]))


def test_batch_changed(text):
    want, log = rr.tightened(rr.BATCH2)
    rr.check_batch_change(log)
    r, _ = _stage_one(text, ar.BUDGET, LOOSE)
    out = r.render_adaptive_resume(ar.NX, ar.NY, ar.BUDGET, 50, **dict(TIGHT, batch_spp=rr.BATCH2))
    np.testing.assert_array_equal(out["count"], want["count"])
    _assert_fixed_frames(text, out["mean"], out["count"])
    assert out["stats"]["passes"] == len(log)
    assert out["stats"]["paths"] == rr.paths_of(log)


def test_nothing_to_do(text):
    r, first = _stage_one(text)
    out = r.render_adaptive_resume(ar.NX, ar.NY, 8, 50, **KW)  # every slot holds 8 or more
    assert out["stats"]["passes"] == 0 and out["stats"]["paths"] == 0 and out["stats"]["world_rays"] == 0
    assert out["stats"]["pixels_retired"] == 0
    _same(out, first)
    # and the state is still what it was: raising the budget goes on from it
    out = r.render_adaptive_resume(ar.NX, ar.NY, 16, 50, **KW)
    assert out["stats"]["passes"] == 0
    _same(out, first)


def test_zero_state_is_a_fresh_frame(text, fresh32):
    npix = ar.NX * ar.NY
    r = capi.Renderer(text)
    rng = np.random.default_rng(7)
    junk = rng.standard_normal((npix, 3)).astype(np.float32) * np.float32(1e20)
    junk[::5] = np.nan
    r.set_adaptive_state(ar.NX, ar.NY, junk, junk[:, :2], np.zeros(npix, np.int32))
    out = r.render_adaptive_resume(ar.NX, ar.NY, ar.BUDGET, 50, **KW)
    _same(out, fresh32)
    assert out["stats"] == {**fresh32["stats"], "total_ms": out["stats"]["total_ms"]}


def test_transplant(text, fresh32):
    a, first = _stage_one(text)
    st = a.adaptive_state()
    np.testing.assert_array_equal(st["count"], first["count"])
    b = capi.Renderer(text)
    b.set_adaptive_state(ar.NX, ar.NY, st["sums"], st["mom"], st["count"])
    back = b.adaptive_state()
    for k in ("sums", "mom"):
        np.testing.assert_array_equal(_bits(back[k]), _bits(st[k]), err_msg=k)
    np.testing.assert_array_equal(back["count"], st["count"])
    out_a = a.render_adaptive_resume(ar.NX, ar.NY, ar.BUDGET, 50, **KW)
    out_b = b.render_adaptive_resume(ar.NX, ar.NY, ar.BUDGET, 50, **KW)
    _same(out_b, out_a)
    _same(out_a, fresh32)
    assert out_b["stats"]["paths"] == out_a["stats"]["paths"]
    assert out_b["stats"]["world_rays"] == out_a["stats"]["world_rays"]


def test_variance_after_a_resume(text):
    r, _ = _stage_one(text)
    out = r.render_adaptive_resume(ar.NX, ar.NY, ar.BUDGET, 50, **KW)
    st = r.adaptive_state()
    np.testing.assert_array_equal(st["count"], out["count"])
    L = capi.lib()
    want = np.array([L.srr_variance_of_mean(int(n), float(s1), float(s2)) for n, (s1, s2) in zip(st["count"], st["mom"])],
                    np.float32)
    np.testing.assert_array_equal(_bits(r.adaptive_variance(out["count"])), _bits(want))
    assert np.unique(out["count"]).size >= 3


def test_many_slots(text):
    """300 x 220 = 66,000 slots: the whole-slot select and compaction of a resume run
    258 blocks, two scan chunks and a partial last block (adaptive_ref.check_big_frame)."""
    nx, ny = ar.BIG_NX, ar.BIG_NYS[0]
    kw = dict(batch_spp=ar.BIG_BATCH, min_spp=ar.BIG_MIN_SPP, rel_tol=ar.BIG_REL_TOL, abs_eps=ar.ABS_EPS)
    fresh = capi.Renderer(text).render_adaptive(nx, ny, ar.BIG_BUDGET, 50, **kw)
    ar.check_big_frame(fresh["count"], ny)
    r = capi.Renderer(text)
    first = r.render_adaptive(nx, ny, 8, 50, **kw)
    out = r.render_adaptive_resume(nx, ny, ar.BIG_BUDGET, 50, **kw)
    _same(out, fresh)
    keep = fresh["count"] > 8  # the slots the resume's one pass takes, selected among all 66,000
    assert keep.sum() > 256 and (~keep[:ar.CHUNK_ROWS]).sum() > 256 and out["stats"]["passes"] == 1
    assert out["stats"]["paths"] == int(keep.sum()) * 4
    assert out["stats"]["world_rays"] + first["stats"]["world_rays"] == fresh["stats"]["world_rays"]


def test_refusals(text, fresh32):
    nx, ny = ar.NX, ar.NY
    r = capi.Renderer(text)
    with pytest.raises(capi.SrrError):  # no adaptive frame yet
        r.render_adaptive_resume(nx, ny, ar.BUDGET, 50, **KW)
    with pytest.raises(capi.SrrError):
        r.adaptive_state()
    first = r.render_adaptive(nx, ny, 16, 50, **KW)
    for kw in (dict(flags=capi.FLAG_CONTINUE), dict(flags=capi.FLAG_KEEP_PATHS), dict(flags=capi.FLAG_SUMS),
               dict(flags=capi.FLAG_WAVEFRONT), dict(flags=capi.FLAG_COUNT_VISITS), dict(batch_spp=0),
               dict(min_spp=0), dict(rel_tol=-1.0), dict(rel_tol=float("nan")), dict(abs_eps=-1e-3),
               dict(sample_begin=1), dict(struct_size=ctypes.sizeof(capi.AdaptiveParams) - 4)):
        with pytest.raises(capi.SrrError):
            r.render_adaptive_resume(nx, ny, ar.BUDGET, 50, **{**KW, **kw})
    with pytest.raises(capi.SrrError):  # another nx
        r.render_adaptive_resume(nx + 1, ny, ar.BUDGET, 50, **KW)
    with pytest.raises(capi.SrrError):  # another shard of the same frame
        r.render_adaptive_resume(nx, ny, ar.BUDGET, 50, shard=(0, 2), tile=8, **KW)
    p = capi.make_params(nx, ny, ar.BUDGET, 50)
    a = capi.AdaptiveParams(ctypes.sizeof(capi.AdaptiveParams), ar.BATCH, ar.MIN_SPP, ar.REL_TOL, ar.ABS_EPS)
    with pytest.raises(capi.SrrError):  # a NULL d_mean
        r.render_adaptive_resume_device(p, a, 0)
    npix = nx * ny
    z3, z2, zc = np.zeros((npix, 3), np.float32), np.zeros((npix, 2), np.float32), np.zeros(npix, np.int32)
    with pytest.raises(capi.SrrError):  # a wrong npix
        r.set_adaptive_state(nx, ny, z3, z2, zc, npix=npix - 1)
    neg = zc.copy()
    neg[npix // 2] = -1
    with pytest.raises(capi.SrrError):  # a negative count
        r.set_adaptive_state(nx, ny, z3, z2, neg)
    multi = capi.Renderer(text, devices=[0, 0])  # the one-GPU rehearsal of a multi-device renderer
    with pytest.raises(capi.SrrError):
        multi.render_adaptive_resume(nx, ny, ar.BUDGET, 50, **KW)
    with pytest.raises(capi.SrrError):
        multi.set_adaptive_state(nx, ny, z3, z2, zc)
    # none of the refusals touched the state: the resume goes on from the first frame
    _same(r.render_adaptive_resume(nx, ny, ar.BUDGET, 50, **KW), fresh32)


@pytest.mark.parametrize("writer", ["render", "accum_set"])
def test_overwritten_sums_refuse_a_resume_but_not_the_variance(text, writer):
    nx, ny = ar.NX, ar.NY
    r = capi.Renderer(text)
    first = r.render_adaptive(nx, ny, 16, 50, **KW)
    var = r.adaptive_variance(first["count"])
    if writer == "render":
        r.render(nx, ny, 2, 50)
    else:
        sums = np.zeros((nx * ny, 3), np.float32)
        capi._check(capi.lib().srr_accum_set(r.h, capi._ptr(sums), nx * ny, 0))
    with pytest.raises(capi.SrrError):
        r.render_adaptive_resume(nx, ny, ar.BUDGET, 50, **KW)
    with pytest.raises(capi.SrrError):
        r.adaptive_state()
    np.testing.assert_array_equal(_bits(r.adaptive_variance(first["count"])), _bits(var))  # needs only the moments
    # a fresh adaptive frame makes the renderer resumable again
    r.render_adaptive(nx, ny, 16, 50, **KW)
    assert r.render_adaptive_resume(nx, ny, 16, 50, **KW)["stats"]["passes"] == 0


def _adaptive_params():
    return capi.AdaptiveParams(ctypes.sizeof(capi.AdaptiveParams), ar.BATCH, ar.MIN_SPP, ar.REL_TOL, ar.ABS_EPS)


def test_progressive_steps_save_and_load(text, fresh32, tmp_path):
    pr = Progressive(capi.Renderer(text), ar.NX, ar.NY, adaptive=_adaptive_params())
    pr.step(16)
    path = str(tmp_path / "state.npz")
    pr.save(path)
    mean = pr.step(16)
    np.testing.assert_array_equal(_bits(mean), _bits(fresh32["mean"]))
    np.testing.assert_array_equal(pr.count, fresh32["count"])
    assert pr.samples == ar.BUDGET
    # the saved first step, continued in a new renderer
    pr2 = Progressive(capi.Renderer(text), ar.NX, ar.NY, adaptive=_adaptive_params())
    pr2.load(path)
    assert pr2.samples == 16
    np.testing.assert_array_equal(_bits(pr2.step(16)), _bits(fresh32["mean"]))
    np.testing.assert_array_equal(pr2.count, fresh32["count"])
    # another frame, another scene, another base_seed and a fixed-spp Progressive refuse it
    from srr import scenes
    for bad in (Progressive(capi.Renderer(text), ar.NX + 1, ar.NY, adaptive=_adaptive_params()),
                Progressive(capi.Renderer(scenes.s2_cornell_teapot()[0].text()), ar.NX, ar.NY, adaptive=True),
                Progressive(capi.Renderer(text), ar.NX, ar.NY, adaptive=_adaptive_params(), base_seed=5),
                Progressive(capi.Renderer(text), ar.NX, ar.NY)):
        with pytest.raises(capi.SrrError):
            bad.load(path)


def test_progressive_variance_guided_denoise(text):
    nx, ny = ar.NX, ar.NY
    dv = capi.DenoiseVarParams.defaults()
    pr = Progressive(capi.Renderer(text), nx, ny, adaptive=_adaptive_params(), denoise=dv, aov_spp=4)
    pr.step(16)
    got = pr.step(16)
    # the pieces by hand
    r = capi.Renderer(text)
    out = r.render_adaptive(nx, ny, ar.BUDGET, 50, **KW)
    np.testing.assert_array_equal(_bits(pr.mean), _bits(out["mean"]))
    var = r.adaptive_variance(out["count"])
    aov = r.render_aov(nx, ny, 4)
    shape = (ny, nx, 3)
    want, _ = capi.denoise_var(out["mean"].reshape(shape), var.reshape(ny, nx), aov["albedo"].reshape(shape),
                               aov["normal"].reshape(shape), aov["depth"].reshape(ny, nx), dv)
    np.testing.assert_array_equal(_bits(got), _bits(want.reshape(-1, 3)))
    assert (_bits(got) != _bits(pr.mean)).any()  # the filter did something
    with pytest.raises(capi.SrrError):  # the variance comes from an adaptive frame
        Progressive(capi.Renderer(text), nx, ny, denoise=dv)
