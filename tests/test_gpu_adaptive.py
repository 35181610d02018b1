"""Adaptive sampling on the GPU (srr_render_adaptive): every pixel ends with its
own sample count n_i and holds bitwise the CPU oracle's image of that pixel at
ns = n_i; the counts are those of the numpy restatement of the pass loop
(tests/adaptive_ref.py); retired pixels are not traced."""
import ctypes

import numpy as np
import pytest

import adaptive_ref as ar
import oracle_bind as ob
from srr import capi

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def text():
    return ar.scene_text()


@pytest.fixture(scope="module")
def whole(text):
    """The parity frame rendered adaptively once (read-only for the tests)."""
    out = capi.Renderer(text).render_adaptive(ar.NX, ar.NY, ar.BUDGET, 50, batch_spp=ar.BATCH, min_spp=ar.MIN_SPP,
                                              rel_tol=ar.REL_TOL, abs_eps=ar.ABS_EPS)
    for k in ("mean", "count"):
        out[k].setflags(write=False)
    return out


def test_oracle_parity(text, whole):
    want, passes = ar.expected_counts()
    ref = ar.oracle_frame()
    count, mean, st = whole["count"], whole["mean"], whole["stats"]
    np.testing.assert_array_equal(count, want)
    for c in np.unique(want):
        px = np.flatnonzero(want == c).astype(np.int32)
        img = ob.render(text, ar.NX, ar.NY, int(c), 50, pixels=px, want_paths=False)["img"]
        np.testing.assert_array_equal(_bits(mean[px]), _bits(img), err_msg=f"pixels with {c} samples")
    assert st["paths"] == int(count.sum())
    assert st["passes"] == passes
    assert st["pixels_retired"] == int((want < ar.BUDGET).sum())
    # retired pixels are really not traced: the world rays are those of each pixel's first n_i paths
    taken = np.arange(ar.BUDGET)[None, :] < want[:, None]
    assert st["world_rays"] == int(ref["rays"].astype(np.int64)[taken].sum())


@pytest.mark.parametrize("batch", [4, 5])  # 5 into 12: the last pass is clipped to 2 (scalar tail of the fold)
def test_zero_tolerance_is_the_fixed_spp_frame(text, batch):
    nx, ny, budget = ar.NX, ar.NY, 12
    r = capi.Renderer(text)
    out = r.render_adaptive(nx, ny, budget, 50, batch_spp=batch, min_spp=1, rel_tol=0.0)
    assert (out["count"] == budget).all()
    fixed = capi.Renderer(text).render(nx, ny, budget, 50)
    np.testing.assert_array_equal(_bits(out["mean"]), _bits(fixed["mean"]))
    np.testing.assert_array_equal(out["img8"], fixed["img8"])
    assert out["stats"]["passes"] == -(-budget // batch)
    assert out["stats"]["paths"] == nx * ny * budget
    assert out["stats"]["world_rays"] == fixed["stats"]["world_rays"]
    assert out["stats"]["pixels_retired"] == 0


@pytest.mark.parametrize("batch,min_spp", [(4, 6), (8, 8), (3, 1)])
def test_huge_tolerance_ends_at_min_spp(text, batch, min_spp):
    nx, ny = 21, 13
    out = capi.Renderer(text).render_adaptive(nx, ny, 32, 50, batch_spp=batch, min_spp=min_spp, rel_tol=1e9)
    passes = -(-min_spp // batch)
    assert out["stats"]["passes"] == passes  # no further pass is launched
    assert (out["count"] == passes * batch).all()
    assert out["stats"]["paths"] == nx * ny * passes * batch
    assert out["stats"]["pixels_retired"] == nx * ny
    fixed = capi.Renderer(text).render(nx, ny, passes * batch, 50)
    np.testing.assert_array_equal(_bits(out["mean"]), _bits(fixed["mean"]))


def test_shard_is_a_slice_of_the_whole_frame(text, whole):
    p = capi.make_params(ar.NX, ar.NY, ar.BUDGET, 50, shard=(1, 2), tile=8)
    px = capi.shard_pixels(p)
    assert 0 < px.size < ar.NX * ar.NY
    out = capi.Renderer(text).render_adaptive(ar.NX, ar.NY, ar.BUDGET, 50, batch_spp=ar.BATCH, min_spp=ar.MIN_SPP,
                                              rel_tol=ar.REL_TOL, abs_eps=ar.ABS_EPS, shard=(1, 2), tile=8)
    np.testing.assert_array_equal(out["count"], whole["count"][px])
    np.testing.assert_array_equal(_bits(out["mean"]), _bits(whole["mean"][px]))


def test_sample_windows_do_not_change_an_adaptive_frame(monkeypatch):
    """A pass larger than the window budget is split into sample windows (here
    6,144 pixels x 32 samples x 12 B = 2.25 MiB against 1 MiB: windows of 14, 14
    and 4 samples, more per window as pixels retire), on a scene with a mesh:
    counts and means are bitwise those of unsplit passes."""
    from srr import scenes
    text = scenes.s2_cornell_teapot()[0].text()
    nx, ny = 96, 64
    kw = dict(batch_spp=32, min_spp=32, rel_tol=0.05)
    one = capi.Renderer(text).render_adaptive(nx, ny, 96, 50, **kw)
    monkeypatch.setenv("SRR_WINDOW_MB", "1")
    many = capi.Renderer(text).render_adaptive(nx, ny, 96, 50, **kw)
    assert set(np.unique(one["count"])) <= {32, 64, 96} and np.unique(one["count"]).size >= 2  # some pixels retire
    np.testing.assert_array_equal(many["count"], one["count"])
    np.testing.assert_array_equal(_bits(many["mean"]), _bits(one["mean"]))
    assert many["stats"] == {**one["stats"], "total_ms": many["stats"]["total_ms"]}
    # and each pixel is the fixed-spp frame of its own count
    for c in (32, 64, 96):
        fixed = capi.Renderer(text).render(nx, ny, c, 50)["mean"]
        sel = one["count"] == c
        np.testing.assert_array_equal(_bits(one["mean"][sel]), _bits(fixed[sel]))


@pytest.mark.parametrize("ny", ar.BIG_NYS)
def test_compaction_carries_across_scan_chunks(text, ny):
    """300 x 220 = 66,000 pixels: 258 blocks of 256 rows, so the compaction's block
    scan runs two chunks of 256 block counts and the second starts from the first
    one's carry; the last block holds 208 rows.  300 x 440 = 132,000 pixels: 516
    blocks in three chunks, and 18,824 rows of the second chunk survive the first
    decision (adaptive_ref.check_big_frame), so a carry missing from a block's row
    offset scatters them over the first chunk's and the later passes trace the wrong
    pixels.  Counts are the restatement's, each pixel is bitwise the fixed-spp frame
    of its own count, and the rays are the oracle's over each pixel's first n_i paths."""
    nx, budget = ar.BIG_NX, ar.BIG_BUDGET
    want, passes = ar.big_expected_counts(ny)
    ar.check_big_frame(want, ny)
    out = capi.Renderer(text).render_adaptive(nx, ny, budget, 50, batch_spp=ar.BIG_BATCH, min_spp=ar.BIG_MIN_SPP,
                                              rel_tol=ar.BIG_REL_TOL, abs_eps=ar.ABS_EPS)
    count, mean, st = out["count"], out["mean"], out["stats"]
    np.testing.assert_array_equal(count, want)
    for c in (4, 8, 12):
        fixed = capi.Renderer(text).render(nx, ny, c, 50)["mean"]
        sel = want == c
        assert sel.any()
        np.testing.assert_array_equal(_bits(mean[sel]), _bits(fixed[sel]), err_msg=f"pixels with {c} samples")
    assert st["paths"] == int(want.sum())
    assert st["passes"] == passes
    assert st["pixels_retired"] == int((want < budget).sum())
    taken = np.arange(budget)[None, :] < want[:, None]
    assert st["world_rays"] == int(ar.big_oracle_frame(ny)["rays"].astype(np.int64)[taken].sum())


def test_refusals_leave_the_renderer_usable(text):
    nx, ny = 16, 12
    want = capi.Renderer(text).render(nx, ny, 6, 50)["mean"]
    multi = capi.Renderer(text, devices=[0, 0])  # the one-GPU rehearsal of a multi-device renderer
    with pytest.raises(capi.SrrError):
        multi.render_adaptive(nx, ny, 8, 50)
    np.testing.assert_array_equal(_bits(multi.render(nx, ny, 6, 50)["mean"]), _bits(want))
    r = capi.Renderer(text)
    for kw in (dict(flags=capi.FLAG_CONTINUE), dict(flags=capi.FLAG_KEEP_PATHS), dict(flags=capi.FLAG_SUMS),
               dict(flags=capi.FLAG_WAVEFRONT), dict(flags=capi.FLAG_COUNT_VISITS), dict(batch_spp=0),
               dict(min_spp=0), dict(rel_tol=-1.0), dict(rel_tol=float("nan")), dict(abs_eps=-1e-3),
               dict(sample_begin=4), dict(struct_size=ctypes.sizeof(capi.AdaptiveParams) - 4)):
        with pytest.raises(capi.SrrError):
            r.render_adaptive(nx, ny, 8, 50, **kw)
    np.testing.assert_array_equal(_bits(r.render(nx, ny, 6, 50)["mean"]), _bits(want))


def test_adaptive_invalidates_the_progressive_sums(text):
    nx, ny = 16, 12
    r = capi.Renderer(text)
    r.render(nx, ny, 4, 50)  # running sums of 4 samples
    r.render_adaptive(nx, ny, 8, 50, batch_spp=4, min_spp=4, rel_tol=0.1)
    with pytest.raises(capi.SrrError):
        r.render(nx, ny, 2, 50, flags=capi.FLAG_CONTINUE, sample_begin=4)
    with pytest.raises(capi.SrrError):
        r.render(nx, ny, 2, 50, flags=capi.FLAG_CONTINUE, sample_begin=8)
    # a fresh render starts new sums that can be continued again
    r.render(nx, ny, 4, 50)
    got = r.render(nx, ny, 2, 50, flags=capi.FLAG_CONTINUE, sample_begin=4)["mean"]
    np.testing.assert_array_equal(_bits(got), _bits(capi.Renderer(text).render(nx, ny, 6, 50)["mean"]))


def test_cli_adaptive_count_map(tmp_path):
    """render_main --adaptive --count-map (the C++ program, built by build()): its
    PPM is the Python API's image and its count map the grey levels 255 * n / ns."""
    import os
    import subprocess
    from srr import render_main, scenes
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))), "render_main")
    nx, ny, ns = 20, 20, 16
    ppm, png = str(tmp_path / "o.ppm"), str(tmp_path / "n.png")
    r = subprocess.run([exe, "--scene", "s1", "--nx", str(nx), "--ny", str(ny), "--ns", str(ns), "--adaptive", "0.1",
                        "--batch-spp", "4", "--min-spp", "4", "--out", ppm, "--count-map", png],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    sc, _ = scenes.s1_cornell()  # (aspect 1, as the program's builder gets for a square frame)
    want = capi.Renderer(sc.text()).render_adaptive(nx, ny, ns, 50, batch_spp=4, min_spp=4, rel_tol=0.1, tile=1)
    assert np.unique(want["count"]).size >= 2
    grey, comp = capi.image_load(png)
    assert comp == 3 and grey.shape == (ny, nx, 3)
    np.testing.assert_array_equal(grey.reshape(-1, 3), render_main.count_map(want["count"], ns))
    tok = open(ppm, "rb").read().split()
    np.testing.assert_array_equal(np.array(tok[4:], np.int64).reshape(-1, 3), want["img8"])
    assert f"{int(want['count'].sum())} of {nx * ny * ns} samples" in r.stderr
    assert subprocess.run([exe, "--scene", "s1", "--count-map", png], capture_output=True).returncode == 2


def test_device_buffers_and_null_count(text):
    """srr_render_adaptive itself: device pointers, d_count NULL."""
    import torch
    nx, ny = 16, 12
    want = capi.Renderer(text).render_adaptive(nx, ny, 16, 50, batch_spp=4, min_spp=4, rel_tol=0.1)
    p = capi.make_params(nx, ny, 16, 50)
    a = capi.AdaptiveParams(ctypes.sizeof(capi.AdaptiveParams), 4, 4, 0.1, 1e-3)
    d_mean = torch.zeros(nx * ny, 3, device="cuda:0")
    st = capi.Renderer(text).render_adaptive_device(p, a, d_mean.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(d_mean.cpu().numpy()), _bits(want["mean"]))
    assert st["paths"] == want["stats"]["paths"]
