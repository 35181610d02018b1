"""End to end on the GPU: a 16-spp S1 frame, its first-hit AOVs and srr_denoise with
the defaults come closer to the 1024-spp frame than the raw 16-spp frame does (the
frames are deterministic: per-path seeds), and render_main --denoise --aov-out
writes that same image plus the three AOV images.  Measured with the defaults (3
iterations, k_c 256, k_n 32, k_z 64, plain): MSE 0.00300995 against the raw frame's
0.00302784 (profiles/r08/denoise.txt)."""
import os
import subprocess

import numpy as np
import pytest

from srr import capi, scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "simple-raytracing-render_amd", "render_main")
NX = NY = 64


@pytest.fixture(scope="module")
def frames():
    r = capi.Renderer(scenes.s1_cornell()[0].text())
    noisy = r.render(NX, NY, 16, 50)["mean"]
    aov = r.render_aov(NX, NY, 16)
    shape = (NY, NX, 3)
    den = capi.denoise(noisy.reshape(shape), aov["albedo"].reshape(shape), aov["normal"].reshape(shape),
                       aov["depth"].reshape(NY, NX)).reshape(-1, 3)
    return r, noisy, den


def test_denoised_frame_is_closer_to_the_converged_one(frames):
    r, noisy, den = frames
    ref = r.render(NX, NY, 1024, 50)["mean"].astype(np.float64)
    mse_raw = float(((noisy - ref) ** 2).mean())
    mse_den = float(((den - ref) ** 2).mean())
    print(f"S1 {NX}x{NY}: MSE against 1024 spp: raw 16 spp {mse_raw:.5g}, denoised {mse_den:.5g}")
    assert np.isfinite(den).all()
    assert mse_den < mse_raw


def test_progressive_denoise_keeps_the_undenoised_sums(frames):
    from srr.progressive import Progressive
    r, noisy, den = frames
    text = scenes.s1_cornell()[0].text()
    pr = Progressive(capi.Renderer(text), NX, NY, denoise=True, aov_spp=16)
    pr.step(8)
    got = pr.step(8)
    np.testing.assert_array_equal(got.view(np.uint32), den.view(np.uint32))
    np.testing.assert_array_equal(pr.mean.view(np.uint32), noisy.view(np.uint32))
    plain = Progressive(capi.Renderer(text), NX, NY)
    plain.step(8)
    np.testing.assert_array_equal(plain.step(8).view(np.uint32), noisy.view(np.uint32))


def test_render_main_denoise(frames, tmp_path):
    _, _, den = frames
    out, prefix = str(tmp_path / "o.ppm"), str(tmp_path / "aov")
    r = subprocess.run([EXE, "--scene", "s1", "--nx", str(NX), "--ny", str(NY), "--ns", "16", "--denoise",
                        "--aov-out", prefix, "--out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want = str(tmp_path / "want.ppm")
    capi.write_ppm(want, NX, NY, capi.tonemap(den))
    assert open(out, "rb").read() == open(want, "rb").read()
    for k in ("albedo", "normal", "depth"):
        px, comp = capi.image_load(f"{prefix}_{k}.png")
        assert px.shape == (NY, NX, 3) and comp == 3, k
        assert px.max() > 0, k
    # a usage error, before any GPU work
    bad = subprocess.run([EXE, "--scene", "s1", "--denoise", "--gpus", "2"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2
