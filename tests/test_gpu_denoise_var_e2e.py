"""End to end on the GPU: a 16-spp S1 frame rendered as one adaptive pass (rel_tol 0:
bitwise the fixed-spp frame, and it keeps the luminance moments), its per-pixel
variance, its first-hit AOVs and srr_denoise_var with the defaults come closer to the
1024-spp frame than the raw 16-spp frame does (the frames are deterministic: per-path
seeds), and render_main --denoise-var writes that same image.  Measured with the defaults
(3 iterations, k_l 2, k_n 128, k_z 64, demodulated): MSE 0.0030122 against the raw
frame's 0.0030278; srr_denoise's defaults give 0.0030100 (profiles/r12/denoise_var.txt)."""
import os
import subprocess

import numpy as np
import pytest

from srr import capi, scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "simple-raytracing-render_amd", "render_main")
NX = NY = 64
SPP = 16


@pytest.fixture(scope="module")
def frames():
    r = capi.Renderer(scenes.s1_cornell()[0].text())
    out = r.render_adaptive(NX, NY, SPP, 50, batch_spp=SPP, min_spp=SPP, rel_tol=0.0, tile=1)
    noisy = out["mean"]
    var = r.adaptive_variance(out["count"])
    aov = r.render_aov(NX, NY, SPP)
    shape = (NY, NX, 3)
    img = [noisy.reshape(shape), aov["albedo"].reshape(shape), aov["normal"].reshape(shape),
           aov["depth"].reshape(NY, NX)]
    den_var, var_out = capi.denoise_var(img[0], var.reshape(NY, NX), *img[1:])
    den = capi.denoise(*img)
    return r, noisy, var, den_var.reshape(-1, 3), var_out.reshape(-1), den.reshape(-1, 3)


def test_denoised_frame_is_closer_to_the_converged_one(frames):
    r, noisy, var, den_var, var_out, den = frames
    fixed = r.render(NX, NY, SPP, 50)["mean"]
    np.testing.assert_array_equal(noisy.view(np.uint32), fixed.view(np.uint32))  # the rel_tol-0 route
    ref = r.render(NX, NY, 1024, 50)["mean"].astype(np.float64)
    mse_raw = float(((noisy - ref) ** 2).mean())
    mse_var = float(((den_var - ref) ** 2).mean())
    mse_den = float(((den - ref) ** 2).mean())
    print(f"S1 {NX}x{NY}: MSE against 1024 spp: raw {SPP} spp {mse_raw:.6g}, srr_denoise_var {mse_var:.6g}, "
          f"srr_denoise {mse_den:.6g}")
    assert np.isfinite(den_var).all() and np.isfinite(var_out).all()
    assert (var >= 0).all() and (var > 0).any()
    assert mse_var < mse_raw


def test_render_main_denoise_var(frames, tmp_path):
    den_var = frames[3]
    out = str(tmp_path / "o.ppm")
    r = subprocess.run([EXE, "--scene", "s1", "--nx", str(NX), "--ny", str(NY), "--ns", str(SPP), "--denoise-var",
                        "--out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want = str(tmp_path / "want.ppm")
    capi.write_ppm(want, NX, NY, capi.tonemap(den_var))
    assert open(out, "rb").read() == open(want, "rb").read()
    # usage errors, before any GPU work
    for bad in (["--denoise", "--denoise-var"], ["--denoise-var", "--gpus", "2"]):
        assert subprocess.run([EXE, "--scene", "s1", *bad], capture_output=True, text=True, timeout=60).returncode == 2
