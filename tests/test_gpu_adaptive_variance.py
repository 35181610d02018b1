"""srr_adaptive_variance on the GPU: on adaptive_ref's parity frame the variance of
every pixel's mean luminance is bit-equal to the numpy restatement
(tests/denoise_var_ref.py) applied to the float32 folds of the CPU oracle's paths over
each pixel's own samples; the call is refused without a valid adaptive frame, and no
other render entry disturbs the moments."""
import numpy as np
import pytest

import adaptive_ref as ar
import denoise_var_ref as dv
from srr import capi

pytestmark = pytest.mark.gpu

ADAPTIVE = dict(batch_spp=ar.BATCH, min_spp=ar.MIN_SPP, rel_tol=ar.REL_TOL, abs_eps=ar.ABS_EPS)


@pytest.fixture(scope="module")
def text():
    return ar.scene_text()


def _want(count, pixels=None):
    """The restatement over the oracle's luminances of each pixel's first count[i] paths."""
    y = ar.luminance(ar.oracle_frame()["paths"])
    if pixels is not None:
        y = y[pixels]
    s1, s2 = dv.fold_moments(y, count)
    return dv.variance_of_mean(count, s1, s2)


def test_parity_frame_is_bit_equal_to_the_restatement(text):
    r = capi.Renderer(text)
    out = r.render_adaptive(ar.NX, ar.NY, ar.BUDGET, 50, **ADAPTIVE)
    count = out["count"]
    np.testing.assert_array_equal(count, ar.expected_counts()[0])
    assert np.unique(count).size >= 3
    var = r.adaptive_variance(count)
    want = _want(count)
    assert np.isfinite(want).all() and (want > 0).any()
    np.testing.assert_array_equal(dv.bits(var), dv.bits(want))
    # a fixed-spp frame in between uses other buffers: the moments are still the adaptive frame's
    p = capi.make_params(ar.NX, ar.NY, 3, 50)
    import torch
    d_mean = torch.zeros(ar.NX * ar.NY, 3, device="cuda:0")
    r.render_device(p, d_mean.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dv.bits(r.adaptive_variance(count)), dv.bits(want))
    # and the device-pointer entry writes the same
    d_count = torch.from_numpy(count.copy()).cuda()
    d_var = torch.zeros(count.size, device="cuda:0")
    torch.cuda.synchronize()
    r.adaptive_variance_device(d_count.data_ptr(), d_var.data_ptr())
    np.testing.assert_array_equal(dv.bits(d_var.cpu().numpy()), dv.bits(want))


def test_zero_tolerance_frame(text):
    """rel_tol = 0: one decision, at the budget; every pixel holds all its samples."""
    r = capi.Renderer(text)
    out = r.render_adaptive(ar.NX, ar.NY, ar.BUDGET, 50, batch_spp=ar.BUDGET, min_spp=ar.BUDGET, rel_tol=0.0)
    assert (out["count"] == ar.BUDGET).all() and out["stats"]["passes"] == 1
    np.testing.assert_array_equal(dv.bits(r.adaptive_variance(out["count"])), dv.bits(_want(out["count"])))


def test_shard_is_a_slice_of_the_whole_frame(text):
    p = capi.make_params(ar.NX, ar.NY, ar.BUDGET, 50, shard=(1, 2), tile=8)
    px = capi.shard_pixels(p)
    assert 0 < px.size < ar.NX * ar.NY
    r = capi.Renderer(text)
    out = r.render_adaptive(ar.NX, ar.NY, ar.BUDGET, 50, shard=(1, 2), tile=8, **ADAPTIVE)
    np.testing.assert_array_equal(out["count"], ar.expected_counts()[0][px])
    var = r.adaptive_variance(out["count"])
    assert var.shape == (px.size,)
    np.testing.assert_array_equal(dv.bits(var), dv.bits(_want(out["count"], px)))


def test_refusals_leave_the_renderer_usable(text):
    nx, ny = 16, 12
    count = np.full(nx * ny, 8, np.int32)
    r = capi.Renderer(text)
    with pytest.raises(capi.SrrError):  # a fresh renderer: no adaptive frame
        r.adaptive_variance(count)
    with pytest.raises(capi.SrrError):  # an adaptive call that was itself refused leaves none either
        r.render_adaptive(nx, ny, 8, 50, batch_spp=0)
    with pytest.raises(capi.SrrError):
        r.adaptive_variance(count)
    r.render(nx, ny, 4, 50)  # a fixed-spp frame is no adaptive frame
    with pytest.raises(capi.SrrError):
        r.adaptive_variance(count)
    L = capi.lib()
    assert L.srr_adaptive_variance_host(r.h, None, count.ctypes.data) == -22
    assert L.srr_adaptive_variance(r.h, None, None) == -22
    # still usable: a frame, and then its variance
    out = r.render_adaptive(nx, ny, 8, 50, batch_spp=4, min_spp=4, rel_tol=0.1)
    var = r.adaptive_variance(out["count"])
    assert np.isfinite(var).all() and (var > 0).any()
    want = capi.Renderer(text).render_adaptive(nx, ny, 8, 50, batch_spp=4, min_spp=4, rel_tol=0.1)
    np.testing.assert_array_equal(dv.bits(out["mean"]), dv.bits(want["mean"]))
    # a refused adaptive call after a valid frame never started: the frame's moments stay
    with pytest.raises(capi.SrrError):
        r.render_adaptive(nx, ny, 8, 50, rel_tol=-1.0)
    np.testing.assert_array_equal(dv.bits(r.adaptive_variance(out["count"])), dv.bits(var))
    multi = capi.Renderer(text, devices=[0, 0])  # the one-GPU rehearsal of a multi-device renderer
    with pytest.raises(capi.SrrError):
        multi.adaptive_variance(count)
