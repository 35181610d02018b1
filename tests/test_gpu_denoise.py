"""srr_denoise on the GPU equals its numpy restatement (tests/denoise_ref.py) bit
for bit: synthetic inputs with guide edges and pixels of zero normal and depth;
sizes that are no multiple of the 32 x 8 tile, smaller than the filter's steps, and
of more than one block; 5 iterations run steps 1..16, hence both kernel variants
(the LDS tile at steps 1 and 2, the direct gather above)."""
import numpy as np
import pytest

import denoise_ref as dr
from srr import capi

pytestmark = pytest.mark.gpu

K = (4.0, 16.0, 64.0)


def _run(nx, ny, iterations, flags, k=K):
    color, albedo, normal, depth = dr.synthetic(nx, ny)
    dp = capi.DenoiseParams.defaults(iterations=iterations, k_c=k[0], k_n=k[1], k_z=k[2], flags=flags)
    got = capi.denoise(color, albedo, normal, depth, dp)
    want = dr.denoise(color, albedo, normal, depth, iterations, *k, flags)
    assert np.isfinite(want).all()
    bad = np.flatnonzero((dr.bits(got) != dr.bits(want)).any(axis=2).ravel())
    assert bad.size == 0, f"{bad.size} of {nx * ny} pixels differ, first at {divmod(int(bad[0]), nx)[::-1]}"
    return got, color


@pytest.mark.parametrize("flags", [0, dr.DEMODULATE])
@pytest.mark.parametrize("nx,ny", [(1, 1), (3, 70), (37, 29), (64, 64)])
def test_bit_equal_to_the_restatement(nx, ny, flags):
    got, color = _run(nx, ny, 5, flags)
    if nx * ny > 1:
        assert (dr.bits(got) != dr.bits(color)).any()  # it filtered


@pytest.mark.parametrize("iterations", [1, 6])
def test_iteration_counts(iterations):
    _run(37, 29, iterations, dr.DEMODULATE)


def test_zero_strengths_and_device_buffers():
    """k = 0 (the plain blur) through srr_denoise itself on device buffers, twice:
    the cached scratch of the second call gives the same image."""
    import ctypes

    import torch
    nx, ny = 45, 19
    color, albedo, normal, depth = dr.synthetic(nx, ny)
    dev = [torch.from_numpy(a).cuda() for a in (color, albedo, normal, depth)]
    out = torch.zeros(ny, nx, 3, device="cuda")
    torch.cuda.synchronize()
    dp = capi.DenoiseParams.defaults(iterations=3, k_c=0.0, k_n=0.0, k_z=0.0, flags=0)
    want = dr.denoise(color, albedo, normal, depth, 3, 0.0, 0.0, 0.0, 0)
    for _ in range(2):
        capi._check(capi.lib().srr_denoise(0, nx, ny, ctypes.byref(dp), *(t.data_ptr() for t in dev), out.data_ptr()))
        np.testing.assert_array_equal(dr.bits(out.cpu().numpy()), dr.bits(want))
        out.zero_()
        torch.cuda.synchronize()
