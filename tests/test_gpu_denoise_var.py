"""srr_denoise_var on the GPU equals its numpy restatement (tests/denoise_var_ref.py)
bit for bit, colour and variance: denoise_ref's synthetic guides with a variance image
that holds exact zeros, 1e30f, 1e-30f and zero variance over zero albedo; sizes of a
single tap, narrower than the steps, no multiple of the 32 x 8 tile, and of 2 x 8
blocks; 5 iterations run steps 1..16, hence both kernel variants (the LDS tile at
steps 1 and 2, the direct gather above)."""
import ctypes
import functools

import numpy as np
import pytest

import denoise_var_ref as dv
from srr import capi

pytestmark = pytest.mark.gpu

K = (4.0, 16.0, 64.0)


@functools.lru_cache(maxsize=None)
def _inputs(nx, ny):
    arrays = (*dv.synthetic(nx, ny), dv.synthetic_var(nx, ny))
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _want(nx, ny, iterations, flags, k=K):
    """The restatement's (colour, variance), computed once per case and shared."""
    color, albedo, normal, depth, var = _inputs(nx, ny)
    want = dv.denoise_var(color, var, albedo, normal, depth, iterations, *k, flags)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    for a in want:
        a.setflags(write=False)
    return want


def _assert_bits(got, want, what, nx):
    diff = dv.bits(got) != dv.bits(want)
    bad = np.flatnonzero(diff.reshape(diff.shape[0] * diff.shape[1], -1).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} pixels differ, first at {divmod(int(bad[0]), nx)[::-1]}"


def _run(nx, ny, iterations, flags, k=K):
    color, albedo, normal, depth, var = _inputs(nx, ny)
    dp = capi.DenoiseVarParams.defaults(iterations=iterations, k_l=k[0], k_n=k[1], k_z=k[2], flags=flags)
    got, got_var = capi.denoise_var(color, var, albedo, normal, depth, dp)
    want, want_var = _want(nx, ny, iterations, flags, k)
    _assert_bits(got, want, "colour", nx)
    _assert_bits(got_var, want_var, "variance", nx)
    return got, got_var


@pytest.mark.parametrize("flags", [0, dv.DEMODULATE])
@pytest.mark.parametrize("nx,ny", [(1, 1), (3, 70), (37, 29), (64, 64)])
def test_bit_equal_to_the_restatement(nx, ny, flags):
    got, got_var = _run(nx, ny, 5, flags)
    if nx * ny > 1:
        color, _, _, _, var = _inputs(nx, ny)
        assert (dv.bits(got) != dv.bits(color)).any() and (dv.bits(got_var) != dv.bits(var)).any()  # it filtered


@pytest.mark.parametrize("iterations", [1, 6])
def test_iteration_counts(iterations):
    _run(37, 29, iterations, dv.DEMODULATE)


@pytest.mark.parametrize("flags", [0, dv.DEMODULATE])
def test_null_var_out_gives_the_same_colour(flags):
    nx, ny = 37, 29
    color, albedo, normal, depth, var = _inputs(nx, ny)
    dp = capi.DenoiseVarParams.defaults(iterations=5, k_l=K[0], k_n=K[1], k_z=K[2], flags=flags)
    got, none = capi.denoise_var(color, var, albedo, normal, depth, dp, want_var=False)
    assert none is None
    _assert_bits(got, _want(nx, ny, 5, flags)[0], "colour", nx)


def test_zero_strengths_and_device_buffers():
    """All k = 0 through srr_denoise_var itself on device buffers, twice: the cached
    scratch of the second call gives the same images.  With k_n = k_z = 0 the guides
    do not matter; k_l = 0 leaves den = 1e-6f (the header's definition), so what is
    left is the plain B3 blur among pixels of one luminance: on a constant colour it
    is the plain blur of the variance, w = h at every tap."""
    import torch
    nx, ny = 45, 19
    color, albedo, normal, depth, var = _inputs(nx, ny)
    flat = np.full((ny, nx, 3), np.float32(0.75))
    for c in (color, flat):
        dev = [torch.from_numpy(np.array(a)).cuda() for a in (c, var, albedo, normal, depth)]
        out = torch.zeros(ny, nx, 3, device="cuda")
        var_out = torch.zeros(ny, nx, device="cuda")
        torch.cuda.synchronize()
        dp = capi.DenoiseVarParams.defaults(iterations=3, k_l=0.0, k_n=0.0, k_z=0.0, flags=0)
        want, want_var = dv.denoise_var(c, var, albedo, normal, depth, 3, 0.0, 0.0, 0.0, 0)
        for _ in range(2):
            capi._check(capi.lib().srr_denoise_var(0, nx, ny, ctypes.byref(dp), *(t.data_ptr() for t in dev),
                                                   out.data_ptr(), var_out.data_ptr()))
            np.testing.assert_array_equal(dv.bits(out.cpu().numpy()), dv.bits(want))
            np.testing.assert_array_equal(dv.bits(var_out.cpu().numpy()), dv.bits(want_var))
            out.zero_()
            var_out.zero_()
            torch.cuda.synchronize()
    # the flat colour came back as it was, and its variance is the h^2-weighted plain blur
    np.testing.assert_array_equal(dv.bits(want), dv.bits(flat))
    assert (want_var != var).any()
