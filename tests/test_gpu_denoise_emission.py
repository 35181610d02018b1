"""srr_denoise_emission and srr_denoise_var_emission on the GPU equal their numpy restatements
(tests/denoise_emission_ref.py) bit for bit: denoise_ref's synthetic inputs with an emission
block whose one half equals the colour exactly and whose other half exceeds it; sizes of a
single tap, narrower than the steps, no multiple of the 32 x 8 tile, and of 3 x 6 blocks;
iterations 1, 3 and 5 run the LDS tile alone, both tiles, and the tiles and the direct gather."""
import ctypes
import functools

import numpy as np
import pytest

import denoise_emission_ref as de
import denoise_var_ref as dv
from srr import capi

pytestmark = pytest.mark.gpu

K = (4.0, 16.0, 64.0)
EINVAL = -22
SIZES = [(1, 1), (5, 3), (33, 9), (70, 41)]


@functools.lru_cache(maxsize=None)
def _inputs(nx, ny):
    color, albedo, normal, depth = dv.synthetic(nx, ny)
    arrays = (color, albedo, normal, depth, dv.synthetic_var(nx, ny), de.synthetic_emission(nx, ny, color))
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _assert_bits(got, want, what, nx):
    diff = de.bits(got) != de.bits(want)
    bad = np.flatnonzero(diff.reshape(diff.shape[0] * diff.shape[1], -1).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} pixels differ, first at {divmod(int(bad[0]), nx)[::-1]}"


@pytest.mark.parametrize("iterations", [1, 3, 5])
@pytest.mark.parametrize("flags", [0, de.DEMODULATE])
@pytest.mark.parametrize("nx,ny", SIZES)
def test_colour_filter_is_bit_equal_to_the_restatement(nx, ny, flags, iterations):
    color, albedo, normal, depth, _, emission = _inputs(nx, ny)
    dp = capi.DenoiseParams.defaults(iterations=iterations, k_c=K[0], k_n=K[1], k_z=K[2], flags=flags)
    got = capi.denoise(color, albedo, normal, depth, dp, emission=emission)
    want = de.denoise_emission(color, emission, albedo, normal, depth, iterations, *K, flags)
    assert np.isfinite(want).all()
    _assert_bits(got, want, "colour", nx)


@pytest.mark.parametrize("iterations", [1, 3, 5])
@pytest.mark.parametrize("flags", [0, de.DEMODULATE])
@pytest.mark.parametrize("nx,ny", SIZES)
def test_variance_filter_is_bit_equal_to_the_restatement(nx, ny, flags, iterations):
    color, albedo, normal, depth, var, emission = _inputs(nx, ny)
    dp = capi.DenoiseVarParams.defaults(iterations=iterations, k_l=K[0], k_n=K[1], k_z=K[2], flags=flags)
    got, got_var = capi.denoise_var(color, var, albedo, normal, depth, dp, emission=emission)
    want, want_var = de.denoise_var_emission(color, var, emission, albedo, normal, depth, iterations, *K, flags)
    assert np.isfinite(want).all() and np.isfinite(want_var).all()
    _assert_bits(got, want, "colour", nx)
    _assert_bits(got_var, want_var, "variance", nx)
    if (nx, ny) == (70, 41) and iterations == 3:  # the emission matters, and a NULL var_out changes nothing
        base, _ = capi.denoise_var(color, var, albedo, normal, depth, dp)
        assert (de.bits(base) != de.bits(got)).any()
        again, none = capi.denoise_var(color, var, albedo, normal, depth, dp, want_var=False, emission=emission)
        assert none is None
        _assert_bits(again, want, "colour", nx)


def test_device_buffers_and_refusals():
    import torch
    nx, ny = 33, 9
    color, albedo, normal, depth, var, emission = _inputs(nx, ny)
    L = capi.lib()
    dev = {k: torch.from_numpy(np.array(a)).cuda() for k, a in
           dict(color=color, var=var, emission=emission, albedo=albedo, normal=normal, depth=depth).items()}
    out = torch.zeros(ny, nx, 3, device="cuda")
    var_out = torch.zeros(ny, nx, device="cuda")
    torch.cuda.synchronize()
    ptr = {k: t.data_ptr() for k, t in dev.items()}
    dp = capi.DenoiseParams.defaults(iterations=3, k_c=K[0], k_n=K[1], k_z=K[2], flags=0)
    dvp = capi.DenoiseVarParams.defaults(iterations=3, k_l=K[0], k_n=K[1], k_z=K[2], flags=de.DEMODULATE)

    def colour(emission=ptr["emission"], o=out.data_ptr()):
        return L.srr_denoise_emission(0, nx, ny, ctypes.byref(dp), ptr["color"], emission, ptr["albedo"], ptr["normal"],
                                      ptr["depth"], o)

    def variance(emission=ptr["emission"], o=out.data_ptr(), vo=var_out.data_ptr()):
        return L.srr_denoise_var_emission(0, nx, ny, ctypes.byref(dvp), ptr["color"], ptr["var"], emission,
                                          ptr["albedo"], ptr["normal"], ptr["depth"], o, vo)
    assert colour(emission=None) == EINVAL and variance(emission=None) == EINVAL
    assert colour(o=ptr["emission"]) == EINVAL and variance(o=ptr["emission"]) == EINVAL
    assert colour(o=ptr["emission"] + 4 * (3 * nx * ny - 1)) == EINVAL
    assert variance(vo=ptr["emission"] + 8) == EINVAL
    assert (out == 0).all()  # refusals never write
    assert colour() == 0
    _assert_bits(out.cpu().numpy(), de.denoise_emission(color, emission, albedo, normal, depth, 3, *K, 0), "colour", nx)
    assert variance() == 0
    want, want_var = de.denoise_var_emission(color, var, emission, albedo, normal, depth, 3, *K, de.DEMODULATE)
    _assert_bits(out.cpu().numpy(), want, "colour", nx)
    _assert_bits(var_out.cpu().numpy(), want_var, "variance", nx)
