"""CPU: the numpy restatements of the emission-separated filters (tests/denoise_emission_ref.py)
against those of the base filters, the symbols and the refusals that need no GPU."""
import ctypes

import numpy as np
import pytest

import denoise_emission_ref as de
import denoise_ref as dn
import denoise_var_ref as dv
from srr import capi

f32 = np.float32
EINVAL = -22
NX, NY = 16, 12
K = (2.0, 128.0, 64.0)


def test_symbols():
    L = capi.lib()
    for fn in ("srr_render_aov_emission", "srr_render_aov_emission_host", "srr_denoise_emission",
               "srr_denoise_emission_host", "srr_denoise_var_emission", "srr_denoise_var_emission_host"):
        assert hasattr(L, fn), fn
    assert capi.AOV_EMISSION == 8


@pytest.mark.parametrize("flags", [0, de.DEMODULATE])
def test_zero_emission_is_the_base_filter(flags):
    """As values: y + 0 turns a -0 of the base filter into +0, so the bits may differ there."""
    color, albedo, normal, depth = dn.synthetic(NX, NY)
    var = dv.synthetic_var(NX, NY)
    zero = np.zeros_like(color)
    want = dn.denoise(color, albedo, normal, depth, 3, 4.0, 16.0, 64.0, flags)
    np.testing.assert_array_equal(de.denoise_emission(color, zero, albedo, normal, depth, 3, 4.0, 16.0, 64.0, flags), want)
    want, want_var = dv.denoise_var(color, var, albedo, normal, depth, 3, *K, flags)
    got, got_var = de.denoise_var_emission(color, var, zero, albedo, normal, depth, 3, *K, flags)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(de.bits(got_var), de.bits(want_var))


def _lit_room():
    """A 16 x 12 frame: random colour on a wall facing +z, and a block (the light) with a normal of its
    own, a random emission texture and a colour that equals it exactly.  With k_n = 128 a tap across
    the block's edge weighs rexp(-256) = 0."""
    rng = np.random.default_rng(5)
    color = rng.random((NY, NX, 3), dtype=f32)
    albedo = np.full((NY, NX, 3), f32(0.73))
    normal = np.zeros((NY, NX, 3), f32)
    normal[..., 2] = 1
    depth = np.full((NY, NX), f32(500.0))
    var = rng.random((NY, NX), dtype=f32) * f32(0.1)
    block = (slice(3, 8), slice(5, 12))
    emission = np.zeros((NY, NX, 3), f32)
    emission[block] = f32(10.0) + rng.random((5, 7, 3), dtype=f32) * f32(5.0)
    color[block] = emission[block]
    albedo[block] = emission[block]  # a light's albedo guide is its emission texture
    normal[block] = (0, -1, 0)
    return color, var, emission, albedo, normal, depth, block


@pytest.mark.parametrize("flags", [0, de.DEMODULATE])
def test_where_the_colour_is_the_emission_the_output_is_the_emission(flags):
    color, var, emission, albedo, normal, depth, block = _lit_room()
    for got in (de.denoise_emission(color, emission, albedo, normal, depth, 3, 4.0, K[1], K[2], flags),
                de.denoise_var_emission(color, var, emission, albedo, normal, depth, 3, *K, flags)[0]):
        np.testing.assert_array_equal(de.bits(got[block]), de.bits(emission[block]))
        assert np.isfinite(got).all()
        outside = np.ones((NY, NX), bool)
        outside[block] = False
        assert (de.bits(got[outside]) != de.bits(color[outside])).any()  # and the wall was filtered
    if not flags:  # unseparated, the plain filters blur the light's texture
        plain = dv.denoise_var(color, var, albedo, normal, depth, 3, *K, 0)[0]
        assert (de.bits(plain[block]) != de.bits(emission[block])).any()


# ------------------------------------------------------------ refusals (decided before the GPU is touched)
BUF = dict(color=0x100000, var=0x180000, emission=0x1c0000, albedo=0x200000, normal=0x300000, depth=0x400000,
           out=0x500000, var_out=0x580000)


def _call(fn, **over):
    b = dict(BUF, **over)
    L = capi.lib()
    if "var" in fn:
        dp = capi.DenoiseVarParams.defaults()
        order = ("color", "var", "emission", "albedo", "normal", "depth", "out", "var_out")
    else:
        dp = capi.DenoiseParams.defaults()
        order = ("color", "emission", "albedo", "normal", "depth", "out")
    return getattr(L, fn)(0, NX, NY, ctypes.byref(dp), *(b[k] or None for k in order))


@pytest.mark.parametrize("fn", ["srr_denoise_emission", "srr_denoise_emission_host", "srr_denoise_var_emission",
                                "srr_denoise_var_emission_host"])
def test_refusals(fn):
    assert _call(fn, emission=0) == EINVAL
    assert _call(fn, color=0) == EINVAL
    n3 = NX * NY * 3 * 4
    assert _call(fn, out=BUF["emission"]) == EINVAL                # the output on the emission
    assert _call(fn, out=BUF["emission"] + n3 - 4) == EINVAL       # ... on its last float
    assert _call(fn, out=BUF["emission"] - n3 + 4) == EINVAL       # ... ending on its first
    if "var" in fn:
        assert _call(fn, var_out=BUF["emission"] + 8) == EINVAL
