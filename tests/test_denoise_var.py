"""srr_denoise_var / srr_adaptive_variance without a GPU: the exported symbols and the
struct, every refusal of srr_denoise_var (decided before the GPU is touched),
srr_variance_of_mean against its numpy restatement, and the restatement of the
filter (tests/denoise_var_ref.py) on hand-checkable cases."""
import ctypes

import numpy as np
import pytest

import denoise_var_ref as dv
from srr import capi

EINVAL = -22
f32 = np.float32


def test_symbols_and_struct():
    L = capi.lib()
    for name in ("srr_variance_of_mean", "srr_adaptive_variance", "srr_adaptive_variance_host", "srr_denoise_var",
                 "srr_denoise_var_host", "srr_denoise_var_defaults"):
        assert hasattr(L, name), name
    assert ctypes.sizeof(capi.DenoiseVarParams) == 24
    dp = capi.DenoiseVarParams.defaults()
    assert dp.struct_size == 24
    assert 1 <= dp.iterations <= 6
    for k in (dp.k_l, dp.k_n, dp.k_z):
        assert k >= 0 and np.isfinite(k)
    assert dp.flags & ~capi.DENOISE_DEMODULATE == 0


# fake, distinct, non-overlapping "device" buffers of a 16 x 16 frame: a refusal never reads them
NX = NY = 16
BUF = dict(color=0x100000, var=0x180000, albedo=0x200000, normal=0x300000, depth=0x400000, out=0x500000,
           var_out=0x600000)
ORDER = ("color", "var", "albedo", "normal", "depth", "out", "var_out")


def _call(fn="srr_denoise_var", nx=NX, ny=NY, dp=None, **over):
    b = dict(BUF, **over)
    dp = dp if dp is not None else capi.DenoiseVarParams.defaults()
    return getattr(capi.lib(), fn)(0, nx, ny, ctypes.byref(dp), *(b[k] for k in ORDER))


@pytest.mark.parametrize("fn", ["srr_denoise_var", "srr_denoise_var_host"])
def test_refusals(fn):
    D = capi.DenoiseVarParams.defaults
    nan, inf = float("nan"), float("inf")
    n3, n1 = 4 * 3 * NX * NY, 4 * NX * NY  # bytes of a 3-float and of a 1-float image
    cases = {
        "nx 0": dict(nx=0), "ny 0": dict(ny=0), "nx < 0": dict(nx=-4), "too large": dict(nx=65536, ny=65536),
        "nx too wide": dict(nx=65537, ny=1),
        "iterations 0": dict(dp=D(iterations=0)), "iterations 7": dict(dp=D(iterations=7)),
        "k_l < 0": dict(dp=D(k_l=-1.0)), "k_n < 0": dict(dp=D(k_n=-0.5)), "k_z < 0": dict(dp=D(k_z=-2.0)),
        "k_l nan": dict(dp=D(k_l=nan)), "k_n nan": dict(dp=D(k_n=nan)), "k_z nan": dict(dp=D(k_z=nan)),
        "k_l inf": dict(dp=D(k_l=inf)), "k_n inf": dict(dp=D(k_n=inf)), "k_z inf": dict(dp=D(k_z=inf)),
        "unknown flag": dict(dp=D(flags=2)), "unknown flag with a known one": dict(dp=D(flags=5)),
        "struct_size": dict(dp=D(struct_size=20)),
        "null color": dict(color=None), "null var": dict(var=None), "null albedo": dict(albedo=None),
        "null normal": dict(normal=None), "null depth": dict(depth=None), "null out": dict(out=None),
        "out is color": dict(out=BUF["color"]), "out is var": dict(out=BUF["var"]),
        "out is albedo": dict(out=BUF["albedo"]), "out is normal": dict(out=BUF["normal"]),
        "out is depth": dict(out=BUF["depth"]),
        "out overlaps the end of color": dict(out=BUF["color"] + n3 - 4),
        "out ends inside depth": dict(out=BUF["depth"] - n3 + 4),
        "var_out is color": dict(var_out=BUF["color"]), "var_out is var": dict(var_out=BUF["var"]),
        "var_out is albedo": dict(var_out=BUF["albedo"]), "var_out is normal": dict(var_out=BUF["normal"]),
        "var_out is depth": dict(var_out=BUF["depth"]),
        "var_out is the last float of var": dict(var_out=BUF["var"] + n1 - 4),
        "var_out ends inside normal": dict(var_out=BUF["normal"] - n1 + 4),
        "var_out is out": dict(var_out=BUF["out"]),
        "var_out is the last float of out": dict(var_out=BUF["out"] + n3 - 4),
        "var_out ends inside out": dict(var_out=BUF["out"] - n1 + 4),
    }
    for name, kw in cases.items():
        assert _call(fn, **kw) == EINVAL, name
        assert capi.lib().srr_last_error(), name
    assert getattr(capi.lib(), fn)(0, NX, NY, None, *(BUF[k] for k in ORDER)) == EINVAL  # null params
    assert capi.lib().srr_denoise_var_defaults(None) == EINVAL


def test_adaptive_variance_refusals_that_need_no_renderer():
    L = capi.lib()
    assert L.srr_adaptive_variance(None, 16, 16) == EINVAL
    assert L.srr_adaptive_variance_host(None, 16, 16) == EINVAL


# ------------------------------------------------------------ the variance of the mean
def test_variance_of_mean_equals_the_restatement():
    rng = np.random.default_rng(5)
    nan = float("nan")
    for n in (0, 1, 2, 3, 1000, 2 ** 24):
        y = rng.random(64, dtype=f32) * f32(3.0)
        # plausible moments of n samples around y, moments of a constant pixel (d rounds to
        # about 0, either sign), s2*n < s1*s1 (d < 0), zeros, and NaN moments
        rows = [(f32(n) * y[i], f32(n) * y[i] * y[i] * f32(1.0 + 0.3 * (i % 5))) for i in range(64)]
        rows += [(f32(n) * y[i], f32(n) * (y[i] * y[i])) for i in range(8)]
        rows += [(f32(7.5), f32(0.25)), (f32(1e3), f32(1e-3)), (f32(0), f32(0)), (f32(2.0), f32(3.0))]
        rows += [(f32(nan), f32(1.0)), (f32(1.0), f32(nan)), (f32(nan), f32(nan))]
        s1 = np.array([r[0] for r in rows], f32)
        s2 = np.array([r[1] for r in rows], f32)
        want = dv.variance_of_mean(np.full(s1.size, n, np.int64), s1, s2)
        got = np.array([capi.variance_of_mean(n, a, b) for a, b in zip(s1, s2)], f32)
        same = (dv.bits(got) == dv.bits(want)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), (n, s1[~same], s2[~same], got[~same], want[~same])
    # the cases by hand
    assert capi.variance_of_mean(1, 3.0, 100.0) == f32(9.0)  # n < 2: s1*s1
    assert capi.variance_of_mean(0, 0.5, nan) == f32(0.25)
    assert capi.variance_of_mean(4, 8.0, 10.0) == f32(0.0)   # s2*n = 40 < s1*s1 = 64
    assert capi.variance_of_mean(4, nan, 1.0) == f32(0.0) and capi.variance_of_mean(4, 1.0, nan) == f32(0.0)
    # samples 1, 3: s1 = 4, s2 = 10, var(mean) = ((1 + 1) / 1) / 2 = 1: d = 20 - 16 = 4, 4 / (4 * 1)
    assert capi.variance_of_mean(2, 4.0, 10.0) == f32(1.0)


# ------------------------------------------------------------ the restatement of the filter
def _guides(nx, ny):
    normal = np.zeros((ny, nx, 3), f32)
    normal[..., 2] = 1
    return np.full((ny, nx, 3), f32(0.5)), normal, np.full((ny, nx), f32(100.0))


def test_synthetic_inputs_have_the_hard_values_and_a_finite_result():
    for nx, ny in ((1, 1), (3, 70), (37, 29), (64, 64)):
        color, albedo, normal, depth = dv.synthetic(nx, ny)
        var = dv.synthetic_var(nx, ny)
        assert var.dtype == f32 and var.shape == (ny, nx) and (var >= 0).all()
        assert (var == f32(1e30)).sum() == 1 and ((var < f32(0.5)) | (var == f32(1e30))).all()
        if nx * ny > 1:
            assert (var == 0).any() and (var == f32(1e-30)).any()
        if nx >= 8:
            assert ((var == 0) & (albedo[..., 0] == 0)).any()  # zero variance over zero albedo
        for flags in (0, dv.DEMODULATE):
            for it in (1, 5, 6):
                out, vout = dv.denoise_var(color, var, albedo, normal, depth, it, 4.0, 16.0, 64.0, flags)
                assert np.isfinite(out).all() and np.isfinite(vout).all(), (nx, ny, flags, it)
                assert out.dtype == f32 and vout.dtype == f32


@pytest.mark.parametrize("flags", [0, dv.DEMODULATE])
def test_constant_image_is_a_fixed_point_for_any_variance(flags):
    nx, ny = 13, 9
    albedo, normal, depth = _guides(nx, ny)
    # dl = dn = dz = 0 at every tap, whatever den is (den >= 1e-6f > 0): w = h exactly, and
    # with x = 0.75 (plain) or 1 (demodulated) every sum is a small dyadic rational
    color = albedo + f32(1e-3) if flags else np.full((ny, nx, 3), f32(0.75))
    var = dv.synthetic_var(nx, ny)
    out, vout = dv.denoise_var(color, var, albedo, normal, depth, 5, 4.0, 16.0, 64.0, flags)
    np.testing.assert_array_equal(dv.bits(out), dv.bits(color))
    assert np.isfinite(vout).all()


def test_zero_variance_keeps_distinct_luminances():
    nx, ny = 12, 10
    albedo, normal, depth = _guides(nx, ny)
    # luminances at least 0.01 * 0.2126 apart: den = 1e-6f, wl >= 2126, w = h * expf(-2126) = 0
    # off the centre; the centre gives sum / wsum = (h*x) / h, within an ulp or two of x
    grey = (f32(0.2) + f32(0.01) * np.arange(nx * ny, dtype=f32)).reshape(ny, nx)
    color = np.repeat(grey[..., None], 3, axis=2) * np.array([1.0, 0.9, 1.1], f32)
    var = np.zeros((ny, nx), f32)
    out, vout = dv.denoise_var(color, var, albedo, normal, depth, 4, 4.0, 0.0, 0.0, 0)
    np.testing.assert_allclose(out, color, rtol=1e-6, atol=0)
    np.testing.assert_array_equal(vout, 0)


def test_variance_of_a_flat_region_shrinks_by_the_kernel_s_sum_of_squares():
    nx, ny = 11, 9
    albedo, normal, depth = _guides(nx, ny)
    color = np.full((ny, nx, 3), f32(0.75))
    for v in (f32(0.5), f32(3.0), f32(2.0 ** -40)):
        var = np.full((ny, nx), v)
        _, vout = dv.denoise_var(color, var, albedo, normal, depth, 1, 4.0, 16.0, 64.0, 0)
        # w = h: wsum = 1, vsum = v * sum h^2 = v * (sum B^2)^2 = v * (70/256)^2 = v * 1225/16384,
        # every partial sum a dyadic rational of few bits times v: exact
        want = v * f32(1225 / 16384)
        np.testing.assert_array_equal(dv.bits(vout[2:-2, 2:-2]), dv.bits(np.full((ny - 4, nx - 4), want)))
        assert (vout[0, 0] > want)  # the corner averages fewer pixels
