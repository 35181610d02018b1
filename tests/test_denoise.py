"""srr_denoise / srr_render_aov without a GPU: the exported symbols and the struct,
every refusal of srr_denoise (decided before the GPU is touched), and the numpy
restatement of the filter (tests/denoise_ref.py) on hand-checkable cases."""
import ctypes

import numpy as np
import pytest

import denoise_ref as dr
from srr import capi

EINVAL = -22
f32 = np.float32


def test_symbols_and_struct():
    L = capi.lib()
    for name in ("srr_render_aov", "srr_render_aov_host", "srr_denoise", "srr_denoise_host", "srr_denoise_defaults"):
        assert hasattr(L, name), name
    assert ctypes.sizeof(capi.DenoiseParams) == 24
    dp = capi.DenoiseParams.defaults()
    assert dp.struct_size == 24
    assert 1 <= dp.iterations <= 6
    assert dp.k_c >= 0 and dp.k_n >= 0 and dp.k_z >= 0
    assert dp.flags & ~capi.DENOISE_DEMODULATE == 0
    assert (capi.AOV_ALBEDO, capi.AOV_NORMAL, capi.AOV_DEPTH, dr.DEMODULATE) == (1, 2, 4, capi.DENOISE_DEMODULATE)


# fake, distinct, non-overlapping "device" buffers of a 16 x 16 frame: a refusal never reads them
NX = NY = 16
BUF = dict(color=0x100000, albedo=0x200000, normal=0x300000, depth=0x400000, out=0x500000)


def _call(fn="srr_denoise", nx=NX, ny=NY, dp=None, **over):
    b = dict(BUF, **over)
    dp = dp if dp is not None else capi.DenoiseParams.defaults()
    return getattr(capi.lib(), fn)(0, nx, ny, ctypes.byref(dp) if dp else None, b["color"], b["albedo"], b["normal"],
                                   b["depth"], b["out"])


@pytest.mark.parametrize("fn", ["srr_denoise", "srr_denoise_host"])
def test_refusals(fn):
    D = capi.DenoiseParams.defaults
    nan, inf = float("nan"), float("inf")
    cases = {
        "nx 0": dict(nx=0), "ny 0": dict(ny=0), "nx < 0": dict(nx=-4), "too large": dict(nx=65536, ny=65536),
        "nx too wide": dict(nx=65537, ny=1),
        "iterations 0": dict(dp=D(iterations=0)), "iterations 7": dict(dp=D(iterations=7)),
        "k_c < 0": dict(dp=D(k_c=-1.0)), "k_n < 0": dict(dp=D(k_n=-0.5)), "k_z < 0": dict(dp=D(k_z=-2.0)),
        "k_c nan": dict(dp=D(k_c=nan)), "k_n nan": dict(dp=D(k_n=nan)), "k_z nan": dict(dp=D(k_z=nan)),
        "k_c inf": dict(dp=D(k_c=inf)), "k_n inf": dict(dp=D(k_n=inf)), "k_z inf": dict(dp=D(k_z=inf)),
        "unknown flag": dict(dp=D(flags=2)), "unknown flag with a known one": dict(dp=D(flags=5)),
        "struct_size": dict(dp=D(struct_size=20)),
        "null color": dict(color=None), "null albedo": dict(albedo=None), "null normal": dict(normal=None),
        "null depth": dict(depth=None), "null out": dict(out=None),
        "out is color": dict(out=BUF["color"]), "out is albedo": dict(out=BUF["albedo"]),
        "out is normal": dict(out=BUF["normal"]), "out is depth": dict(out=BUF["depth"]),
        "out overlaps the end of color": dict(out=BUF["color"] + 4 * (3 * NX * NY - 1)),
        "out ends inside depth": dict(out=BUF["depth"] - 4 * (3 * NX * NY - 1)),
    }
    for name, kw in cases.items():
        assert _call(fn, **kw) == EINVAL, name
        assert capi.lib().srr_last_error(), name
    assert getattr(capi.lib(), fn)(0, NX, NY, None, *BUF.values()) == EINVAL  # null params
    assert capi.lib().srr_denoise_defaults(None) == EINVAL


def test_aov_refusals_that_need_no_renderer():
    L = capi.lib()
    p = capi.make_params(8, 8, 4)
    assert L.srr_render_aov(None, ctypes.byref(p), 7, 16, 16, 16) == EINVAL
    assert L.srr_render_aov_host(None, ctypes.byref(p), 7, 16, 16, 16) == EINVAL


# ------------------------------------------------------------ the restatement
def _guides(nx, ny):
    normal = np.zeros((ny, nx, 3), f32)
    normal[..., 2] = 1
    return np.full((ny, nx, 3), f32(0.5)), normal, np.full((ny, nx), f32(100.0))


@pytest.mark.parametrize("flags", [0, dr.DEMODULATE])
def test_constant_image_is_a_fixed_point(flags):
    nx, ny = 13, 9
    albedo, normal, depth = _guides(nx, ny)
    # every tap sees dc = dn = dz = 0, so w = h = k / 1024 with a small integer k; with
    # x = 0.75 (plain) or x = c / (a + 1e-3f) = 1 (demodulated) every product w * x and
    # every partial sum is a small dyadic rational, hence exact, and sum / wsum = x
    color = albedo + f32(1e-3) if flags else np.full((ny, nx, 3), f32(0.75))
    out = dr.denoise(color, albedo, normal, depth, 5, 4.0, 16.0, 64.0, flags)
    np.testing.assert_array_equal(dr.bits(out), dr.bits(color))


def test_zero_strengths_give_the_b3_blur_with_border_renormalisation():
    nx, ny = 11, 7
    rng = np.random.default_rng(3)
    color = rng.random((ny, nx, 3), dtype=f32)
    albedo, normal, depth = _guides(nx, ny)
    normal = rng.random((ny, nx, 3), dtype=f32)  # the guides must not matter
    depth = rng.random((ny, nx), dtype=f32) * f32(50.0)
    out = dr.denoise(color, albedo, normal, depth, 1, 0.0, 0.0, 0.0, 0)
    k1 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625])
    want = np.zeros((ny, nx, 3))
    for y in range(ny):
        for x in range(nx):
            acc, ws = np.zeros(3), 0.0
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if 0 <= y + dy < ny and 0 <= x + dx < nx:
                        h = k1[dy + 2] * k1[dx + 2]
                        acc += h * color[y + dy, x + dx].astype(np.float64)
                        ws += h
            want[y, x] = acc / ws
    # float32 sums of 25 terms in [0, 1) against float64: 25 roundings of 6e-8, one division
    np.testing.assert_allclose(out, want, rtol=0, atol=4e-6)
    # the corner's weight sum is (0.375 + 0.25 + 0.0625)^2 of the full kernel's: renormalised, not darkened
    flat = dr.denoise(np.ones((ny, nx, 3), f32), albedo, normal, depth, 1, 0.0, 0.0, 0.0, 0)
    np.testing.assert_array_equal(dr.bits(flat), dr.bits(np.ones((ny, nx, 3), f32)))


def test_a_huge_k_n_leaves_the_sides_of_a_normal_edge_unmixed():
    nx, ny = 16, 6
    albedo, normal, depth = _guides(nx, ny)
    normal[:, nx // 2:] = (1, 0, 0)  # dn = 2 across the edge: w = h * expf(-2e6) = 0
    color = np.zeros((ny, nx, 3), f32)
    color[:, : nx // 2] = 1
    color[:, nx // 2:] = 3
    out = dr.denoise(color, albedo, normal, depth, 3, 0.0, 1e6, 0.0, 0)
    np.testing.assert_array_equal(dr.bits(out), dr.bits(color))
    mixed = dr.denoise(color, albedo, normal, depth, 3, 0.0, 0.0, 0.0, 0)
    assert (mixed[:, nx // 2 - 1] > 1).all() and (mixed[:, nx // 2] < 3).all()
