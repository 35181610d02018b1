"""numpy float32 restatement of srr_variance_of_mean and srr_denoise_var
(include/srr_capi.h): every operation in float32, in the header's order, the taps
visited (dy, dx) row-major; numpy's float32 +, -, *, / and sqrt are the IEEE
operations (no FMA) and the exponential is the host libm's expf, so the device
outputs must equal these bit for bit.  Test infrastructure: shared by
test_denoise_var.py (CPU) and the GPU tests."""
import numpy as np

import oracle_bind as ob
from denoise_ref import B, DEMODULATE, _sq3, bits, synthetic  # noqa: F401  (bits, synthetic: for the tests)

f32 = np.float32
G = (f32(0.25), f32(0.125), f32(0.0625))  # centre, edge, corner of the 3 x 3 prefilter


def variance_of_mean(n, s1, s2):
    """n [...] int, s1, s2 [...] float32 -> the variance of the mean, float32, elementwise."""
    n = np.asarray(n)
    s1 = np.asarray(s1, f32)
    s2 = np.asarray(s2, f32)
    nf = n.astype(f32)
    with np.errstate(all="ignore"):
        d = s2 * nf - s1 * s1
        d = np.where(d > 0, d, f32(0))  # (!(d > 0): a NaN too)
        v = d / ((nf * nf) * (nf - f32(1.0)))
        return np.where(n < 2, s1 * s1, v).astype(f32)


def fold_moments(y, count):
    """The luminance moments of the adaptive fold: y [npix, >= max(count)] float32
    samples, folded in sample order in float32 over each pixel's first count[i]."""
    y = np.asarray(y, f32)
    s1 = np.zeros(y.shape[0], f32)
    s2 = np.zeros(y.shape[0], f32)
    with np.errstate(all="ignore"):
        for s in range(int(count.max())):
            on = count > s
            s1[on] = s1[on] + y[on, s]
            s2[on] = s2[on] + y[on, s] * y[on, s]
    return s1, s2


def lum(x):
    return (f32(0.2126) * x[..., 0] + f32(0.7152) * x[..., 1]) + f32(0.0722) * x[..., 2]


def _windows(ny, nx, dy, dx):
    """The pixels P whose tap Q = P + (dx, dy) lies inside the image, as slices (or None)."""
    y0, y1 = max(0, -dy), min(ny, ny - dy)
    x0, x1 = max(0, -dx), min(nx, nx - dx)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def denoise_var(color, var, albedo, normal, depth, iterations, k_l, k_n, k_z, flags=0):
    """color, albedo, normal: [ny, nx, 3]; var, depth: [ny, nx] -> (out [ny, nx, 3], var_out [ny, nx])."""
    c = np.ascontiguousarray(color, f32)
    v = np.ascontiguousarray(var, f32).copy()
    a = np.ascontiguousarray(albedo, f32)
    n = np.ascontiguousarray(normal, f32)
    z = np.ascontiguousarray(depth, f32)
    ny, nx = z.shape
    k_l, k_n, k_z = f32(k_l), f32(k_n), f32(k_z)
    with np.errstate(all="ignore"):
        if flags & DEMODULATE:
            m = a + f32(1e-3)
            x = c / m
            la = lum(m)
            v = v / (la * la)
        else:
            x = c.copy()
        for k in range(iterations):
            s = 1 << k
            gs = np.zeros((ny, nx), f32)
            gw = np.zeros((ny, nx), f32)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    win = _windows(ny, nx, dy, dx)
                    if win is None:
                        continue
                    P, Q = win
                    g = G[abs(dx) + abs(dy)]
                    gs[P] += g * v[Q]
                    gw[P] += g
            vbar = gs / gw
            den = k_l * np.sqrt(vbar) + f32(1e-6)
            assert den.dtype == f32
            lx = lum(x)
            total = np.zeros((ny, nx, 3), f32)
            wsum = np.zeros((ny, nx), f32)
            vsum = np.zeros((ny, nx), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    win = _windows(ny, nx, s * dy, s * dx)
                    if win is None:
                        continue
                    P, Q = win
                    h = B[abs(dx)] * B[abs(dy)]
                    dl = np.abs(lx[Q] - lx[P])
                    wl = dl / den[P]
                    dn = _sq3(n[Q], n[P])
                    zp, zq = z[P], z[Q]
                    dz = ((zp - zq) * (zp - zq)) / ((zp * zp + zq * zq) + f32(1e-20))
                    arg = -((wl + dn * k_n) + dz * k_z)
                    w = h * ob.libm("expf", arg)
                    total[P] += w[..., None] * x[Q]
                    wsum[P] += w
                    vsum[P] += (w * w) * v[Q]
            x = total / wsum[..., None]
            v = vsum / (wsum * wsum)
        if flags & DEMODULATE:
            return x * m, v * (la * la)
        return x, v


def synthetic_var(nx, ny, seed=11):
    """Seeded variance in [0, 0.5) for denoise_ref.synthetic(nx, ny), with the values a
    filter can stumble over: a block of exact zeros, one pixel of 1e30f, a block of
    1e-30f, and a zero-variance block laid over part of the zero-albedo region (rows
    ny // 2 .., columns .. nx // 4 of synthetic)."""
    rng = np.random.default_rng(seed)
    var = rng.random((ny, nx), dtype=f32) * f32(0.5)
    var[: max(1, ny // 5), : max(1, nx // 3)] = 0                    # exact zeros
    var[ny // 4: ny // 4 + max(1, ny // 6), nx // 2: nx // 2 + max(1, nx // 5)] = f32(1e-30)
    var[ny // 2 + ny // 8: ny // 2 + ny // 4, : max(1, nx // 8)] = 0  # zeros over zero albedo
    var[ny // 3, (2 * nx) // 3] = f32(1e30)                           # (written last: it survives at 1 x 1)
    return var
