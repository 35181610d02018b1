"""numpy float32 restatement of srr_denoise (include/srr_capi.h): every operation
in float32, in the header's order, the taps visited (dy, dx) row-major; numpy's
float32 +, -, *, / are the IEEE operations (no FMA) and the exponential is the
host libm's expf (oracle_bind.libm), so the device output must equal this bit for
bit.  Test infrastructure: shared by test_denoise.py (CPU) and the GPU tests."""
import numpy as np

import oracle_bind as ob

f32 = np.float32
B = (f32(0.375), f32(0.25), f32(0.0625))
DEMODULATE = 1


def _sq3(a, b):
    """((a0-b0)^2 + (a1-b1)^2) + (a2-b2)^2 over the last axis."""
    d = a - b
    d = d * d
    return (d[..., 0] + d[..., 1]) + d[..., 2]


def denoise(color, albedo, normal, depth, iterations, k_c, k_n, k_z, flags=0):
    """color, albedo, normal: [ny, nx, 3]; depth: [ny, nx] -> [ny, nx, 3] float32."""
    c = np.ascontiguousarray(color, f32)
    a = np.ascontiguousarray(albedo, f32)
    n = np.ascontiguousarray(normal, f32)
    z = np.ascontiguousarray(depth, f32)
    ny, nx = z.shape
    k_c, k_n, k_z = f32(k_c), f32(k_n), f32(k_z)
    with np.errstate(all="ignore"):
        x = c / (a + f32(1e-3)) if flags & DEMODULATE else c.copy()
        for k in range(iterations):
            s = 1 << k
            kc = k_c * f32(4 ** k)
            total = np.zeros((ny, nx, 3), f32)
            wsum = np.zeros((ny, nx), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    # pixels p whose tap q = p + s*(dx, dy) lies inside the image
                    y0, y1 = max(0, -s * dy), min(ny, ny - s * dy)
                    x0, x1 = max(0, -s * dx), min(nx, nx - s * dx)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))
                    h = B[abs(dx)] * B[abs(dy)]
                    dc = _sq3(x[Q], x[P])
                    dn = _sq3(n[Q], n[P])
                    zp, zq = z[P], z[Q]
                    dz = ((zp - zq) * (zp - zq)) / ((zp * zp + zq * zq) + f32(1e-20))
                    arg = -((dc * kc + dn * k_n) + dz * k_z)
                    w = h * ob.libm("expf", arg)
                    total[P] += w[..., None] * x[Q]
                    wsum[P] += w
            x = total / wsum[..., None]
        return x * (a + f32(1e-3)) if flags & DEMODULATE else x


def synthetic(nx, ny, seed=7):
    """Seeded random colour over guides with a few edges: a vertical normal edge, a
    horizontal depth edge, an albedo step, and a block of pixels with zero normal
    and zero depth (misses)."""
    rng = np.random.default_rng(seed)
    color = rng.random((ny, nx, 3), dtype=f32) * f32(2.0)
    albedo = np.full((ny, nx, 3), f32(0.73))
    albedo[:, nx // 3:] = (f32(0.65), f32(0.05), f32(0.05))
    albedo[ny // 2:, : nx // 4] = 0  # misses have albedo 0
    normal = np.zeros((ny, nx, 3), f32)
    normal[:, : nx // 2, 2] = 1
    normal[:, nx // 2:, 0] = -1
    yy, xx = np.mgrid[0:ny, 0:nx]
    depth = (f32(500.0) + f32(3.0) * xx.astype(f32) + f32(0.5) * yy.astype(f32)).astype(f32)
    depth[ny // 3:] += f32(250.0)
    normal[ny // 2:, : nx // 4] = 0
    depth[ny // 2:, : nx // 4] = 0
    return color, albedo, normal, depth


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)
