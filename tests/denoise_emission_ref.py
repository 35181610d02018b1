"""numpy float32 restatements of srr_denoise_emission and srr_denoise_var_emission
(include/srr_capi.h) on those of the base filters: subtract the emission, filter, add it
back, each one float32 operation.  Demodulated, x = rdiv(c - e, a + 1e-3f) is the base
filter's set-up on c - e, and the remodulated y = x * (a + 1e-3f) is what it returns, so
the two roundings of the output are its multiply and the add here.  Test infrastructure:
shared by test_denoise_emission.py (CPU) and the GPU tests."""
import numpy as np

import denoise_ref as dn
import denoise_var_ref as dv

f32 = np.float32
DEMODULATE = dn.DEMODULATE
bits = dn.bits


def denoise_emission(color, emission, albedo, normal, depth, iterations, k_c, k_n, k_z, flags=0):
    """color, emission, albedo, normal: [ny, nx, 3]; depth: [ny, nx] -> [ny, nx, 3] float32."""
    c = np.ascontiguousarray(color, f32)
    e = np.ascontiguousarray(emission, f32)
    with np.errstate(all="ignore"):
        y = dn.denoise(c - e, albedo, normal, depth, iterations, k_c, k_n, k_z, flags)
        return y + e


def denoise_var_emission(color, var, emission, albedo, normal, depth, iterations, k_l, k_n, k_z, flags=0):
    """-> (out [ny, nx, 3], var_out [ny, nx]); the variance goes through unchanged."""
    c = np.ascontiguousarray(color, f32)
    e = np.ascontiguousarray(emission, f32)
    with np.errstate(all="ignore"):
        y, var_out = dv.denoise_var(c - e, var, albedo, normal, depth, iterations, k_l, k_n, k_z, flags)
        return y + e, var_out


def synthetic_emission(nx, ny, color):
    """An emission image for denoise_ref.synthetic's colour: zero but for a block (the light), whose
    left half equals the colour exactly (c - e = 0 there) and whose right half is a constant (15, 12,
    9), larger than any colour (c - e < 0: a frame of few samples can hold less than its emission
    only by rounding, the filters must not care)."""
    e = np.zeros((ny, nx, 3), f32)
    y0, y1, x0, x1 = ny // 4, max(ny // 4 + 1, ny // 2), nx // 3, max(nx // 3 + 1, (2 * nx) // 3)
    xm = (x0 + x1 + 1) // 2
    e[y0:y1, x0:xm] = np.ascontiguousarray(color, f32)[y0:y1, x0:xm]
    e[y0:y1, xm:x1] = (f32(15.0), f32(12.0), f32(9.0))
    return e
