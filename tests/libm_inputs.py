"""Input sets of the libm sweeps (tests/test_device_libm.py, tests/golden/
make_libm_pins.py, make_libm_hard.py): one fixed-seed set per function, shared by
the host libm, the host build and the device build of csrc/glibc_mathf.h and
include/srr/glibc_math64.h.

Each set is: bit patterns stratified over every exponent and both signs (the whole
subnormal range included), the special values, and every branch edge of the
routine +-64 ulps, read off the two headers.  Only exactly rounded numpy steps are
used to build inputs (+ - * /, casts, bit views); no numpy transcendental."""
from __future__ import annotations

import functools

import numpy as np

F32, F64 = np.float32, np.float64
SEED = 20191108
SIN64_LIMIT = 105414336.0  # glibc_math64.h: sin / cos / sincos are restated below __branred's range

# device name -> (host libm name, element type, operands, results); "rdiv" has no libm
# counterpart (its reference is numpy's float32 division, which is correctly rounded)
FUNCS = {
    "rsin": ("sinf", F32, 1, 1), "rcos": ("cosf", F32, 1, 1), "rexp": ("expf", F32, 1, 1),
    "rlog": ("logf", F32, 1, 1), "rpow": ("powf", F32, 2, 1), "racos": ("acosf", F32, 1, 1),
    "rasin": ("asinf", F32, 1, 1), "ratan2": ("atan2f", F32, 2, 1), "sincosf": ("sincosf", F32, 1, 2),
    "atanf": ("atanf", F32, 1, 1),
    "sin64": ("sin", F64, 1, 1), "cos64": ("cos", F64, 1, 1), "sincos64": ("sincos", F64, 1, 2),
    "acos64": ("acos", F64, 1, 1), "atan2_64": ("atan2", F64, 2, 1), "log64": ("log", F64, 1, 1),
}
# random mantissas per (exponent, sign): 512 x 8,192 = 2^22 floats, 4,096 x 256 = 2^20 doubles
PER_EXP32 = 8192
PER_EXP64 = 256
RANDOM_PAIRS = 1 << 22


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng([SEED, *name.encode()])


def f32_bits(u) -> np.ndarray:
    return np.asarray(u, dtype=np.uint32).view(F32)


def f64_bits(u) -> np.ndarray:
    return np.asarray(u, dtype=np.uint64).view(F64)


def stratified32(rng, per=None, exps=range(256)) -> np.ndarray:
    """`per` random mantissas for every (exponent, sign); exponent 0 is the subnormal
    range (smallest and largest added by specials32), 255 is inf / NaN."""
    per = per or PER_EXP32
    e = np.repeat(np.asarray(list(exps), np.uint32), 2 * per)
    s = np.tile(np.repeat(np.uint32([0, 1]), per), len(e) // (2 * per))
    m = rng.integers(0, 1 << 23, size=e.size, dtype=np.uint32)
    return f32_bits((s << np.uint32(31)) | (e << np.uint32(23)) | m)


def stratified64(rng, per=None, exps=range(2048)) -> np.ndarray:
    per = per or PER_EXP64
    e = np.repeat(np.asarray(list(exps), np.uint64), 2 * per)
    s = np.tile(np.repeat(np.uint64([0, 1]), per), len(e) // (2 * per))
    m = rng.integers(0, 1 << 52, size=e.size, dtype=np.uint64)
    return f64_bits((s << np.uint64(63)) | (e << np.uint64(52)) | m)


def around(values, dtype, k: int = 64) -> np.ndarray:
    """Every value within +-k ulps of each edge, and the negatives of them all."""
    it = np.uint32 if dtype == F32 else np.uint64
    sign = it(1) << it(31 if dtype == F32 else 63)
    b = np.abs(np.asarray(values, dtype=dtype)).view(it).astype(np.int64)
    w = (b[:, None] + np.arange(-k, k + 1, dtype=np.int64)[None, :]).ravel()
    w = w[w >= 0].astype(it)
    return np.concatenate([w, w | sign]).view(dtype)


def specials32() -> np.ndarray:
    tiny, big = np.finfo(F32).tiny, np.finfo(F32).max
    pos = np.concatenate([F32([0, 1, np.inf, np.nan, big]), f32_bits([1, 2, 0x7FFFFF, 0x7FFFFE]),
                          around([tiny, 1.0], F32, 2)])
    return np.concatenate([pos, -pos]).astype(F32)


def specials64() -> np.ndarray:
    tiny = np.finfo(F64).tiny
    pos = np.concatenate([F64([0, 1, np.inf, np.nan, np.finfo(F64).max, np.finfo(F32).max, np.finfo(F32).tiny]),
                          f64_bits([1, 2, (1 << 52) - 1, (1 << 52) - 2]), around([tiny, 1.0], F64, 2)])
    return np.concatenate([pos, -pos]).astype(F64)


# ---- branch edges, as the headers state them --------------------------------

def _log_rows() -> np.ndarray:  # logf_ / powf_: table row = ((ix - 0x3f330000) >> 19) % 16
    return f32_bits(0x3F330000 + (np.arange(17, dtype=np.uint32) << np.uint32(19)))


def _pio4_multiples32() -> np.ndarray:  # k * pi/4 up to the 120 threshold (float32 product of exact steps)
    k = np.arange(1, 156, dtype=F64)
    return (k * F64(0.78539816339744830962)).astype(F32)


EDGES32 = {
    # 88 (the range check), overflow / underflow thresholds, log(FLT_MIN) (subnormal results), |x| = 32
    "rexp": lambda: np.concatenate([F32([88.0, 32.0, 1.0, 87.33654475, 103.2789, 0.5 * 0.021660849, 0.021660849]),
                                    f32_bits([0x42B17218, 0x42CFF1B4, 0x42AEAC50])]),
    # near-1 window, the 16 table rows, subnormal / normal boundary
    "rlog": lambda: np.concatenate([_log_rows(), F32([1.0, 2.0, 0.5, 4.0]), f32_bits([0x00800000, 0x7F7FFFFF])]),
    # pi/4 (float) and its multiples, 120 (switch to reduce_large), 2^-12 (tiny), exponent steps of reduce_large
    "rsin": lambda: np.concatenate([_pio4_multiples32(), f32_bits([0x3F490FDB]),
                                    F32([120.0, 2.0 ** -12, 128.0, 1024.0, 2.0 ** 23, 2.0 ** 24, 2.0 ** 26, 2.0 ** 30])]),
    # 0.5, 1, 2^-26 (acosf_), 2^-27 and 0.975 (asinf_), just above 1
    "racos": lambda: np.concatenate([F32([0.5, 1.0, 2.0 ** -26, 2.0 ** -27, 0.975, 0.25, 0.75]),
                                     f32_bits([0x3F79999A, 0x32800000, 0x32000000])]),
    # 7/16, 11/16, 19/16, 39/16, 2^-29, 2^25, 1
    "atanf": lambda: F32([0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** -29, 2.0 ** 25, 1.0, 2.0 ** 24]),
}
EDGES32["rcos"] = EDGES32["sincosf"] = EDGES32["rsin"]
EDGES32["rasin"] = EDGES32["racos"]


def _sincos_rows64() -> np.ndarray:  # do_sin / do_cos: |x| + 1.5 * 2^45 rounds to a multiple of 1/128
    return (np.arange(0, 128, dtype=F64) + 0.5) / 128.0


def _acos_rows64() -> np.ndarray:  # e_asin.c rows: [0.125, 0.25) in 32, [0.25, 0.5) in 64, [0.5, 1) in 128
    return np.concatenate([b * (1.0 + np.arange(r, dtype=F64) / r) for b, r in ((0.125, 32), (0.25, 64), (0.5, 128))])


_PIO2 = 1.5707963267948966
EDGES64 = {
    "sin64": lambda: np.concatenate([F64([2.0 ** -26, 2.0 ** -27, 0.126, 0.855469, 0.85546875, 2.426265,
                                          2.4262650203704834, 105414335.0, 1.0]),
                                     f64_bits([0x3FEB600000000000, 0x400368FD00000000]),
                                     _PIO2 * np.arange(1, 9, dtype=F64), _sincos_rows64(),
                                     _PIO2 - _sincos_rows64(), _PIO2 + _sincos_rows64()]),
    "acos64": lambda: np.concatenate([F64([2.0 ** -55, 0.125, 0.25, 0.5, 0.75, 0.921875, 0.953125, 0.96875, 1.0]),
                                      _acos_rows64()]),
}
EDGES64["cos64"] = EDGES64["sincos64"] = EDGES64["sin64"]


def _log_rows64() -> np.ndarray:  # e_log.c: row = ((ix - 0x3fe6000000000000) >> 45) % 128, z in [0x1.6p-1, 0x1.6p0)
    return f64_bits(np.uint64(0x3FE6000000000000) + (np.arange(129, dtype=np.uint64) << np.uint64(45)))


# the near-1 window [1 - 2^-4, 1 + 0x1.09p-4), 1 itself, the 128 rows, the subnormal boundary, 2^+-k
EDGES64["log64"] = lambda: np.concatenate([F64([1.0 - 2.0 ** -4, 1.0, 2.0, 0.5, 2.0 ** -32, 2.0 ** -1022]),
                                           f64_bits([0x3FF1090000000000]), _log_rows64()])


# ---- one-operand sets -------------------------------------------------------

def _unary32(name: str) -> np.ndarray:
    rng = _rng(name)
    parts = [stratified32(rng), specials32(), around(EDGES32[name](), F32)]
    if name in ("racos", "rasin"):  # most of the bit patterns lie outside [-1, 1]: fill the domain by value too
        parts.append((rng.random(RANDOM_PAIRS // 4) * 2 - 1).astype(F32))
    if name in ("rsin", "rcos", "sincosf"):  # the kernels' angles
        parts.append((rng.random(RANDOM_PAIRS // 4) * 14 - 7).astype(F32))
    return np.concatenate(parts).astype(F32)


def _unary64(name: str) -> np.ndarray:
    rng = _rng(name)
    if name == "acos64":
        u = rng.random(RANDOM_PAIRS // 8)
        near1 = 1.0 - u * F64(2.0) ** -rng.integers(0, 60, size=u.size).astype(F64)
        parts = [stratified64(rng), specials64(), around(EDGES64[name](), F64), rng.random(RANDOM_PAIRS // 8) * 2 - 1,
                 near1, -near1]
        return np.concatenate(parts)
    if name == "log64":
        # the near-1 window by value, and the medium's draws k / 2^32 (drand): small, large and random k
        near1 = 1.0 + (rng.random(RANDOM_PAIRS // 8) - 0.5) * 0.15
        k = np.concatenate([np.arange(0, 4096), (1 << 32) - 1 - np.arange(4096),
                            rng.integers(0, 1 << 32, size=RANDOM_PAIRS // 8)]).astype(F64)
        return np.concatenate([stratified64(rng), specials64(), around(EDGES64[name](), F64), near1,
                               k / F64(4294967296.0)])
    # exponents below 2^27 only, then the stated domain
    x = np.concatenate([stratified64(rng, per=2 * PER_EXP64, exps=range(0, 1023 + 27)), specials64(),
                        around(EDGES64[name](), F64), rng.random(RANDOM_PAIRS // 8) * 14 - 7])
    keep = ~(np.abs(x) >= SIN64_LIMIT) | ~np.isfinite(x)  # finite values at or beyond the limit are left out
    return x[keep]


# ---- two-operand sets -------------------------------------------------------

def _powf_pairs():
    rng = _rng("rpow")
    n = RANDOM_PAIRS // 2
    u = rng.random(n, dtype=F32)
    v = rng.random(n, dtype=F32)
    # the Beckmann sampler's pow(1 - u, fit) (tools/check_glibc_mathf.cpp) ...
    x1 = F32(1) - np.maximum(u, F32(1e-6))
    y1 = F32(1) + v * (F32(-0.876) + rng.random(n, dtype=F32) * F32(0.4265))
    # ... and general pairs
    x2 = (F32(1e-7) + rng.random(n, dtype=F32) * F32(4.0 - 1e-7)).astype(F32)
    y2 = (rng.random(n, dtype=F32) * F32(16) - F32(8)).astype(F32)
    # the log2 table rows +-64 ulps against a few exponents
    rows = around(_log_rows(), F32)
    rows = rows[rows > 0]
    x3 = np.tile(rows, 6)
    y3 = np.repeat(F32([1.0, -1.0, 0.124, 2.5, -7.75, 40.0]), rows.size)
    # results that are subnormal, just below overflow, or beyond either: y * log2(x) near +-126 .. +-150.
    # x = 2^a * (1 + f) over exponents, y = t / a' with a' the float of x's exponent (exact steps only)
    m = RANDOM_PAIRS // 8
    ex = rng.integers(-120, 121, size=m)
    ex = ex[ex != 0]
    x4 = (F64(2.0) ** ex.astype(F64) * (1.0 + rng.random(ex.size) * 2.0 ** -8)).astype(F32)
    t = np.where(rng.random(ex.size) < 0.5, -1.0, 1.0) * (124.0 + rng.random(ex.size) * 27.0)
    y4 = (t / ex.astype(F64)).astype(F32)
    # special operands (the header's double route): zero, inf, NaN, negative and subnormal x; y zero / inf / NaN
    sx = np.concatenate([specials32(), F32([-2.0, -0.5, 2.0, 0.5, 3.0]), f32_bits([0x00000100, 0x80000100, 0x00400000])])
    sy = np.concatenate([specials32(), F32([2.0, 3.0, -2.0, -3.0, 0.5, -0.5, 1e30, -1e30])])
    gx, gy = np.meshgrid(sx, sy, indexing="ij")
    x5, y5 = gx.ravel(), gy.ravel()
    sub = stratified32(rng, per=max(1, PER_EXP32 // 8), exps=[0])  # subnormal and negative-subnormal x
    x6, y6 = sub, (rng.random(sub.size, dtype=F32) * F32(4) - F32(2)).astype(F32)
    # every exponent and both signs of x against exponents of any size down to 2^-8
    x7 = stratified32(rng, per=PER_EXP32 // 4)
    y7 = ((rng.random(x7.size) * 16 - 8) * F64(2.0) ** -rng.integers(0, 9, size=x7.size).astype(F64)).astype(F32)
    return (np.concatenate([x1, x2, x3, x4, x5, x6, x7]).astype(F32),
            np.concatenate([y1, y2, y3, y4, y5, y6, y7]).astype(F32))


def _atan2f_pairs():
    rng = _rng("ratan2")
    n = RANDOM_PAIRS // 4
    # get_sphere_uv: components of unit vectors (normalised with exactly rounded steps)
    v = (rng.random((n, 3)) * 2 - 1).astype(F32)
    ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]).astype(F32))
    with np.errstate(all="ignore"):
        y1, x1 = (v[:, 2] / ln).astype(F32), (v[:, 0] / ln).astype(F32)
    # general pairs, every quadrant
    y2 = ((rng.random(n) * 2 - 1) * np.where(rng.random(n) < 0.5, 1000.0, 1.0)).astype(F32)
    x2 = (rng.random(n) * 2 - 1).astype(F32)
    # any two bit patterns (the exponent-difference cut-offs at +-60 among them)
    y3 = stratified32(rng, per=max(1, PER_EXP32 // 4))
    x3 = rng.permutation(stratified32(rng, per=max(1, PER_EXP32 // 4)))
    # ratios at atanf_'s breakpoints: y = edge +- 64 ulps against x = +-1 and +-2^k
    e = around(EDGES32["atanf"](), F32)
    k = F32([1.0, -1.0, 0.25, -8.0])
    y4, x4 = np.tile(e, k.size), np.repeat(k, e.size)
    with np.errstate(all="ignore"):
        y4 = (y4 * np.abs(x4)).astype(F32)
    # |y| / |x| = 2^+-60, 2^+-61 (k > 60, k < -60)
    base = (F32(1) + rng.random(4096, dtype=F32)).astype(F32)
    sh = np.repeat(F32([2.0 ** 59, 2.0 ** 60, 2.0 ** 61, 2.0 ** 62]), 1024)
    sg = np.where(rng.random(4096) < 0.5, F32(-1), F32(1)).astype(F32)
    y5 = np.concatenate([base * sh * F32(2.0 ** -40), base * F32(2.0 ** -40)]).astype(F32)
    x5 = np.concatenate([sg * base[::-1] * F32(2.0 ** -40), sg * base[::-1] * sh * F32(2.0 ** -40)]).astype(F32)
    # zeros, infinities, NaN, +-1, FLT_MIN neighbours: all pairs
    s = specials32()
    gy, gx = np.meshgrid(s, s, indexing="ij")
    return (np.concatenate([y1, y2, y3, y4, y5, gy.ravel()]).astype(F32),
            np.concatenate([x1, x2, x3, x4, x5, gx.ravel()]).astype(F32))


def _atan2_64_pairs():
    rng = _rng("atan2_64")
    n = RANDOM_PAIRS // 16
    # directions: a point in the square scaled (every quadrant, any ratio)
    y1, x1 = rng.random(n) * 4 - 2, rng.random(n) * 4 - 2
    # any two bit patterns
    y2 = stratified64(rng, per=max(1, PER_EXP64 // 4))
    x2 = rng.permutation(stratified64(rng, per=max(1, PER_EXP64 // 4)))
    # the MERL lookup's ~1e-17 residues (tools/check_glibc_math64.cpp), zeros mixed in
    def residue(m):
        v = (0.5 + 0.5 * rng.random(m)) * F64(2.0) ** -(50 + rng.integers(0, 20, size=m)).astype(F64)
        v = np.where(rng.random(m) < 0.5, -v, v)
        return np.where(rng.integers(0, 16, size=m) == 0, 0.0, v)
    y3, x3 = residue(n), residue(n)
    # ratio u = small / large at 1/16, at every cij row boundary (j + 0.5) / 256 and at 1, +-64 ulps,
    # against large = 2^k, both orders, every quadrant
    u = around(np.concatenate([F64([0.0625, 1.0]), (np.arange(16, 256, dtype=F64) + 0.5) / 256.0]), F64)
    u = np.abs(u)
    big = F64(2.0) ** rng.integers(-20, 20, size=u.size).astype(F64)
    a, b = u * big, big
    swap = rng.random(u.size) < 0.5
    a, b = np.where(swap, b, a), np.where(swap, a, b)
    y4 = np.where(rng.random(u.size) < 0.5, -a, a)
    x4 = np.where(rng.random(u.size) < 0.5, -b, b)
    ur = rng.random(n)
    y4 = np.concatenate([y4, ur * 3.0, -ur * 0.5])
    x4 = np.concatenate([x4, np.full(n, 3.0), np.full(n, -0.5)])
    # exponent differences at the +-57 cut-off, and operands below 2^-500 / above 2^500
    m = 4096
    f1, f2 = 1.0 + rng.random(m), 1.0 + rng.random(m)
    sh = F64(2.0) ** rng.integers(55, 60, size=m).astype(F64)
    sg = np.where(rng.random(m) < 0.5, -1.0, 1.0)
    y5 = np.concatenate([f1 * sh, f1, f1 * 2.0 ** -510, f1 * 2.0 ** 505, f1 * 2.0 ** -510])
    x5 = np.concatenate([sg * f2, sg * f2 * sh, sg * f2 * 2.0 ** -505, sg * f2 * 2.0 ** 510, sg * f2 * 2.0 ** 505])
    s = specials64()
    gy, gx = np.meshgrid(s, s, indexing="ij")
    return (np.concatenate([y1, y2, y3, y4, y5, gy.ravel()]).astype(F64),
            np.concatenate([x1, x2, x3, x4, x5, gx.ravel()]).astype(F64))


def _rdiv_pairs():
    """rdiv: 2^22 random pairs, quotients that are subnormal and quotients just above
    and below FLT_MIN, zeros / infinities / NaN."""
    rng = _rng("rdiv")
    a1 = stratified32(rng)
    b1 = rng.permutation(stratified32(rng))
    m = RANDOM_PAIRS // 8
    fa, fb = (F32(1) + rng.random(m, dtype=F32)).astype(F32), (F32(1) + rng.random(m, dtype=F32)).astype(F32)
    sg = np.where(rng.random(m) < 0.5, F32(-1), F32(1)).astype(F32)
    # subnormal quotients: 2^-100 / 2^(27..49); around FLT_MIN: 2^-100 / 2^26 = 2^-126, times (1 +- a few 2^-23)
    ka = (F32(2.0) ** rng.integers(27, 50, size=m).astype(F32)).astype(F32)
    a2, b2 = (fa * F32(2.0 ** -100) * sg).astype(F32), (fb * ka).astype(F32)
    near = (F32(1) + (rng.integers(-64, 65, size=m).astype(F32) * F32(2.0 ** -23))).astype(F32)
    a3, b3 = (fb * near * F32(2.0 ** -100) * sg).astype(F32), (fb * F32(2.0 ** 26)).astype(F32)
    a4, b4 = (near * F32(2.0 ** -126) * sg).astype(F32), np.ones(m, F32)   # the FLT_MIN neighbours themselves
    a5, b5 = (fa * F32(2.0 ** -126)).astype(F32), (fb * F32(2.0)).astype(F32)   # subnormal from a normal / 2..4
    s = specials32()
    ga, gb = np.meshgrid(s, s, indexing="ij")
    return (np.concatenate([a1, a2, a3, a4, a5, ga.ravel()]).astype(F32),
            np.concatenate([b1, b2, b3, b4, b5, gb.ravel()]).astype(F32))


# ---- the kernels' double calls (tests/test_device_libm.py part 4, make_libm_hard.py) ----

# every medium density and dielectric index of srr/scenes.py, srr/ref_scenes.py and the golden scenes, and density 1
DENSITIES = (0.0001, 0.2, 1.0)
INDICES = (1.5, 1.4, 1.2)
TWO_PI = F64(2.0) * F64(3.14159265358979323846)  # devmath.h kPi; `2 * kPi * u2` is (2 * kPi) * (double)u2


def pcg_u2(u32):
    """devmath.h pcg_uniform's result for the 32-bit draw u: fminf(0.99999994f, float(u) * 2^-32f)."""
    return np.minimum(F32(0.99999994), u32.astype(np.uint32).astype(F32) * F32(2.3283064365386963e-10))


@functools.lru_cache(maxsize=None)
def inputs(name: str):
    """(x, y or None) of one function: read-only arrays, built once per process."""
    if name == "rpow":
        x, y = _powf_pairs()
    elif name == "ratan2":
        x, y = _atan2f_pairs()
    elif name == "atan2_64":
        x, y = _atan2_64_pairs()
    elif name == "rdiv":
        x, y = _rdiv_pairs()
    elif FUNCS[name][1] == F32:
        x, y = _unary32(name), None
    else:
        x, y = _unary64(name), None
    for a in (x, y):
        if a is not None:
            a.setflags(write=False)
    return x, y


def same_bits(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Elementwise: identical bit patterns, or both NaN."""
    it = np.uint32 if a.dtype == F32 else np.uint64
    return (a.view(it) == b.view(it)) | (np.isnan(a) & np.isnan(b))
