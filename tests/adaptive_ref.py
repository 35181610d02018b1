"""Adaptive sampling restated in numpy (include/srr_capi.h srr_render_adaptive):
the convergence rule in np.float32 scalars in the stated order, and the whole
pass loop over a CPU-oracle render's per-path radiance, which gives the sample
count every pixel must end with.  Shared by tests/test_adaptive.py (CPU) and
tests/test_gpu_adaptive.py."""
from __future__ import annotations

import functools

import numpy as np

F = np.float32

# The frame of the oracle-parity test: a Cornell box with its light in view, ragged
# on purpose (37 * 29 = 1,073 pixels: 5 blocks of 256, the last one partial, and a
# partial wave), 4 samples per pass, none retiring before 8, budget 32.
NX, NY, BUDGET, BATCH, MIN_SPP = 37, 29, 32, 4, 8
ABS_EPS = 1e-3
# Chosen on the CPU from the oracle's paths alone (tests/test_adaptive.py checks
# the condition): at 0.05 about half the pixels stop at 8 samples, 31 % run to the
# budget and every pass boundary in between (12, 16, ... 28) retires some.
REL_TOL = 0.05


def converged(n, s1, s2, rel_tol, abs_eps) -> bool:
    """(s2*nf - s1*s1) <= ((rel_tol*rel_tol) * (nf - 1)) * ((s1 + abs_eps*nf) * (s1 + abs_eps*nf)),
    every operation rounded to float32, in this order."""
    s1, s2, rel_tol, abs_eps = F(s1), F(s2), F(rel_tol), F(abs_eps)
    nf = F(n)
    with np.errstate(all="ignore"):
        lhs = F(F(s2 * nf) - F(s1 * s1))
        m = F(s1 + F(abs_eps * nf))
        rhs = F(F(F(rel_tol * rel_tol) * F(nf - F(1.0))) * F(m * m))
        return bool(lhs <= rhs)


def converged_many(n, s1: np.ndarray, s2: np.ndarray, rel_tol, abs_eps) -> np.ndarray:
    """converged() over float32 arrays: the same operations in the same order, each
    rounded to float32 elementwise (tests/test_adaptive.py holds it to the scalar)."""
    assert s1.dtype == F and s2.dtype == F
    rel_tol, abs_eps, nf = F(rel_tol), F(abs_eps), F(n)
    with np.errstate(all="ignore"):
        lhs = (s2 * nf) - (s1 * s1)
        m = s1 + F(abs_eps * nf)
        rhs = F(F(rel_tol * rel_tol) * F(nf - F(1.0))) * (m * m)
        assert lhs.dtype == F and rhs.dtype == F
        return lhs <= rhs


def luminance(rgb: np.ndarray) -> np.ndarray:
    """y = (0.2126f*r + 0.7152f*g) + 0.0722f*b of de_nan'd float32 samples [..., 3]."""
    c = np.where(np.isnan(rgb), F(0), rgb).astype(F)
    with np.errstate(all="ignore"):
        return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def pass_loop(paths: np.ndarray, budget: int, batch_spp: int, min_spp: int, rel_tol: float, abs_eps: float):
    """The pass loop over paths[npix, >= budget, 3] (raw radiance per path, as the
    oracle returns it): returns (count[npix], passes)."""
    npix = paths.shape[0]
    y = luminance(paths[:, :budget])
    s1 = np.zeros(npix, F)
    s2 = np.zeros(npix, F)
    count = np.zeros(npix, np.int32)
    active = np.ones(npix, bool)
    n = passes = 0
    with np.errstate(all="ignore"):
        while active.any() and n < budget:
            w = min(batch_spp, budget - n)
            for s in range(n, n + w):  # folded in sample order, float32
                s1[active] = s1[active] + y[active, s]
                s2[active] = s2[active] + y[active, s] * y[active, s]
            n += w
            passes += 1
            count[active] = n
            if n >= budget:
                active[:] = False
            elif n >= min_spp and rel_tol > 0:
                active &= ~converged_many(n, s1, s2, rel_tol, abs_eps)
    return count, passes


def scene_text() -> str:
    from srr import scenes
    return scenes.s1_cornell()[0].text()


# The frames of the scan-chunk test: the same scene at 300 x 220 = 66,000 pixels, which
# is 258 blocks of 256 rows (the last one holds 208), so the compaction's block scan
# (kernels.hip k_compact_scan, 256 block counts per chunk) runs two chunks and the
# second starts from the first one's carry; and at 300 x 440 = 132,000 pixels (516
# blocks, the last one holds 160: three chunks), where the second chunk covers the
# lower half of the picture, so the 18,824 rows that survive the first decision there
# are written at offsets that include the first chunk's carry of 37,240.  (At 300 x 220
# blocks 256 and 257 see only the black background and keep nothing, as the third chunk
# does at 300 x 440: there the carry shows in the compacted total alone.  The later
# compactions have fewer than 65,536 rows, one chunk.)
# 4 samples per pass, budget 12.
BIG_NX, BIG_BUDGET, BIG_BATCH, BIG_MIN_SPP = 300, 12, 4, 4
BIG_NYS = (220, 440)
# Chosen on the CPU from the oracle's paths alone (tests/test_adaptive.py checks the
# condition and prints the counts).  At 300 x 220 and 0.05: 37,718 pixels (57 %) retire
# at the first decision (4 samples), 7,211 at 8 and 21,071 (32 %) stay active to the budget.
BIG_REL_TOL = 0.05
CHUNK_ROWS = 256 * 256  # pixels per scan chunk: 256 block counts of 256 rows


@functools.lru_cache(maxsize=None)
def oracle_frame(nx: int = NX, ny: int = NY, budget: int = BUDGET, threads: int = 1):
    """The oracle's render of a frame of scene_text() at the budget (default: the
    parity frame), computed once per process: dict(paths, rays, img) -- read-only
    for its users."""
    import oracle_bind as ob
    ref = ob.render(scene_text(), nx, ny, budget, 50, threads=threads)
    for a in (ref["paths"], ref["rays"], ref["img"]):
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def expected_counts():
    count, passes = pass_loop(oracle_frame()["paths"], BUDGET, BATCH, MIN_SPP, REL_TOL, ABS_EPS)
    count.setflags(write=False)
    return count, passes


def big_oracle_frame(ny: int):
    return oracle_frame(BIG_NX, ny, BIG_BUDGET, 8)  # 792,000 paths at 220 rows, 1,584,000 at 440


@functools.lru_cache(maxsize=None)
def big_expected_counts(ny: int):
    count, passes = pass_loop(big_oracle_frame(ny)["paths"], BIG_BUDGET, BIG_BATCH, BIG_MIN_SPP, BIG_REL_TOL, ABS_EPS)
    count.setflags(write=False)
    return count, passes


def check_big_frame(count, ny: int) -> None:
    """The scan-chunk test's precondition, from the restatement's counts alone: more
    than one scan chunk, a partial last block, 20-80 % of the pixels retired at the
    first decision, a non-zero carry into the second chunk, and some pixels active to
    the end.  At 440 rows also: the first compaction keeps rows in the second chunk,
    behind a non-zero carry that their offsets must include."""
    npix = BIG_NX * ny
    blocks = -(-npix // 256)
    assert count.shape == (npix,) and blocks == {220: 258, 440: 516}[ny] and npix % 256 == {220: 208, 440: 160}[ny]
    first = float((count == BIG_BATCH).mean())
    assert 0.2 <= first <= 0.8, first
    assert (count == BIG_BUDGET).any() and (count == 2 * BIG_BATCH).any()
    keep = count > BIG_BATCH  # the rows the first compaction keeps
    assert keep[:CHUNK_ROWS].sum() > 256 and (~keep[CHUNK_ROWS:]).any()
    if ny == 440:
        assert keep[CHUNK_ROWS:2 * CHUNK_ROWS].sum() > 256 and (~keep[CHUNK_ROWS:2 * CHUNK_ROWS]).sum() > 256
