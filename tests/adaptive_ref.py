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
            for i in np.flatnonzero(active):
                if n >= budget or (n >= min_spp and rel_tol > 0 and converged(n, s1[i], s2[i], rel_tol, abs_eps)):
                    active[i] = False
    return count, passes


def scene_text() -> str:
    from srr import scenes
    return scenes.s1_cornell()[0].text()


@functools.lru_cache(maxsize=None)
def oracle_frame():
    """The oracle's render of the parity frame at the budget, computed once per
    process: dict(paths, rays, img) -- read-only for its users."""
    import oracle_bind as ob
    ref = ob.render(scene_text(), NX, NY, BUDGET, 50)
    for a in (ref["paths"], ref["rays"], ref["img"]):
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def expected_counts():
    count, passes = pass_loop(oracle_frame()["paths"], BUDGET, BATCH, MIN_SPP, REL_TOL, ABS_EPS)
    count.setflags(write=False)
    return count, passes
