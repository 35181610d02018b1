"""Adaptive sampling, host side (include/srr_capi.h srr_render_adaptive): the
exported symbols, the convergence rule against its numpy float32 restatement
(tests/adaptive_ref.py), and the condition on the inputs of the GPU parity test
(tests/test_gpu_adaptive.py) -- none of which needs a GPU."""
import ctypes

import numpy as np
import pytest

import adaptive_ref as ar
from srr import capi

F = np.float32


def test_symbols_and_struct_sizes():
    L = capi.lib()
    for name in ("srr_render_adaptive", "srr_render_adaptive_host", "srr_adaptive_converged"):
        assert hasattr(L, name), name
    # srr_adaptive_params: uint32, int, int, float, float; srr_adaptive_stats: uint32,
    # int32, 3 x int64, double (no padding in either)
    assert ctypes.sizeof(capi.AdaptiveParams) == 20
    assert ctypes.sizeof(capi.AdaptiveStats) == 40
    assert capi.AdaptiveStats.paths.offset == 8 and capi.AdaptiveStats.total_ms.offset == 32


def _ulp_neighbours(x):
    x = F(x)
    return [np.nextafter(x, F(-np.inf)), x, np.nextafter(x, F(np.inf))]


def _crafted():
    cases = []
    # zero variance: n equal samples y, s1 = n*y, s2 = n*y*y exactly (powers of two)
    for n, y in ((4, 0.5), (16, 2.0), (64, 0.25)):
        for tol in (0.0, 0.02, 1.0):
            cases.append((n, n * y, n * y * y, tol, 1e-3))
    # all black, floor zero and positive
    for n in (1, 8, 1024):
        for tol in (0.0, 0.02):
            for eps in (0.0, 1e-3):
                cases.append((n, 0.0, 0.0, tol, eps))
    # rel_tol = 0 with variance; n = 1 (the right-hand side is 0)
    cases += [(16, 3.0, 5.0, 0.0, 0.0), (16, 3.0, 5.0, 0.0, 1e-3), (1, 0.7, 0.49, 0.02, 1e-3),
              (1, 0.7, 0.7 * 0.7, 0.5, 0.0), (1, 3.0, 9.0, 0.0, 0.0)]
    # near an equality, walking s2, s1 and rel_tol by single ulps
    for n, s1, tol, eps in ((16, 8.0, 0.1, 0.0), (32, 5.25, 0.05, 1e-3), (8, 100.0, 0.25, 0.0), (1000, 77.7, 0.02, 1e-3)):
        nf = F(n)
        m = F(F(s1) + F(F(eps) * nf))
        rhs = F(F(F(F(tol) * F(tol)) * F(nf - F(1))) * F(m * m))
        s2_eq = F(F(rhs + F(F(s1) * F(s1))) / nf)
        for s2 in _ulp_neighbours(s2_eq):
            cases += [(n, s1, s2, t, eps) for t in _ulp_neighbours(tol)]
        cases += [(n, s, s2_eq, tol, eps) for s in _ulp_neighbours(s1)]
    # non-finite sums never converge
    cases += [(16, np.inf, np.inf, 0.02, 1e-3), (16, np.nan, 1.0, 0.02, 1e-3)]
    return cases


def test_criterion_matches_the_float32_restatement():
    cases = _crafted()
    got = [capi.adaptive_converged(*c) for c in cases]
    want = [ar.converged(*c) for c in cases]
    assert got == want, [c for c, g, w in zip(cases, got, want) if g != w]
    assert any(want) and not all(want)
    # the array form the pass loop uses decides each case as the scalar form does
    for n, tol, eps in {(c[0], c[3], c[4]) for c in cases}:
        sel = [c for c in cases if (c[0], c[3], c[4]) == (n, tol, eps)]
        many = ar.converged_many(n, F([c[1] for c in sel]), F([c[2] for c in sel]), tol, eps)
        assert many.tolist() == [ar.converged(*c) for c in sel], (n, tol, eps)


@pytest.mark.parametrize("n,s1,tol,eps", [(16, 0.0, 0.1, 0.5), (64, 0.0, 0.02, 1e-3), (4, 0.5, 0.3, 1.0)])
def test_criterion_either_side_of_equality(n, s1, tol, eps):
    """Inputs whose left-hand side is exactly the right-hand side, and one ulp of
    the right-hand side below and above it: n a power of two and s1*s1 small and
    exact, so that s2 = (t + s1*s1) / n gives s2*nf - s1*s1 == t without rounding
    (asserted).  The rule holds at and below equality, not above."""
    nf, s1 = F(n), F(s1)
    m = F(s1 + F(F(eps) * nf))
    rhs = F(F(F(F(tol) * F(tol)) * F(nf - F(1))) * F(m * m))
    below, at, above = _ulp_neighbours(rhs)
    for t, want in ((below, True), (at, True), (above, False)):
        s2 = F(F(t + F(s1 * s1)) / nf)
        assert F(F(s2 * nf) - F(s1 * s1)) == t  # the crafting is exact
        assert ar.converged(n, s1, s2, tol, eps) is want
        assert capi.adaptive_converged(n, s1, s2, tol, eps) is want


def test_criterion_properties():
    # zero variance converges at any tolerance, 0 included (which is why the pass
    # loop, not the rule, implements "rel_tol = 0 never retires")
    assert capi.adaptive_converged(16, 32.0, 64.0, 0.0, 0.0)
    assert capi.adaptive_converged(8, 0.0, 0.0, 0.0, 0.0)
    # variance and rel_tol = 0: never
    assert not capi.adaptive_converged(16, 3.0, 5.0, 0.0, 1e-3)
    # n = 1: one sample has s2 = s1*s1, both sides are 0
    assert capi.adaptive_converged(1, 3.0, 9.0, 0.02, 0.0)


def test_parity_frame_exercises_every_branch():
    """Condition on the inputs of the GPU parity test (not on the code under
    test): with the chosen tolerance the oracle's own paths make at least 10 % of
    the pixels retire early, at least 10 % run to the budget, and at least three
    distinct counts occur."""
    count, passes = ar.expected_counts()
    assert count.shape == (ar.NX * ar.NY,)
    early = float((count < ar.BUDGET).mean())
    full = float((count == ar.BUDGET).mean())
    print(f"retire early {early:.3f}, run to the budget {full:.3f}, counts {np.unique(count).tolist()}, passes {passes}")
    assert early >= 0.10 and full >= 0.10
    assert np.unique(count).size >= 3
    assert count.min() >= ar.MIN_SPP and count.max() == ar.BUDGET
    assert ((count - ar.MIN_SPP) % ar.BATCH == 0).all()


@pytest.mark.parametrize("ny", ar.BIG_NYS)
def test_scan_chunk_frame_meets_its_precondition(ny):
    """Condition on the inputs of the GPU scan-chunk test (tests/test_gpu_adaptive.py),
    from the restatement alone: see adaptive_ref.check_big_frame."""
    count, passes = ar.big_expected_counts(ny)
    ar.check_big_frame(count, ny)
    assert passes == 3
    print("retired at 4 / 8 / 12 samples:", [int((count == c).sum()) for c in (4, 8, 12)])


def test_pass_loop_restatement_limits():
    """rel_tol = 0 never retires early; a huge tolerance retires every pixel at the
    first pass boundary at or after min_spp."""
    paths = ar.oracle_frame()["paths"][:64]
    c0, p0 = ar.pass_loop(paths, 12, 5, 4, 0.0, 1e-3)
    assert (c0 == 12).all() and p0 == 3
    c1, p1 = ar.pass_loop(paths, 32, 4, 6, 1e9, 1e-3)
    assert (c1 == 8).all() and p1 == 2


@pytest.mark.parametrize("argv", [["--adaptive", "0.05", "--count-map", "c.png"], []])
def test_cli_options_parse(argv):
    from srr import render_main
    a = render_main.parse(argv)
    assert a.batch_spp == 16 and a.min_spp == 16
    assert (a.adaptive, a.count_map) == ((0.05, "c.png") if argv else (None, None))
    g = render_main.count_map(np.array([0, 8, 16, 32]), 32)
    assert g.tolist() == [[0] * 3, [63] * 3, [127] * 3, [255] * 3]
