"""Speculative adaptive passes on the CPU (include/srr_capi.h srr_adaptive_speculate):
the schedule function against its restatement, the restated speculative loop against
the restated resume loop bit for bit (tests/adaptive_spec_ref.py,
tests/adaptive_resume_ref.py), the preconditions of the GPU cases
(tests/test_gpu_adaptive_spec.py), the symbols, and the schedule under host sanitizers."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as ar
import adaptive_resume_ref as rr
import adaptive_spec_ref as sr
from srr import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILLS = (sr.MIXED_FILL, 20000, sr.HUGE)


def test_symbols_and_struct_size():
    L = capi.lib()
    for name in ("srr_adaptive_speculate", "srr_adaptive_last_spec_stats", "srr_adaptive_pass_width",
                 "srr_adaptive_fill_default"):
        assert hasattr(L, name), name
    assert ctypes.sizeof(capi.AdaptiveSpecStats) == 24
    # the structs of the adaptive calls are what they were
    assert ctypes.sizeof(capi.AdaptiveParams) == 20 and ctypes.sizeof(capi.AdaptiveStats) == 40
    assert capi.adaptive_fill_default() > 0


def test_pass_width_is_the_restated_schedule():
    default = capi.adaptive_fill_default()
    grid = itertools.product((1, 7, 530, 1073, 262144, 1 << 31),      # n_active
                             (0, 4, 8, 26, 29),                        # n
                             (30, 32, 1024),                           # budget
                             (1, 4, 6, 64),                            # batch_spp
                             (0, 3, 4, 8, 10, 12, 32, 1024),           # pass_spp_max: below, between and on multiples
                             (0, 1, 6000, 1 << 40))                    # fill_paths
    seen_cut = seen_floor = seen_off = 0
    for n_active, n, budget, batch, pmax, fill in grid:
        want = sr.pass_width(n_active, n, budget, batch, pmax, fill, default)
        assert capi.adaptive_pass_width(n_active, n, budget, batch, pmax, fill) == want, (n_active, n, budget, batch,
                                                                                          pmax, fill)
        assert 1 <= want <= budget - n
        k = min(max(1, pmax // batch), max(1, (fill or default) // (n_active * batch)))
        seen_cut += budget - n < k * batch
        seen_floor += pmax % batch != 0 and pmax > batch
        seen_off += pmax < batch
    assert seen_cut and seen_floor and seen_off
    # k = 1 is the pass without speculation
    assert capi.adaptive_pass_width(1073, 8, 32, 4, 0, 0) == 4
    assert capi.adaptive_pass_width(1073, 8, 32, 4, 7, 1 << 40) == 4
    assert capi.adaptive_pass_width(1073, 8, 32, 4, 10, 1 << 40) == 8
    assert capi.adaptive_pass_width(1073, 28, 30, 4, 12, 1 << 40) == 2
    for bad in ((0, 0, 8, 4, 8, 0), (1, -1, 8, 4, 8, 0), (1, 8, 8, 4, 8, 0), (1, 0, 8, 0, 8, 0), (1, 0, 8, 4, -1, 0),
                (1, 0, 8, 4, 8, -1)):
        with pytest.raises(capi.SrrError):
            capi.adaptive_pass_width(*bad)


@pytest.mark.parametrize("pass_spp_max", [8, 12, 32])
@pytest.mark.parametrize("fill", FILLS)
def test_fresh_state_is_the_plain_loops(pass_spp_max, fill):
    paths = ar.oracle_frame()["paths"]
    want, plain_log = rr.resume(paths, rr.zero_state(paths.shape[0]), ar.BUDGET, ar.BATCH, ar.MIN_SPP, ar.REL_TOL,
                                ar.ABS_EPS)
    np.testing.assert_array_equal(want["count"], ar.expected_counts()[0])
    got, log = sr.fresh(pass_spp_max, fill)
    sr.same_state(got, want)
    assert len(log) <= len(plain_log)
    assert sr.traced_of(log) - sr.discarded_of(log) == int(want["count"].sum())
    for e in log:
        assert e["w"] <= pass_spp_max and (e["k"] == 1 or e["active"].size * e["w"] <= fill)


@pytest.mark.parametrize("pass_spp_max", [8, 12, 32])
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("batch", [ar.BATCH, rr.BATCH2])
def test_resumed_state_is_the_plain_loops(pass_spp_max, fill, batch):
    want, plain_log = rr.tightened(batch)
    got, log = sr.tightened(pass_spp_max, fill, batch)
    sr.same_state(got, want)
    assert len(log) <= len(plain_log)
    assert sr.traced_of(log) - sr.discarded_of(log) == rr.paths_of(plain_log)


def test_speculation_off_is_the_plain_loop_pass_for_pass():
    _, plain_log = rr.tightened()
    for pmax in (0, ar.BATCH, 2 * ar.BATCH - 1):
        _, log = sr.tightened(pmax, sr.HUGE)
        assert [(e["level"], e["w"], e["active"].size) for e in log] == \
            [(e["level"], e["w"], e["active"].size) for e in plain_log]
        assert sr.discarded_of(log) == 0


def test_preconditions_of_the_gpu_cases():
    # one pass
    st, log = sr.fresh(32, sr.HUGE)
    sr.check_one_pass(log)
    print("one pass: stops", dict(zip(*np.unique(log[0]["stop"], return_counts=True))), "discarded", log[0]["discarded"])
    # mixed k
    st, log = sr.fresh(sr.MIXED_PASS_SPP, sr.MIXED_FILL)
    sr.check_mixed(log)
    print("mixed k:", [(e["level"], e["w"], e["active"].size, e["discarded"]) for e in log])
    # odd edges: budget 30, pass_spp_max 10 floors to two batches; batch 6 gives widths 6, 12 and 18
    st, log = sr.fresh(10, sr.HUGE, budget=30)
    assert {e["w"] for e in log} == {8, 6} and (st["count"] == 30).any()
    st, log = sr.fresh(18, sr.MIXED_FILL, budget=30, batch_spp=6)
    assert {e["w"] for e in log} == {6, 12}, [e["w"] for e in log]
    st, log = sr.fresh(18, sr.HUGE, budget=30, batch_spp=6)
    assert [e["w"] for e in log] == [18, 12]
    # the resumes speculate too and throw samples away
    for batch in (ar.BATCH, rr.BATCH2):
        _, log = sr.tightened(32, sr.HUGE, batch)
        assert any(e["k"] > 1 for e in log) and sr.discarded_of(log) > 0
    # rel_tol = 0: one pass to the budget, nothing discarded
    st, log = sr.fresh(32, sr.HUGE, rel_tol=0.0)
    assert len(log) == 1 and log[0]["discarded"] == 0 and (st["count"] == ar.BUDGET).all()


def test_schedule_under_host_sanitizers(tmp_path):
    exe = tmp_path / "adaptive_schedule_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",  # the runtimes in the program: no library order to mind
                    "-Wall", "-Werror", "-I", os.path.join(ROOT, "simple-raytracing-render_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "adaptive_schedule_host.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 checks failed" in out.stdout
