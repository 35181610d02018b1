"""k_paths' ring entry and LDS budgets (csrc/kernels.h): the static_asserts there hold
for the host compiler too (the kernel repeats them against its real arrays), and the
figures DESIGN §4 quotes are the ones the header computes.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simple-raytracing-render_amd", "csrc")

PROBE = r"""
#include "kernels.h"
using namespace srr;
// ring entry: ray and RNG in words 0..10, the hit in 11..13
static_assert(kRingRayWords == 11 && kRingHitWord == 11 && kRingWordsHit == 14, "ring words");
static_assert(ring_words(false) == 11 && ring_words(true) == 14, "ring words by variant");
// 1,024-lane blocks: 344 nodes beside the 11-word ring, 248 beside the 14-word one, within 160 KB
static_assert(paths_lds_nodes(1024, true, true, false) == 344 && paths_lds_nodes(1024, true, true, true) == 248, "nodes");
static_assert(paths_lds_bytes(1024, true, true, true) <= 160 * 1024, "1,024 lanes, hit");
static_assert(paths_lds_bytes(1024, true, true, false) <= 160 * 1024, "1,024 lanes, no hit");
static_assert(paths_lds_bytes(1024, true, true, true) + 128 > 160 * 1024 - 1024, "lowered just far enough");
// 256-lane blocks: four per CU
static_assert(paths_lds_bytes(256, true, true, true) <= 40 * 1024 && paths_lds_bytes(256, true, true, false) <= 40 * 1024 &&
              paths_lds_bytes(256, true, false, false) <= 40 * 1024, "256 lanes, world in LDS");
static_assert(paths_lds_bytes(256, false, true, true) <= 40 * 1024 && paths_lds_bytes(256, false, true, false) <= 40 * 1024 &&
              paths_lds_bytes(256, false, false, false) <= 40 * 1024, "256 lanes, world in global memory");
static_assert(paths_lds_nodes(256, false, true, true) >= 64, "the global-world variant keeps a node cache");
int main() { return 0; }
"""


# PathWork::counters word by word (kernels.h PathsCtr): the words paths_finish copies into
# srr_stats keep their numbers (the kernel's immediates, the cursor and error pointers)
CTR_PROBE = r"""
#include "kernels.h"
using namespace srr;
static_assert(kCtrWorldRays == 0 && kCtrCursor == 1 && kCtrError == 2, "world rays, cursor, error");
static_assert(kCtrStackOverflows == 11 && kCtrDeepTraversals == 12, "stack overflows, deep traversals");
static_assert(kCtrMixtureCapped == 15 && kCtrSuspended == 36, "capped loops, suspended walks");
static_assert(kPathsCtrCount <= kPathsCtrWords, "the names fit the allocation");
int main() { return 0; }
"""


def test_ring_entry_and_lds_budgets_compile(tmp_path):
    compile_probe(tmp_path, PROBE)


def test_counter_slots_compile(tmp_path):
    compile_probe(tmp_path, CTR_PROBE)


def compile_probe(tmp_path, text):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = tmp_path / "probe.cpp"
    src.write_text(text)
    inc = []
    for d in ("/opt/rocm/include", os.environ.get("ROCM_PATH", "") + "/include"):
        if os.path.isdir(d):
            inc += ["-I", d]
    p = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, *inc, str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
