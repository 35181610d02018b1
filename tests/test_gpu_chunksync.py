"""k_paths' chunk-synchronous variants (kernels.hip): a 64-path chunk runs in
lockstep in a head pass, the few paths it leaves go to the wave's survivor pool and
are finished by tail passes.  A path's float operations, LCG draws and record order do
not depend on the lane or the pass it runs in: every path's raw radiance, its ray
count and the frame's world rays are bitwise the CPU oracle's, whatever SRR_TAIL_MIN
and SRR_POOL_CAP make of the flow.

Limit: the product build exposes no pass counts, so these cases cannot tell a knob that took
effect from one that was ignored (only the diagnostics build, SRR_PATHS_TIMING=1, prints head
and tail passes).  What they do show is that every flow the knobs can select gives the same paths."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_bind as ob
import parity
from srr import capi, scenes
from srr.scene import Scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simple-raytracing-render_amd", "csrc")


def _s2():
    return scenes.s2_cornell_teapot(divs=1)[0].text()


def _s2_aimed_away():
    """S2 from a camera turned so far that only a strip of the box is in the frame: most
    paths end at depth 0, inside the head pass's first shade."""
    sc = Scene()
    objs, white = scenes._cornell(sc)
    objs.append(scenes._teapot_instance(sc, white, 1))
    sc.set_world(sc.hitable_list(objs))
    sc.camera((278, 278, -800), (900, 278, 0), (0, 1, 0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    sc.set_lights(sc.hitable_list([sc.flip_normals(sc.xz_rect(213, 343, 227, 332, 554))]))
    return sc.text()


def _s2_divs10():
    return scenes.s2_cornell_teapot()[0].text()


SCENES = {"s2": _s2, "s2_away": _s2_aimed_away, "s2_d10": _s2_divs10}
_TEXT = {}
_ORACLE = {}


def _text(scene):
    if scene not in _TEXT:
        _TEXT[scene] = SCENES[scene]()
    return _TEXT[scene]


def _oracle(scene, nx, ny, spp, max_depth):
    k = (scene, nx, ny, spp, max_depth)
    if k not in _ORACLE:
        ref = ob.render(_text(scene), nx, ny, spp, max_depth, threads=8)
        for a in ("paths", "rays"):
            ref[a].setflags(write=False)
        _ORACLE[k] = ref
    return _ORACLE[k]


def _check(out, ref, what):
    pc = parity.compare_paths(out["paths"], ref["paths"])
    print(what, pc, "world_rays", out["stats"]["world_rays"], int(ref["stats"][0]))
    assert pc["bitexact"] >= parity.MIN_BITEXACT, (what, pc)
    np.testing.assert_array_equal(out["rays"], ref["rays"], err_msg=what)
    assert out["stats"]["world_rays"] == int(ref["stats"][0]), what


def _render_and_check(scene, nx, ny, spp, max_depth, what):
    out = capi.Renderer(_text(scene)).render(nx, ny, spp, max_depth, keep_paths=True)
    _check(out, _oracle(scene, nx, ny, spp, max_depth), what)
    return out


# the flows the two knobs force: the defaults; a tail pass after every head pass; survivors
# that do not fit (the head pass keeps looping, slots reused constantly); a tail pass only
# when the wave has no chunk left (the exit condition)
KNOBS = {
    "default": {},
    "tail1": {"SRR_TAIL_MIN": "1"},
    "cap1": {"SRR_POOL_CAP": "1"},
    "cap2": {"SRR_POOL_CAP": "2"},
    "cap2_tail1": {"SRR_POOL_CAP": "2", "SRR_TAIL_MIN": "1"},
    "tail_at_exit": {"SRR_POOL_CAP": "64", "SRR_TAIL_MIN": "64"},
}


# 5x3 px x 37 spp = 555 paths: eight full chunks and a last one of 43; 7x5 x 70 = 2,450:
# several waves.  max_depth 1, 2, 3, 50: a path ends on the head pass's first shade, on its
# second, at the head / tail boundary, deep.
@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,spp", [(5, 3, 37), (7, 5, 70)])
@pytest.mark.parametrize("max_depth", [1, 2, 3, 50])
@pytest.mark.parametrize("knobs", sorted(KNOBS))
@pytest.mark.parametrize("scene", ["s2", "s2_away"])
def test_paths_match_oracle_whatever_the_passes(scene, knobs, max_depth, nx, ny, spp, monkeypatch):
    for k, v in KNOBS[knobs].items():
        monkeypatch.setenv(k, v)
    _render_and_check(scene, nx, ny, spp, max_depth, f"{scene} {knobs} {nx}x{ny}x{spp} depth {max_depth}")
    if scene == "s2_away":
        assert (_oracle(scene, nx, ny, spp, max_depth)["rays"] == 1).mean() > 0.5


@pytest.mark.gpu
def test_tail_walks_suspend_beside_head_passes(monkeypatch):
    """SRR_WALK_Q=64: every tail-pass walk suspends after every node step, between head
    passes whose walks never do."""
    monkeypatch.setenv("SRR_WALK_Q", "64")
    monkeypatch.setenv("SRR_TAIL_MIN", "1")
    out = _render_and_check("s2_d10", 23, 17, 11, 50, "s2 divs 10, walk_q 64, tail_min 1")
    assert out["stats"]["walks_suspended"] > 0


@pytest.mark.gpu
def test_three_sample_windows(monkeypatch):
    """161 x 127 px: 1 MiB holds 4 samples of every pixel, so 12 spp are three windows of
    81,788 paths (not a multiple of 64).  Bitwise the one-window frame."""
    nx, ny, spp = 161, 127, 12
    r = capi.Renderer(_text("s2"))
    one = r.render(nx, ny, spp, 50, keep_paths=True)
    monkeypatch.setenv("SRR_WINDOW_MB", "1")
    many = r.render(nx, ny, spp, 50, keep_paths=True)
    assert one["stats"]["trace_launches"] == 1 and many["stats"]["trace_launches"] == 3
    np.testing.assert_array_equal(many["paths"].view(np.uint32), one["paths"].view(np.uint32))
    np.testing.assert_array_equal(many["rays"], one["rays"])
    np.testing.assert_array_equal(many["mean"].view(np.uint32), one["mean"].view(np.uint32))
    assert many["stats"]["world_rays"] == one["stats"]["world_rays"]


@pytest.mark.gpu
def test_two_frames_in_flight_equal_the_synchronous_frame():
    import torch
    nx, ny, spp = 37, 29, 7
    r = capi.Renderer(_text("s2"))
    p = capi.make_params(nx, ny, spp, 50)
    bufs = [torch.zeros((nx * ny, 3), dtype=torch.float32, device="cuda") for _ in range(3)]
    st = r.render_device(p, bufs[0].data_ptr())
    torch.cuda.synchronize()
    want = bufs[0].cpu().numpy().view(np.uint32)
    t1 = r.render_device_async(p, bufs[1].data_ptr())
    t2 = r.render_device_async(p, bufs[2].data_ptr())
    s1, s2 = r.wait(t1), r.wait(t2)
    for b in bufs[1:]:
        np.testing.assert_array_equal(b.cpu().numpy().view(np.uint32), want)
    assert s1["world_rays"] == s2["world_rays"] == st["world_rays"]


CTR_PROBE = r"""
#include "kernels.h"
using namespace srr;
static_assert(kCtrTicksHead == 42 && kCtrHeadPasses == 43 && kCtrHeadLanes == 44, "head-pass words");
static_assert(kCtrTicksTail == 45 && kCtrTailPasses == 46 && kCtrTailLanes == 47, "tail-pass words");
static_assert(kCtrTicksPretrace == 39 && kCtrShadeRounds == 41, "the words before them keep their numbers");
static_assert(kPathsCtrCount <= kPathsCtrWords, "the names fit the allocation");
static_assert(kPathsTailMin >= 1 && kPathsTailMin <= 64, "default tail threshold");
int main() { return 0; }
"""


def test_head_and_tail_counter_names_fit(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = tmp_path / "probe.cpp"
    src.write_text(CTR_PROBE)
    inc = []
    for d in ("/opt/rocm/include", os.environ.get("ROCM_PATH", "") + "/include"):
        if os.path.isdir(d):
            inc += ["-I", d]
    p = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, *inc, str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
