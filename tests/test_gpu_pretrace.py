"""k_paths traces each ring chunk's camera rays in one pass where they are generated
and refilling lanes take a path over with its hit (kernels.hip): every
path's raw radiance, its ray count and the frame's world rays stay bitwise the CPU
oracle's, whatever the chunking, the misses, the depth limit, the sample windows,
the frames in flight, the variant (mesh scenes' 1,024-lane diffuse blocks pre-trace;
mesh-free S1, media and quad-cooperative keep the earlier flow, through the same
restructured loop) or the size of the LDS node set."""
import numpy as np
import pytest

import oracle_bind as ob
import parity
from srr import capi, scenes
from srr.scene import Scene

pytestmark = pytest.mark.gpu

DIVS = 1  # the teapot's smallest subdivision


def _s1():
    return scenes.s1_cornell()[0].text()


def _s2():
    return scenes.s2_cornell_teapot(divs=DIVS)[0].text()


def _s2_aimed_away():
    """S2 seen from a camera turned so far that only a strip of the box is in the
    frame: most camera rays miss, their paths end at the first shade and their lanes
    refill again in the same iteration."""
    sc = Scene()
    objs, white = scenes._cornell(sc)
    objs.append(scenes._teapot_instance(sc, white, DIVS))
    sc.set_world(sc.hitable_list(objs))
    sc.camera((278, 278, -800), (900, 278, 0), (0, 1, 0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    sc.set_lights(sc.hitable_list([sc.flip_normals(sc.xz_rect(213, 343, 227, 332, 554))]))
    return sc.text()


_ORACLE = {}


def _oracle(key, text, nx, ny, spp, max_depth):
    k = (key, nx, ny, spp, max_depth)
    if k not in _ORACLE:
        ref = ob.render(text, nx, ny, spp, max_depth, threads=8)
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


SCENES = {"s1": _s1, "s2": _s2, "s2_away": _s2_aimed_away}


# 5x3 px x 37 spp = 555 paths: eight full chunks of 64 and a last one of 43;
# 7x5 x 70 = 2,450: several waves, each with a partial last chunk somewhere
@pytest.mark.parametrize("nx,ny,spp", [(5, 3, 37), (7, 5, 70)])
@pytest.mark.parametrize("max_depth", [1, 2, 50])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_paths_rays_and_world_rays_match_oracle(scene, max_depth, nx, ny, spp):
    text = SCENES[scene]()
    out = capi.Renderer(text).render(nx, ny, spp, max_depth, keep_paths=True)
    ref = _oracle(scene, text, nx, ny, spp, max_depth)
    _check(out, ref, f"{scene} {nx}x{ny}x{spp} depth {max_depth}")
    if scene == "s2_away":  # most camera rays do miss: one world ray, black
        assert (ref["rays"] == 1).mean() > 0.5


def test_three_sample_windows(monkeypatch):
    """161 x 127 px: 1 MiB holds 4 samples of every pixel, so 12 spp are three windows of
    81,788 paths (not a multiple of 64).  Bitwise the one-window frame, whose sampled
    pixels are the oracle's."""
    text = _s2()
    nx, ny, spp = 161, 127, 12
    r = capi.Renderer(text)
    one = r.render(nx, ny, spp, 50, keep_paths=True)
    monkeypatch.setenv("SRR_WINDOW_MB", "1")
    many = r.render(nx, ny, spp, 50, keep_paths=True)
    assert one["stats"]["trace_launches"] == 1 and many["stats"]["trace_launches"] == 3
    np.testing.assert_array_equal(many["paths"].view(np.uint32), one["paths"].view(np.uint32))
    np.testing.assert_array_equal(many["rays"], one["rays"])
    np.testing.assert_array_equal(many["mean"].view(np.uint32), one["mean"].view(np.uint32))
    assert many["stats"]["world_rays"] == one["stats"]["world_rays"]
    pix = np.sort(np.random.default_rng(5).choice(nx * ny, size=200, replace=False)).astype(np.int32)
    ref = ob.render(text, nx, ny, spp, 50, pixels=pix, threads=8)
    pc = parity.compare_paths(many["paths"][pix], ref["paths"])
    assert pc["bitexact"] >= parity.MIN_BITEXACT, pc
    np.testing.assert_array_equal(many["rays"][pix], ref["rays"])


def test_two_frames_in_flight_equal_the_synchronous_frame():
    import torch
    nx, ny, spp = 37, 29, 7
    r = capi.Renderer(_s2())
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


def test_media_variant_still_matches_oracle():
    """S5 (fog): the media variants keep the earlier flow."""
    text = scenes.s4_soldier_standin(divs=4, fog=True)[0].text()
    nx, ny, spp = 16, 9, 9
    out = capi.Renderer(text).render(nx, ny, spp, 50, keep_paths=True)
    _check(out, ob.render(text, nx, ny, spp, 50, threads=8), "s5")


def test_quad_variant_still_matches_oracle(monkeypatch):
    """SRR_QUAD=1 (read when the scene is uploaded): the quad-cooperative flow, no ring."""
    monkeypatch.setenv("SRR_QUAD", "1")
    text = _s2()
    out = capi.Renderer(text).render(5, 3, 37, 50, keep_paths=True)
    _check(out, _oracle("s2", text, 5, 3, 37, 50), "s2 quad")


def test_suspending_trace_phase_beside_the_pretrace(monkeypatch):
    """1,024-lane blocks (a mesh scene's default) with SRR_WALK_Q=8: walks of the trace
    phase suspend; the ring's chunk never does, and a lane with a suspended walk leaves
    its entry untraced."""
    monkeypatch.setenv("SRR_WALK_Q", "8")
    text = scenes.s2_cornell_teapot()[0].text()
    nx, ny, spp = 23, 17, 11
    out = capi.Renderer(text).render(nx, ny, spp, 50, keep_paths=True)
    _check(out, ob.render(text, nx, ny, spp, 50, threads=8), "s2 walk_q 8")
    assert out["stats"]["walks_suspended"] > 0
    monkeypatch.setenv("SRR_WALK_Q", "64")  # every walk, after every node step
    out = capi.Renderer(text).render(nx, ny, spp, 50, keep_paths=True)
    _check(out, ob.render(text, nx, ny, spp, 50, threads=8), "s2 walk_q 64")


@pytest.mark.parametrize("cap", ["1", "248"])
def test_lds_node_set_of_one_and_of_the_maximum(cap, monkeypatch):
    """SRR_LDS_NODES_CAP (read per launch): one BVH4 node in LDS, and the 1,024-lane
    block's whole set (248 beside the 14-word ring).  The 6,400-triangle teapot has more
    nodes than that, so both sides of the LDS / global node fetch run."""
    monkeypatch.setenv("SRR_LDS_NODES_CAP", cap)
    text = scenes.s2_cornell_teapot()[0].text()
    nx, ny, spp = 23, 17, 11
    out = capi.Renderer(text).render(nx, ny, spp, 50, keep_paths=True)
    _check(out, _oracle("s2_d10", text, nx, ny, spp, 50), f"lds nodes {cap}")
