"""The renderer's device buffers are grown, kept and reused across calls (csrc/devmem.h, the
owners in csrc/renderer.h): a renderer driven through frames that grow every buffer, then
through smaller ones that reuse them, gives bitwise what a fresh renderer gives for each call.
(Allocation failures are not provoked here: tests/test_devmem.py covers them on the CPU.)"""
import numpy as np
import pytest

from srr import capi, scenes

pytestmark = pytest.mark.gpu


def _async_pair(r):
    """Two async frames of different sizes in flight together, waited for in order."""
    import torch
    frames = [capi.make_params(32, 24, 8, 12), capi.make_params(20, 12, 4, 5)]
    bufs = [torch.zeros((p.nx * p.ny, 3), dtype=torch.float32, device="cuda") for p in frames]
    tickets = [r.render_device_async(p, b.data_ptr()) for p, b in zip(frames, bufs)]
    stats = [r.wait(t) for t in tickets]
    out = {f"mean{k}": b.cpu().numpy() for k, b in enumerate(bufs)}
    out["stats"] = dict(world_rays=sum(s["world_rays"] for s in stats), paths=sum(s["paths"] for s in stats))
    return out


# each step: a call that sizes some buffer anew, or one that finds it larger than it needs
STEPS = [
    ("small", lambda r: r.render(16, 16, 4, 5)),
    ("large, kept paths", lambda r: r.render(48, 32, 8, 12, keep_paths=True)),
    ("small, kept paths", lambda r: r.render(16, 16, 4, 5, keep_paths=True)),
    ("small, kept paths, wavefront", lambda r: r.render(16, 16, 4, 5, keep_paths=True, flags=capi.FLAG_WAVEFRONT)),
    ("adaptive", lambda r: r.render_adaptive(24, 24, 32, 5, batch_spp=8, min_spp=8)),
    ("aov large", lambda r: r.render_aov(40, 24, 4, max_depth=5)),
    ("aov small", lambda r: r.render_aov(8, 8, 4, max_depth=5)),
    ("async pair", _async_pair),
    ("small again", lambda r: r.render(16, 16, 4, 5)),
]


def _same(got, want, what):
    assert got.keys() == want.keys(), what
    for k, w in want.items():
        if k == "stats":  # the counts (the times differ from run to run)
            for c in ("world_rays", "paths"):
                assert got[k][c] == w[c], f"{what}: stats[{c}]"
        else:
            assert got[k].dtype == w.dtype and got[k].shape == w.shape, f"{what}: {k}"
            np.testing.assert_array_equal(got[k].view(np.uint8), w.view(np.uint8), err_msg=f"{what}: {k}")


@pytest.mark.parametrize("scene", ["s2_teapot_mesh", "s1_no_mesh_256_lane_blocks"])
def test_reused_buffers_give_a_fresh_renderers_results(scene):
    # S2: a mesh, so the traversal-stack extension and both bounce-record column sets;
    # S1: no mesh, so k_paths in 256-lane blocks
    sc, _ = scenes.s2_cornell_teapot(divs=4) if scene.startswith("s2") else scenes.s1_cornell()
    text = sc.text()
    used = capi.Renderer(text)
    fresh = {}
    for name, step in STEPS:
        got = step(used)
        if name == "small again":  # the first call's reference serves
            want = fresh["small"]
        else:
            want = fresh[name] = step(capi.Renderer(text))
        _same(got, want, f"{scene}, step '{name}'")
    assert fresh["small, kept paths"]["paths"].shape == (256, 4, 3)
    assert np.isfinite(fresh["large, kept paths"]["mean"]).all() and fresh["large, kept paths"]["mean"].max() > 0
