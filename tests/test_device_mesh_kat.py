"""The mesh walk against the reference, ray by ray: every walker the release build
reaches -- mesh_hit (threaded BVH2), mesh_hit4 without and with pruning, and the
quad-cooperative mesh_hit4_quad -- replays the reference's `mesh` KAT records
(tests/golden/kat_mesh.bin: bvh_node::hit over the ten adversarial meshes of
kat_mesh.scene, tests/golden/README.md) through srr_device_mesh_kat, with the LDS
stack at its full depth and at one entry, with and without the global extension (so
the walk also ends in the exact BVH2 re-walk), and for the quads with every wave
served by quads (quad_max 64) and with the busy waves sent to the per-lane walk
(quad_max 4).  Every output column must equal the reference's bit for bit."""
import os

import numpy as np
import pytest

import kat_classes
import oracle_bind as ob
from srr import capi

OUT = list(range(10, 21))  # hit t tri p(3) n(3) u v
K_STACK = 8                # kernels.h kPathsLdsStack


@pytest.fixture(scope="module")
def kat():
    rec = ob.read_kat("mesh")
    rec.setflags(write=False)
    text = open(os.path.join(ob.GOLDEN, "kat_mesh.scene")).read()
    # triangle::hit's back-face retest (is_medium) is the one hit prim_record does not restate: it is
    # front-only, as in the frames, where only a medium's boundary walk passes is_medium and takes t
    # alone (the `triangle` KAT has the same rule).  So for a medium record the columns after tri are
    # compared only where the line meets the winning triangle well inside it (float64, 1e-4 from every
    # edge): there the front test hit, and the record is the front test's.
    t_only = (rec[:, 9] != 0) & (rec[:, 10] == 1) & ~kat_classes.mesh_front_hit_sure(rec)
    return rec, text, t_only


def check(kat, n, variant, **kw):
    rec, text, t_only = kat
    rec, t_only = rec[:n], t_only[:n]
    got = capi.device_mesh_kat(text, rec, variant, **kw)
    assert (got[:, :10].view(np.uint32) == rec[:, :10].view(np.uint32)).all(), "inputs changed"
    eq = (got[:, OUT].view(np.uint32) == rec[:, OUT].view(np.uint32)) | (np.isnan(got[:, OUT]) & np.isnan(rec[:, OUT]))
    eq[t_only, 3:] = True
    bad = np.flatnonzero(~eq.all(axis=1))
    per_col = {c: int((~eq[:, k]).sum()) for k, c in enumerate(OUT) if (~eq[:, k]).any()}
    classes = {}
    for i in bad:
        for c in kat_classes.classes_of("mesh", rec, i).split("; "):
            classes[c] = classes.get(c, 0) + 1
    for i in bad[:4]:
        print(variant, kw, "record", i, f"[{kat_classes.classes_of('mesh', rec, i)}]", "in", rec[i, :10].tolist(),
              "\n  ref", rec[i, OUT].tolist(), "\n  dev", got[i, OUT].tolist())
    assert len(bad) == 0, (f"{variant} {kw}: {len(bad)} of {len(rec)} records differ; per output column {per_col}; "
                           f"classes of the differing records {classes}")


@pytest.mark.gpu
@pytest.mark.parametrize("use_gstack", [False, True])
@pytest.mark.parametrize("stack_cap", [K_STACK, 1])
@pytest.mark.parametrize("variant", ["bvh2", "bvh4", "bvh4prune"])
def test_mesh_walk_bitexact(kat, variant, stack_cap, use_gstack):
    check(kat, len(kat[0]), variant, stack_cap=stack_cap, use_gstack=use_gstack)


@pytest.mark.gpu
@pytest.mark.parametrize("use_gstack", [False, True])
@pytest.mark.parametrize("stack_cap", [K_STACK, 1])
@pytest.mark.parametrize("quad_max", [64, 4])
def test_quad_walk_bitexact(kat, quad_max, stack_cap, use_gstack):
    check(kat, len(kat[0]), "quad", quad_max=quad_max, stack_cap=stack_cap, use_gstack=use_gstack)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("variant", ["bvh2", "bvh4", "bvh4prune"])
def test_partial_wave_bitexact(kat, variant, n):
    check(kat, n, variant, stack_cap=K_STACK, use_gstack=True)
