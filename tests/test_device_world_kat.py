"""The world-list walk against the reference, ray by ray: the frames' own world_hit
and world_record -- the list walk with its threaded closest-so-far, sgroup_hit over
runs of plain spheres, obvh_hit over object BVHs, and the record path item -> DObj ->
prim_record -> chain_out -- replay the reference's `world` KAT records
(tests/golden/kat_world.bin: hitable_list::hit over the seven worlds of
kat_world.scene, tests/golden/README.md) through srr_device_world_kat, with the world
tables read from global memory and from their copy in LDS.  Every output column must
equal the reference's bit for bit.  An is_medium record runs the list walk a medium
makes over its boundary, which yields hit and t alone: those two columns are compared
(kat_classes.WORLD_T_ONLY_CAP bounds their share, tests/test_kat_edges.py)."""
import os

import numpy as np
import pytest

import kat_classes
import oracle_bind as ob
from srr import capi

N_IN = 11
OUT = list(range(11, 24))  # hit t obj p(3) n(3) u v, two spare
# how each fixture world must flatten (sphere groups, object BVHs): without this the KAT could test the plain list
FLATTEN = {0: (0, 0), 1: (1, 0), 2: (1, 0), 3: (3, 0), 4: (0, 4), 5: (0, 1), 6: (0, 1)}


@pytest.fixture(scope="module")
def kat():
    rec = ob.read_kat("world")
    rec.setflags(write=False)
    text = open(os.path.join(ob.GOLDEN, "kat_world.scene")).read()
    return rec, text, kat_classes.world_t_only(rec)


def test_worlds_flatten_to_groups_and_object_bvhs(kat):
    """Host only: world 0 stays a plain list, world 1 is one sphere group, world 3 three,
    worlds 4-6 hold object BVHs, and every world's packed tables fit the LDS copy."""
    rec, text, _ = kat
    assert set(rec[:, 0].astype(int)) == set(FLATTEN)
    for w, (groups, bvhs) in FLATTEN.items():
        c = capi.world_kat_counts(text, w)
        assert (c["sgroups"], c["obvhs"]) == (groups, bvhs), (w, c)
        assert c["table_bytes"] <= 8192, (w, c)  # kernels.h kPathsWorldLdsBytes
    assert capi.world_kat_counts(text, 0)["objects"] == 7
    assert capi.world_kat_counts(text, 1)["objects"] == 1 and capi.world_kat_counts(text, 1)["leaves"] == 8
    assert capi.world_kat_counts(text, 2)["objects"] == 9  # rect, the group, the box's six rects, rect
    assert capi.world_kat_counts(text, 3)["objects"] == 5  # group, translate(sphere), group, moving sphere, group


def check(kat, n, tables):
    rec, text, t_only = kat
    rec, t_only = rec[:n], t_only[:n]
    got = capi.device_world_kat(text, rec, tables)
    assert (got[:, :N_IN].view(np.uint32) == rec[:, :N_IN].view(np.uint32)).all(), "inputs changed"
    eq = (got[:, OUT].view(np.uint32) == rec[:, OUT].view(np.uint32)) | (np.isnan(got[:, OUT]) & np.isnan(rec[:, OUT]))
    eq[t_only, 2:] = True
    bad = np.flatnonzero(~eq.all(axis=1))
    per_col = {c: int((~eq[:, k]).sum()) for k, c in enumerate(OUT) if (~eq[:, k]).any()}
    classes = {}
    for i in bad:
        for c in kat_classes.classes_of("world", rec, i).split("; "):
            classes[c] = classes.get(c, 0) + 1
    for i in bad[:4]:
        print("tables", tables, "record", i, f"[{kat_classes.classes_of('world', rec, i)}]", "in", rec[i, :N_IN].tolist(),
              "\n  ref", rec[i, OUT].tolist(), "\n  dev", got[i, OUT].tolist())
    assert len(bad) == 0, (f"tables {tables}: {len(bad)} of {len(rec)} records differ; per output column {per_col}; "
                           f"classes of the differing records {classes}")


@pytest.mark.gpu
@pytest.mark.parametrize("tables", [0, 1])
def test_world_walk_bitexact(kat, tables):
    check(kat, len(kat[0]), tables)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("tables", [0, 1])
def test_partial_wave_bitexact(kat, tables, n):
    check(kat, n, tables)
