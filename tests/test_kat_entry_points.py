"""The device KAT entry points themselves (csrc/capi_kat.cpp), not the kernels behind them:
what they refuse before touching the device, how they fail without one, that the one table
of KAT kinds (kernels.h kKats) carries the fixtures' record widths, and that the world and
bounce KATs, which launch once per group of records, write each group's outputs back to
the records they came from."""
import ctypes
import os

import numpy as np
import pytest

import oracle_bind as ob
import test_device_bounce_kat as bounce_kat
import test_device_kat as function_kat
import test_device_world_kat as world_kat
from srr import capi

EINVAL, ENOMEM, EIO = -22, -12, -5  # include/srr_capi.h
KAT_NAMES = sorted(function_kat.OUT) + ["sqrt"]


def scene(name):
    return open(os.path.join(ob.GOLDEN, f"kat_{name}.scene")).read()


def records(name, n=8):
    return np.zeros((n, 2), np.float32) if name == "sqrt" else ob.read_kat(name)[:n].copy()


def mesh_kat(rec, variant=2, stack_cap=8):  # (capi.device_mesh_kat takes the variant by name: no way to say 4)
    L = capi.lib()
    L.srr_device_mesh_kat.argtypes = [ctypes.c_char_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    out = np.ascontiguousarray(rec, np.float32).copy()
    capi._check(L.srr_device_mesh_kat(scene("mesh").encode(), variant, 64, stack_cap, 1, out.shape[0], out.shape[1],
                                      out.ctypes.data))


def code_of(call):
    """0, or the code of the SrrError the call raises, with its message."""
    try:
        call()
    except capi.SrrError as e:
        return int(str(e).split()[2].rstrip(":")), str(e)
    return 0, ""


def world_with(col0):
    rec = records("world")
    rec[3, 0] = col0
    return rec


def bounce_with_material(m):
    rec = records("bounce")
    rec[3, 1] = m
    return rec


def fold(kind, **over):
    """A call of srr_device_fold_kat whose arguments are all good (8 rows of 4 samples), then `over`."""
    rows, spp = 8, 4
    i32 = lambda *shape, fill=0: np.full(shape, fill, np.int32)
    f32 = lambda *shape: np.zeros(shape, np.float32)
    words = dict(window=3, adaptive_fold=3, adaptive_fold_spec=3, aov_fold=8, aov_fold_emission=4, scatter=3).get(kind)
    a = dict(rows=rows, spp=spp, n_slots=rows, sums=f32(rows, 8), mom=f32(rows, 2), mean=f32(rows, 3), count=i32(rows),
             keep=np.zeros(rows, np.uint8), live=np.zeros(rows, np.uint8), lvl=i32(4), ctr=np.zeros(2, np.uint64),
             n_new=4, budget=16, batch_spp=4, min_spp=4, ns=4, n=0, w=spp, s0=0, rel_tol=0.05, abs_eps=1e-3,
             slot_out=i32(rows), pixel_out=i32(rows), n_out=i32(1), n_shard=rows, n_image=rows, index=i32(rows),
             emission=f32(rows, 3), image=f32(rows, 3))
    if words:
        a["sample"] = f32(rows, 1 if kind == "scatter" else spp, words)
    if kind == "level_finish":
        del a["rows"], a["spp"]
    a.update(over)
    capi.device_fold_kat(kind, **a)


def slots(*v):
    return np.array(v, np.int32)


REFUSED = {
    "fold: unknown kind": lambda: fold("accumulate"),
    "fold: active_slot out of range": lambda: fold("adaptive_fold", active_slot=slots(0, 1, 2, 3, 4, 5, 6, 8)),
    "fold: active_slot negative": lambda: fold("adaptive_fold_spec", active_slot=slots(0, 1, 2, 3, 4, 5, 6, -1)),
    "fold: active_slot repeated": lambda: fold("compact", active_slot=slots(0, 1, 2, 3, 4, 5, 6, 3)),
    "fold: n_slots < rows": lambda: fold("adaptive_fold", n_slots=7),
    "fold: pixels outside the output": lambda: fold("compact", pixels=slots(0, 1, 2, 3, 4, 5, 6, 8)),
    "fold: index outside the image": lambda: fold("scatter", index=slots(0, 1, 2, 3, 4, 5, 6, 8)),
    "fold: index negative": lambda: fold("scatter", index=slots(0, 1, 2, 3, 4, 5, 6, -1)),
    "fold: p0 + np beyond the shard": lambda: fold("aov_fold", p0=1),
    "fold: emission p0 + np beyond the shard": lambda: fold("aov_fold_emission", p0=1),
    "fold: negative p0": lambda: fold("aov_fold", p0=-1, n_shard=16),
    "fold: negative count": lambda: fold("level_finish", count=slots(0, 1, 2, 3, 4, 5, 6, -1)),
    "fold: count above budget": lambda: fold("level_finish", count=slots(0, 1, 2, 3, 4, 5, 6, 17)),
    "fold: count above the pass": lambda: fold("adaptive_fold_spec", w=8, s0=4, count=slots(4, 4, 4, 4, 4, 4, 4, 9)),
    "fold: batch_spp 0": lambda: fold("adaptive_fold_spec", batch_spp=0),
    "fold: spp_w 0": lambda: fold("window", spp=0),
    "fold: n_active 0": lambda: fold("adaptive_fold", rows=0),
    "fold: s0 + spp_w > w": lambda: fold("adaptive_fold_spec", w=7, s0=4),
    "fold: misalign 4": lambda: fold("window", misalign=4),
    "fold: ns 0": lambda: fold("finish", ns=0),
    "fold: n_new 0": lambda: fold("adaptive_fold", n_new=0),
    "fold: sizes overflow": lambda: fold("window", rows=1 << 24, spp=1 << 16, n_slots=1 << 24),
    "fold: rows overflow": lambda: fold("compact", rows=(1 << 24) + 1),
    "fold: no samples": lambda: fold("window", sample=None),
    "unknown name": lambda: function_kat.device_kat("erfc", records("erf")),
    "wrong width": lambda: function_kat.device_kat("erf", records("sphere")),
    "n = 0": lambda: function_kat.device_kat("erf", records("erf", 0)),
    "mesh variant 4": lambda: mesh_kat(records("mesh"), variant=4),
    "mesh stack_cap 0": lambda: mesh_kat(records("mesh"), stack_cap=0),
    "world 2.5": lambda: capi.device_world_kat(scene("world"), world_with(2.5), 0),
    "material 10^6": lambda: capi.device_bounce_kat(scene("bounce"), bounce_with_material(1e6), 1),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refused_before_the_device_is_touched(what):
    with pytest.raises(capi.SrrError, match=f"^srr error {EINVAL}: "):
        REFUSED[what]()


NO_DEVICE = {
    "fold window": (lambda: fold("window"), ENOMEM, "device allocation failed"),
    "fold spec": (lambda: fold("adaptive_fold_spec", w=8, s0=4, count=slots(4, 4, 4, 4, 4, 4, 4, 8)), ENOMEM,
                  "device allocation failed"),
    "fold compact": (lambda: fold("compact"), ENOMEM, "device allocation failed"),
    "erf": (lambda: function_kat.device_kat("erf", records("erf")), ENOMEM, "device allocation failed"),
    "sphere": (lambda: function_kat.device_kat("sphere", records("sphere")), ENOMEM, "device allocation failed"),
    "texture_image": (lambda: function_kat.device_kat("texture_image", records("texture_image")), ENOMEM,
                      "device allocation failed"),
    "mesh": (lambda: mesh_kat(records("mesh")), EIO, "no ROCm-capable device"),
    "world": (lambda: capi.device_world_kat(scene("world"), records("world"), 0), EIO, "no ROCm-capable device"),
    "bounce": (lambda: capi.device_bounce_kat(scene("bounce"), records("bounce"), 1), EIO, "no ROCm-capable device"),
}


@pytest.mark.parametrize("what", sorted(NO_DEVICE))
def test_valid_calls_without_a_device_fail_loudly(what):
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is visible")
    except ImportError:
        pass
    call, code, text = NO_DEVICE[what]
    got, msg = code_of(call)
    assert got == code and text in msg, (got, msg)


@pytest.mark.parametrize("name", KAT_NAMES)
def test_the_kat_table_has_the_fixtures_widths(name):
    """The fixture's width gets past the argument checks (the call then succeeds, or fails for
    want of a device); one float more is refused."""
    rec = records(name)
    got, msg = code_of(lambda: function_kat.device_kat(name, rec))
    assert got != EINVAL, msg
    wider = np.zeros((8, rec.shape[1] + 1), np.float32)
    with pytest.raises(capi.SrrError, match=f"^srr error {EINVAL}: KAT {name}: unexpected record width"):
        function_kat.device_kat(name, wider)


# Every third record of the fixture, in file order: the groups stay interleaved, so a launch's
# outputs go back to scattered rows.  Compared, like the whole files, with the reference's
# recorded outputs for those records.
@pytest.mark.gpu
def test_world_kat_scatters_back_every_third_record():
    rec = ob.read_kat("world")
    pick = np.arange(0, len(rec), 3)
    sub = rec[pick].copy()
    sub.setflags(write=False)
    world_kat.check((sub, scene("world"), world_kat.kat_classes.world_t_only(rec)[pick]), len(sub), 1)


@pytest.mark.gpu
def test_bounce_kat_scatters_back_every_third_record():
    rec = ob.read_kat("bounce")
    pick = np.arange(0, len(rec), 3)
    sub = rec[pick].copy()
    sub.setflags(write=False)
    classes = {c: m[pick] for c, m in bounce_kat.kat_classes.classify("bounce", rec).items()}
    bounce_kat.check((sub, scene("bounce"), classes), len(sub), 1)
