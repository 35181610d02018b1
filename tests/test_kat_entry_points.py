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


REFUSED = {
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
