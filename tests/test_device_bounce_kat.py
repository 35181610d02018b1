"""One shading bounce against the reference, record by record: the product's shading
code -- family_of, hit_emitted and scatter<family> of the wavefront engine (variant 0), and
the path kernel's split diffuse bounce with bsdf_dead, skip_mixture and the wave-cooperative
coop_mixture (variant 1, with deep_tries 32 and 0) -- replays the reference's `bounce` KAT
records (tests/golden/kat_bounce.bin: color() itself over a probe world, the light lists
and the materials of kat_bounce.scene, tests/golden/README.md) through
srr_device_bounce_kat.  Every output column of every record must equal the reference's bit
for bit (NaN equals NaN: payloads differ between x86 and gfx950), except the attempts
column, a class label of the reference's: the LCG state after the bounce pins the draws.
A failure names the classes (tests/kat_classes.py) of the differing records, and with them
the shading function whose inputs they stress."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import kat_classes
import oracle_bind as ob
from srr import capi

N_IN = 25
ATTEMPTS = 36
OUT = [c for c in range(25, 43) if c != ATTEMPTS]  # scattered origin(3) dir(3) time colour(3) | lcg(2) pcg(4)
NAMES = {25: "scattered", 26: "origin.x", 27: "origin.y", 28: "origin.z", 29: "dir.x", 30: "dir.y", 31: "dir.z", 32: "time",
         33: "colour.r", 34: "colour.g", 35: "colour.b", 37: "lcg.lo", 38: "lcg.hi", 39: "pcg.0", 40: "pcg.1", 41: "pcg.2",
         42: "pcg.3"}
# how each light list must flatten: (lights, non-sampling, xz_rect, sphere, triangle)
FLATTEN = {0: (1, 0, 1, 0, 0), 1: (3, 0, 1, 1, 1), 2: (1, 0, 0, 1, 0), 3: (2, 1, 1, 0, 0), 4: (2, 2, 0, 0, 0),
           5: (0, 0, 0, 0, 0), 6: (2, 0, 2, 0, 0), 7: (5, 0, 2, 1, 2), 8: (8, 7, 1, 0, 0)}
REF_SRC = os.path.join("/root/reference", "Raytracing_n", "Raytracing_n.cpp")
SCENE = os.path.join(ob.GOLDEN, "kat_bounce.scene")


@pytest.fixture(scope="module")
def kat():
    rec = ob.read_kat("bounce")
    rec.setflags(write=False)
    return rec, open(SCENE).read(), kat_classes.classify("bounce", rec)


def test_light_lists_flatten_to_their_kinds(kat):
    """Host only: every list flattens to the kinds the fixture is built for -- list 3 one
    non-sampling member and one xz_rect, list 4 non-sampling members only, list 5 empty,
    list 8 seven non-sampling members -- and all 17 materials survive flattening."""
    rec, text, _ = kat
    assert set(rec[:, 0].astype(int)) == set(FLATTEN)
    assert set(rec[:, 1].astype(int)) == set(range(17))
    for l, want in FLATTEN.items():
        c = capi.bounce_kat_counts(text, l)
        assert (c["lights"], c["none"], c["xz_rect"], c["sphere"], c["triangle"]) == want, (l, c)
        assert c["materials"] == 17, (l, c)


def test_the_file_has_one_depth_limit_and_no_capped_loop(kat):
    rec, _, _ = kat
    assert (rec[:, 18] == rec[0, 18]).all()
    assert rec[:, ATTEMPTS].max() <= 4096  # far below kMixtureGuard: tests/test_mixture_cap.py stays the test of the cap


@pytest.mark.skipif(not os.path.exists(REF_SRC) or shutil.which("g++") is None or shutil.which("make") is None,
                    reason="needs the reference checkout (development container)")
def test_the_generator_refuses_to_hang(tmp_path):
    """A loop that cannot end (a lambertian seen from the front, non-sampling lights only) stops
    the generator with the record's number: the reference's own loop has no bound.  The harness
    is built here from this tree's oracle/ref into the test's own directory (nothing of it is
    kept), so that no harness left by an earlier build is the one asked."""
    out = tmp_path / "_ref"
    b = subprocess.run(["make", "-C", os.path.join(ob.ROOT, "oracle", "ref"), f"OUT={out}"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    p = subprocess.run([str(out / "ref_harness"), "kat", "bounce_hang", "3", "1", str(tmp_path / "x.bin"), SCENE],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert "record 0: more than 4096 mixture attempts" in p.stderr, p.stderr
    assert not (tmp_path / "x.bin").exists()


def check(kat, n, variant, deep_tries=32):
    rec, text, classes = kat
    rec = rec[:n]
    sent = rec.copy()
    sent[:, OUT] = -12345.0  # (a kernel that writes nothing must not pass)
    got = capi.device_bounce_kat(text, sent, variant, deep_tries)
    keep = list(range(N_IN)) + [ATTEMPTS]
    assert (got[:, keep].view(np.uint32) == rec[:, keep].view(np.uint32)).all(), "inputs changed"
    eq = (got[:, OUT].view(np.uint32) == rec[:, OUT].view(np.uint32)) | (np.isnan(got[:, OUT]) & np.isnan(rec[:, OUT]))
    bad = np.flatnonzero(~eq.all(axis=1))
    per_col = {NAMES[c]: int((~eq[:, k]).sum()) for k, c in enumerate(OUT) if (~eq[:, k]).any()}
    per_class = {c: int(m[bad].sum()) for c, m in classes.items() if m[bad].any()}
    for i in bad[:4]:
        print("variant", variant, "deep_tries", deep_tries, "record", i, "[" + "; ".join(c for c, m in classes.items() if m[i]) + "]",
              "in", rec[i, :N_IN].tolist(), "\n  ref", rec[i, 25:].tolist(), "\n  dev", got[i, 25:].tolist())
    assert len(bad) == 0, (f"variant {variant}, deep_tries {deep_tries}: {len(bad)} of {len(rec)} records differ; per output "
                           f"column {per_col}; classes of the differing records {per_class}")


@pytest.mark.gpu
def test_sequential_bounce_bitexact(kat):
    check(kat, len(kat[0]), 0)


@pytest.mark.gpu
@pytest.mark.parametrize("deep_tries", [32, 0])
def test_cooperative_bounce_bitexact(kat, deep_tries):
    check(kat, len(kat[0]), 1, deep_tries)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("deep_tries", [32, 0])
def test_cooperative_partial_wave_bitexact(kat, deep_tries, n):
    check(kat, n, 1, deep_tries)
