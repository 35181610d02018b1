"""bench.py --dump-outputs and --full.

* CPU: dump_outputs writes the frame as float32 and, past the 64 MB cap, the
  same seeded pixel sample on every call.
* GPU: a plain run's line has no cpu_baseline and its dumped frame is bitwise
  the --save-frame frame and the same from run to run; --full adds cpu_baseline
  and leaves the frame unchanged; --steps sets the number of timed frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ARGS = ["--gpus", "1", "--warmup", "1", "--scene", "s2", "--nx", "96", "--ny", "80", "--spp", "16"]


def test_dump_outputs_small_frame(tmp_path):
    frame = np.random.default_rng(3).random((96 * 80, 3), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "d"), frame, 123456)
    got = np.load(tmp_path / "d" / "frame.npy")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, frame)
    rays = np.load(tmp_path / "d" / "world_rays.npy")
    assert rays.dtype == np.float64 and rays.tolist() == [123456.0]


def test_dump_outputs_caps_at_64mb(tmp_path):
    n = (bench.DUMP_MAX_BYTES // 12) + 1000  # a [n, 3] float32 frame just past the cap
    frame = np.zeros((n, 3), dtype=np.float32)
    frame[:, 0] = np.arange(n)  # (row numbers: exact in float32 below 2^24)
    frame[:, 2] = 0.5
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), frame, 1)
    a, b = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "b" / "frame.npy")
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_MAX_BYTES
    assert a.dtype == np.float32 and a.shape[1] == 3 and a.shape[0] > n // 2
    np.testing.assert_array_equal(a, b)  # the same sample every time
    rows = a[:, 0].astype(np.int64)  # the sampled pixels, ascending, each a whole row of the frame
    assert (np.diff(rows) > 0).all()
    np.testing.assert_array_equal(a, frame[rows])


def _run(*extra):
    rc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, *extra], capture_output=True,
                        text=True, timeout=300, cwd=ROOT)
    assert rc.returncode == 0, rc.stderr[-3000:]
    lines = [l for l in rc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, rc.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_full_and_dump(tmp_path):
    d1, d2, d3, f1 = (str(tmp_path / n) for n in ("d1", "d2", "d3", "f1.npy"))
    j1 = _run("--steps", "2", "--dump-outputs", d1, "--save-frame", f1)
    j2 = _run("--steps", "3", "--dump-outputs", d2)
    j3 = _run("--steps", "2", "--dump-outputs", d3, "--full", "--cpu-seconds", "0.2")
    for j, steps in ((j1, 2), (j2, 3), (j3, 2)):
        assert j["steps"] == steps and j["ms_per_step"] > 0 and j["value"] > 0
        assert j["unit"] == "Msamples/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
        # value = world rays of the timed steps over their time
        assert j["value"] == pytest.approx(j["config"]["world_rays_per_step"] / j["ms_per_step"] / 1e3, rel=1e-3)
    assert "cpu_baseline" not in j1 and "cpu_baseline" not in j2
    assert j3["cpu_baseline"]["value"] > 0
    frames = [np.load(os.path.join(d, "frame.npy")) for d in (d1, d2, d3)]
    assert frames[0].dtype == np.float32 and frames[0].shape == (96 * 80, 3)
    np.testing.assert_array_equal(frames[0].view(np.uint32), np.load(f1).view(np.uint32))
    for f in frames[1:]:
        np.testing.assert_array_equal(f.view(np.uint32), frames[0].view(np.uint32))
    rays = [np.load(os.path.join(d, "world_rays.npy")) for d in (d1, d2, d3)]
    assert rays[0].dtype == np.float64 and rays[0].tolist() == [float(j1["config"]["world_rays_per_step"])]
    assert rays[1].tolist() == rays[0].tolist() == rays[2].tolist()
