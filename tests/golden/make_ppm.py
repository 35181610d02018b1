"""Fixtures for tests/test_progressive.py::test_ppm_writer_matches_reference_outputs:
the reference's own output images (its results/*.ppm, written by
Raytracing_n.cpp:873-886), each too large to commit as text, stored as what the
test needs: the frame size, the pixels (uint8, parsed from the file) and the
file's length and SHA-256.  The writer reproduces the file byte for byte exactly
when its output has that length and digest.

    python tests/golden/make_ppm.py RESULTS_DIR      -> tests/golden/ppm_<name>.npz
"""
import glob
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main(results):
    for path in sorted(glob.glob(os.path.join(results, "*.ppm")))[:2]:
        raw = open(path, "rb").read()
        tok = raw.split()
        assert tok[0] == b"P3" and int(tok[3]) == 255
        nx, ny = int(tok[1]), int(tok[2])
        assert len(tok) == 4 + 3 * nx * ny
        px = np.array([int(t) for t in tok[4:]], np.uint8).reshape(-1, 3)
        name = os.path.splitext(os.path.basename(path))[0]
        out = os.path.join(HERE, f"ppm_{name}.npz")
        np.savez_compressed(out, nx=nx, ny=ny, pixels=px, nbytes=len(raw), sha256=hashlib.sha256(raw).hexdigest())
        print(out, nx, ny, len(raw), os.path.getsize(out))


if __name__ == "__main__":
    main(sys.argv[1])
