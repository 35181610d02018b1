"""Record the host libm's results on a few thousand inputs per function
(tests/golden/libm_pins.npz), so that tests/test_device_libm.py can say whether
the machine it runs on has the libm the suite's bit-exact claims refer to:
glibc 2.35 with the x86-64 FMA ifunc variants, as for the MERL KATs
(tests/golden/make_golden.py).  Like make_golden.py it refuses to regenerate on
another glibc or on a CPU without FMA / AVX2.

    python tests/golden/make_libm_pins.py

Per function `f` of oracle_libm: f.x, f.y (two-operand functions), f.out0, f.out1
(sincosf / sincos): 4,096 inputs taken at a fixed stride from the sweep's own input
set (tests/libm_inputs.py), so edges, specials and every exponent are among them.
log and pow, which have no restatement, take the medium's u = k / 2^32 and the
dielectric's (1 - cosine, 5)."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import libm_inputs as li  # noqa: E402
import oracle_bind as ob  # noqa: E402
from make_golden import MERL_LIBM_PIN, host_libm  # noqa: E402

N = 4096


def pick(a, n=N):
    idx = np.unique(np.linspace(0, a.size - 1, n).astype(np.int64))
    return idx


def main():
    libm = host_libm()
    if libm != MERL_LIBM_PIN:
        sys.exit(f"libm_pins.npz NOT regenerated: this host's libm {libm} is not the pinned {MERL_LIBM_PIN}")
    out = {"libm": np.array(f"{libm['glibc']}, FMA ifunc variants")}
    by_libm = {v[0]: k for k, v in li.FUNCS.items()}
    rng = np.random.default_rng([li.SEED, 99])
    for name in ob.LIBM_F32 + ob.LIBM_F64:
        if name == "log":
            k = np.concatenate([np.arange(0, 1024), (1 << 32) - 1 - np.arange(1024),
                                rng.integers(0, 1 << 32, size=N - 2048)]).astype(np.float64)
            x, y = k / 4294967296.0, None
        elif name == "pow":
            x = np.concatenate([rng.random(N - 2, dtype=np.float32), np.float32([0, 1])]).astype(np.float64)
            y = np.full_like(x, 5.0)
        else:
            x, y = li.inputs(by_libm[name])
            idx = pick(x)
            x, y = x[idx], None if y is None else y[idx]
        with np.errstate(all="ignore"):
            r = ob.libm(name, x, y)
        r = r if isinstance(r, tuple) else (r,)
        out[f"{name}.x"] = x
        if y is not None:
            out[f"{name}.y"] = y
        for k, o in enumerate(r):
            out[f"{name}.out{k}"] = o
        print(name, x.size, "inputs")
    np.savez_compressed(os.path.join(HERE, "libm_pins.npz"), **out)


if __name__ == "__main__":
    main()
