"""Speculative adaptive passes on C2: time, passes, traced and discarded
samples of srr_render_adaptive and of the 0.1 -> 0.05 tightening resume, with speculation
off and over a sweep of fill_paths, and fixed-spp frames for the equal-time comparison.
512 x 512, budget 1024, batch_spp = min_spp = 64; host clock around the synchronous call
with device buffers, median of 7 warm rounds, the configurations interleaved in every round.
Every frame's mean and counts are hashed: the outputs must not depend on the setting.

    python tools/adaptive_spec_sweep.py [--off-only] [--rounds 7]     (SRR_LIB=... for another library)
"""
import argparse
import ctypes
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-raytracing-render_amd"))

import torch  # noqa: E402

from srr import capi, scenes  # noqa: E402

NX = NY = 512
BUDGET, BATCH = 1024, 64
LANES = 262144
TOLS = (0.02, 0.05, 0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--factors", default="1,2,4,8,16")
    ap.add_argument("--pass-spp", type=int, default=BUDGET)
    a = ap.parse_args()
    text = scenes.s2_cornell_teapot()[0].text()
    r = capi.Renderer(text)
    can_spec = hasattr(capi.lib(), "srr_adaptive_speculate")
    fills = [] if a.off_only or not can_spec else [int(f) * LANES for f in a.factors.split(",")]
    if fills:
        fills.append(0)  # the library's default
    npix = NX * NY
    d_mean = torch.zeros((npix, 3), dtype=torch.float32, device="cuda")
    d_count = torch.zeros(npix, dtype=torch.int32, device="cuda")
    p = capi.make_params(NX, NY, BUDGET, 50)

    def params(tol):
        return capi.AdaptiveParams(ctypes.sizeof(capi.AdaptiveParams), BATCH, BATCH, tol, 1e-3)

    def setting(fill):
        if can_spec:
            r.adaptive_speculate(0 if fill is None else a.pass_spp, fill or 0)

    def digest():
        h = hashlib.sha1(d_mean.cpu().numpy().tobytes())
        h.update(d_count.cpu().numpy().tobytes())
        return h.hexdigest()[:12]

    def fresh(tol, fill):
        setting(fill)
        t0 = time.perf_counter()
        st = r.render_adaptive_device(p, params(tol), d_mean.data_ptr(), d_count.data_ptr())
        return (time.perf_counter() - t0) * 1e3, st

    def tighten(fill):
        setting(fill)
        r.render_adaptive_device(p, params(0.1), d_mean.data_ptr(), d_count.data_ptr())
        t0 = time.perf_counter()
        st = r.render_adaptive_resume_device(p, params(0.05), d_mean.data_ptr(), d_count.data_ptr())
        return (time.perf_counter() - t0) * 1e3, st

    configs = [("fresh", tol, fill) for tol in TOLS for fill in [None] + fills]
    configs += [("resume", 0.05, fill) for fill in [None] + fills]
    times = {c: [] for c in configs}
    info = {}
    for rnd in range(a.rounds + 2):  # two warm-up rounds
        for c in configs:
            kind, tol, fill = c
            ms, st = fresh(tol, fill) if kind == "fresh" else tighten(fill)
            if rnd >= 2:
                times[c].append(ms)
            sp = r.adaptive_spec_stats() if can_spec else dict(windows=st["passes"], paths_traced=st["paths"],
                                                              paths_discarded=0)
            info[c] = (st, sp, digest())
    print(f"lib {capi.LIB_PATH}")
    print("kind    tol   fill_paths   median_ms  min-max_ms     passes windows      paths     traced  discarded  "
          "world_rays  retired  sha1(mean,count)")
    for c in configs:
        kind, tol, fill = c
        st, sp, dg = info[c]
        t = times[c]
        print(f"{kind:6s} {tol:5.2f} {'off' if fill is None else fill:>11}  {statistics.median(t):9.3f}  "
              f"{min(t):6.2f}-{max(t):6.2f}  {st['passes']:6d} {sp['windows']:7d} {st['paths']:10d} "
              f"{sp['paths_traced']:10d} {sp['paths_discarded']:10d} {st['world_rays']:11d} {st['pixels_retired']:8d}  {dg}")
    if a.off_only:
        return
    # fixed frames: the 1024-spp reference, and frames of other spp for the equal-time comparison
    img = {}
    tfix = {}
    spps = [BUDGET] + list(range(64, 449, 32))
    for rnd in range(a.rounds + 1):
        for spp in spps:
            t0 = time.perf_counter()
            out = r.render(NX, NY, spp, 50)
            ms = (time.perf_counter() - t0) * 1e3
            if rnd >= 1:
                tfix.setdefault(spp, []).append(ms)
            img[spp] = out["img8"]
    ref = img[BUDGET].astype(np.float64)

    def rmse(x):
        return float(np.sqrt(np.mean((x.astype(np.float64) - ref) ** 2)))
    print("fixed frames (host arrays, so the times include the copy back): spp median_ms rmse_vs_1024")
    for spp in spps:
        print(f"  {spp:5d} {statistics.median(tfix[spp]):8.3f} {rmse(img[spp]):7.3f}")
    print("adaptive frames (host arrays): tol setting median_ms rmse_vs_1024")
    for tol in TOLS:
        for fill in (None, 0):
            setting(fill)
            ts = []
            for rnd in range(a.rounds + 1):
                t0 = time.perf_counter()
                out = r.render_adaptive(NX, NY, BUDGET, 50, batch_spp=BATCH, min_spp=BATCH, rel_tol=tol)
                ts.append((time.perf_counter() - t0) * 1e3)
            print(f"  {tol:5.2f} {'off' if fill is None else 'default':8s} {statistics.median(ts[1:]):8.3f} "
                  f"{rmse(out['img8']):7.3f}")


if __name__ == "__main__":
    main()
