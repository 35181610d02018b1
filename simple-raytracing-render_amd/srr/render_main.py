"""The reference's program, ``main()`` (Raytracing_n.cpp:882-952), over srr:
pick a scene by ``sceneid``, build it with the reference's builder (restated in
srr/ref_scenes.py, pinned to the reference's own builder code by
tests/test_ref_builders_compile.py), render nx x ny x ns with maxDepth on the
GPU, print the elapsed milliseconds and write the P3 PPM (the tone map and byte
format of Raytracing_n.cpp:850-886).

    python -m srr.render_main [--sceneid 2] [--nx 1000] [--ny 1000] [--ns 50] [--max-depth 50] [--out out.ppm]
                              [--gpus N]   (srr_renderer_create_multi: one RCCL gather at frame end)
                              [--adaptive REL_TOL [--batch-spp 16] [--min-spp 16] [--count-map FILE]
                                                  [--adaptive-pass-spp N [--adaptive-fill P]]]
                                           (srr_render_adaptive: --ns is the per-pixel budget; one GPU;
                                            --adaptive-pass-spp: speculative passes of up to N samples,
                                            srr_adaptive_speculate -- the same image in fewer passes)
                              [--denoise [--aov-spp N] [--aov-out PREFIX]]
                                           (srr_denoise over the first-hit AOVs of srr_render_aov; one GPU;
                                            --out is the tone-mapped denoised frame; PREFIX_albedo.png,
                                            PREFIX_normal.png, PREFIX_depth.png)
                              [--denoise-var [--aov-spp N] [--aov-out PREFIX]]
                                           (the same with srr_denoise_var, guided by the variance of every
                                            pixel's mean luminance; not with --denoise; without --adaptive the
                                            frame is one srr_render_adaptive pass at rel_tol 0, bitwise the
                                            fixed-spp frame)
                              [--aov-through-specular]
                                           (with --denoise, --denoise-var or --aov-out: their AOVs are those of
                                            the first hit that is neither metal nor dielectric,
                                            srr_render_aov_through; one GPU)
                              [--denoise-emission]
                                           (with --denoise or --denoise-var: the filter runs on the frame less
                                            its emission, srr_render_aov_emission over the frame's own samples
                                            -- the adaptive frame's counts under --adaptive -- and adds it back;
                                            --aov-out also writes PREFIX_emission.png; one GPU)

Defaults are the reference's globals (Raytracing_n.cpp:39-43).  Differences, all
forced by the reference: its 8 render threads race on shared state
and its pixel mapping scrambles non-square frames (Q12); srr renders every
(pixel, sample) path with its per-path seed and writes the intended image.
Assets are read from $SRR_CONTENTS (default /root/reference/contents), which
the builders need (images, meshes)."""
from __future__ import annotations

import argparse
import sys
import time

from . import capi, ref_scenes

SCENE_NAMES = {k: f.__name__ for k, f in ref_scenes.BY_SCENEID.items()}


def parse(argv=None):
    ap = argparse.ArgumentParser(prog="python -m srr.render_main", description=__doc__.split("\n\n")[0])
    ap.add_argument("--sceneid", type=int, default=2, choices=sorted(ref_scenes.BY_SCENEID),
                    help="; ".join(f"{k}: {v}" for k, v in SCENE_NAMES.items()))
    ap.add_argument("--nx", type=int, default=1000)
    ap.add_argument("--ny", type=int, default=1000)
    ap.add_argument("--ns", type=int, default=50, help="samples per pixel")
    ap.add_argument("--max-depth", type=int, default=50)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--gpus", type=int, default=1,
                    help="render on devices device .. device+gpus-1 (pixels dealt round-robin, one RCCL gather)")
    ap.add_argument("--contents", default=None, help="the reference's contents/ directory (assets)")
    ap.add_argument("--out", default="out.ppm")
    ap.add_argument("--adaptive", type=float, default=None, metavar="REL_TOL",
                    help="adaptive sampling: --ns is the per-pixel budget; a pixel stops once the relative "
                         "standard error of its mean luminance is at most REL_TOL (one GPU)")
    ap.add_argument("--batch-spp", type=int, default=16, help="adaptive: samples per pixel and pass")
    ap.add_argument("--min-spp", type=int, default=16, help="adaptive: no pixel stops with fewer samples")
    ap.add_argument("--count-map", default=None, metavar="FILE",
                    help="adaptive: PNG of the samples each pixel took, as grey level count / ns")
    ap.add_argument("--adaptive-pass-spp", type=int, default=0, metavar="N",
                    help="adaptive: speculative passes of up to N samples per pixel (0: off); the image does not change")
    ap.add_argument("--adaptive-fill", type=int, default=0, metavar="P",
                    help="adaptive: the pass size, in paths, that speculative passes aim at (0: the library's default)")
    ap.add_argument("--denoise", action="store_true",
                    help="filter the frame with the a-trous denoiser over its first-hit AOVs (one GPU)")
    ap.add_argument("--denoise-var", action="store_true",
                    help="filter the frame with the variance-guided a-trous denoiser (one GPU; not with --denoise)")
    ap.add_argument("--aov-spp", type=int, default=None, help="samples of the AOVs (default min(ns, 16))")
    ap.add_argument("--aov-out", default=None, metavar="PREFIX",
                    help="write PREFIX_albedo.png, PREFIX_normal.png, PREFIX_depth.png")
    ap.add_argument("--aov-through-specular", action="store_true",
                    help="the AOVs of --denoise, --denoise-var and --aov-out follow mirrors and glass to the first "
                         "diffuse hit (one GPU)")
    ap.add_argument("--denoise-emission", action="store_true",
                    help="with --denoise or --denoise-var: filter the frame less its emission and add it back (one GPU)")
    return ap.parse_args(argv)


def aov_images(aov):
    """The AOVs as 8-bit rgb: 255.99 * albedo, 255.99 * (normal / 2 + 1/2), grey 255.99 * depth / max."""
    import numpy as np

    def byte(v):
        return (np.float32(255.99) * v.astype(np.float32)).astype(np.int64).clip(0, 255).astype(np.uint8)
    z = aov["depth"]
    zmax = z.max() if z.size else np.float32(0)
    grey = byte(z / zmax if zmax > 0 else np.zeros_like(z))
    return dict(albedo=byte(aov["albedo"]), normal=byte(aov["normal"] * np.float32(0.5) + np.float32(0.5)),
                depth=np.repeat(grey[:, None], 3, axis=1))


def count_map(count, max_spp):
    """Per-pixel sample counts as 8-bit grey rgb: 255 * count / max_spp, rounded down."""
    import numpy as np
    g = (np.asarray(count, np.int64) * 255 // max(1, max_spp)).clip(0, 255).astype(np.uint8)
    return np.repeat(g[:, None], 3, axis=1)


def main(argv=None) -> int:
    a = parse(argv)
    if a.denoise and a.denoise_var:
        print("--denoise and --denoise-var exclude each other", file=sys.stderr)
        return 2
    if a.denoise_var and a.gpus != 1:
        print("--denoise-var needs one GPU", file=sys.stderr)
        return 2
    if a.aov_through_specular and not (a.denoise or a.denoise_var or a.aov_out):
        print("--aov-through-specular needs --denoise, --denoise-var or --aov-out", file=sys.stderr)
        return 2
    if a.aov_through_specular and a.gpus != 1:
        print("--aov-through-specular needs one GPU", file=sys.stderr)
        return 2
    if a.denoise_emission and not (a.denoise or a.denoise_var):
        print("--denoise-emission needs --denoise or --denoise-var", file=sys.stderr)
        return 2
    if a.denoise_emission and a.gpus != 1:
        print("--denoise-emission needs one GPU", file=sys.stderr)
        return 2
    sc = ref_scenes.BY_SCENEID[a.sceneid](float(a.nx) / float(a.ny), contents=a.contents)  # :894-919
    r = (capi.Renderer(sc.text(), device=a.device) if a.gpus == 1 else
         capi.Renderer(sc.text(), devices=list(range(a.device, a.device + a.gpus))))
    if a.adaptive is None and a.count_map:
        print("--count-map needs --adaptive", file=sys.stderr)
        return 2
    if (a.denoise or a.aov_out) and a.gpus != 1:
        print("--denoise and --aov-out need one GPU", file=sys.stderr)
        return 2
    if a.adaptive is None and (a.adaptive_pass_spp or a.adaptive_fill):
        print("--adaptive-pass-spp and --adaptive-fill need --adaptive", file=sys.stderr)
        return 2
    if a.adaptive_pass_spp or a.adaptive_fill:
        r.adaptive_speculate(a.adaptive_pass_spp, a.adaptive_fill)
    t0 = time.perf_counter()
    if a.adaptive is not None:
        out = r.render_adaptive(a.nx, a.ny, a.ns, a.max_depth, batch_spp=a.batch_spp, min_spp=a.min_spp,
                                rel_tol=a.adaptive, tile=1)
    elif a.denoise_var:  # the fixed-spp frame as one adaptive pass, which keeps its moments
        out = r.render_adaptive(a.nx, a.ny, a.ns, a.max_depth, batch_spp=a.ns, min_spp=a.ns, rel_tol=0.0, tile=1)
    else:
        out = r.render(a.nx, a.ny, a.ns, a.max_depth, tile=1)
    if a.denoise or a.denoise_var or a.aov_out:
        aov = r.render_aov(a.nx, a.ny, a.aov_spp or min(a.ns, 16), max_depth=a.max_depth,
                           through_specular=a.aov_through_specular)
        emission = None
        if a.denoise_emission:  # the emission of exactly the samples the frame holds, in a call of its own
            em = r.render_aov(a.nx, a.ny, a.ns, capi.AOV_EMISSION, max_depth=a.max_depth,
                              through_specular=a.aov_through_specular,
                              count=out["count"] if a.adaptive is not None else None)["emission"]
            emission = em.reshape(a.ny, a.nx, 3)
        if a.denoise:
            shape = (a.ny, a.nx, 3)
            den = capi.denoise(out["mean"].reshape(shape), aov["albedo"].reshape(shape), aov["normal"].reshape(shape),
                               aov["depth"].reshape(a.ny, a.nx), device=a.device, emission=emission)
            out["img8"] = capi.tonemap(den.reshape(-1, 3))
        if a.denoise_var:
            shape = (a.ny, a.nx, 3)
            var = r.adaptive_variance(out["count"])
            den, _ = capi.denoise_var(out["mean"].reshape(shape), var.reshape(a.ny, a.nx), aov["albedo"].reshape(shape),
                                      aov["normal"].reshape(shape), aov["depth"].reshape(a.ny, a.nx), device=a.device,
                                      want_var=False, emission=emission)
            out["img8"] = capi.tonemap(den.reshape(-1, 3))
        if a.aov_out:
            for k, img in aov_images(aov).items():
                capi.write_png(f"{a.aov_out}_{k}.png", a.nx, a.ny, img)
            if emission is not None:  # tone-mapped like the frame
                capi.write_png(f"{a.aov_out}_emission.png", a.nx, a.ny, capi.tonemap(emission.reshape(-1, 3)))
    ms = (time.perf_counter() - t0) * 1e3
    print(f"{int(ms)}ms")  # :944-947
    capi.write_ppm(a.out, a.nx, a.ny, out["img8"])
    st = out["stats"]
    if a.adaptive is not None:
        sp = r.adaptive_spec_stats()
        print(f"adaptive: {st['paths']} of {a.nx * a.ny * a.ns} samples in {st['passes']} passes, "
              f"{st['pixels_retired']} pixels stopped early; {sp['paths_traced']} traced, "
              f"{sp['paths_discarded']} discarded", file=sys.stderr)
        if a.count_map:
            capi.write_png(a.count_map, a.nx, a.ny, count_map(out["count"], a.ns))
    print(f"{SCENE_NAMES[a.sceneid]}: {a.nx}x{a.ny}x{a.ns}, {st['world_rays']} world rays, "
          f"{st['world_rays'] / max(ms, 1e-3) / 1e3:.1f} Msamples/s -> {a.out}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
