"""Generate the golden fixtures in tests/golden/ by running the REFERENCE's own
code (oracle/_ref/ref_harness, built by `make -C oracle ref` from
/root/reference -- development container only).  The fixtures are data: scene
descriptions (inputs) and the reference's outputs for them.

    python tests/golden/make_golden.py
    python tests/golden/make_golden.py --kats sphere rect ...   # only these KATs; every
                                                                # other fixture stays as it is

Fixture list and layouts: tests/golden/README.md.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "simple-raytracing-render_amd"))

from srr import scenes  # noqa: E402

HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")

# (name, scene factory, nx, ny, spp, max_depth)
RENDERS = [
    ("s1", lambda: scenes.s1_cornell()[0], 32, 32, 16, 50),
    ("s2", lambda: scenes.s2_cornell_teapot()[0], 32, 32, 16, 50),
    ("s3", lambda: scenes.s3_cornell_teapot_microfacet()[0], 32, 32, 16, 50),
    ("s3_metal", lambda: scenes.s3_cornell_teapot_microfacet("metal")[0], 32, 32, 16, 50),
    ("s4_small", lambda: scenes.s4_soldier_standin(divs=8)[0], 32, 18, 8, 50),
    ("s5_small", lambda: scenes.s4_soldier_standin(divs=8, fog=True)[0], 32, 18, 8, 50),
    ("s2_depth3", lambda: scenes.s2_cornell_teapot()[0], 16, 16, 8, 3),
    # the reference's as-shipped teapot (teapot.h:77, divs 100: 640,000 triangles)
    ("s2_d100", lambda: scenes.s2_cornell_teapot(divs=100)[0], 32, 32, 8, 50),
    # sphere and triangle lights next to the rect in the light list
    ("s6_lights", lambda: scenes.s6_mixed_lights()[0], 32, 32, 16, 50),
    # C4 / C5 stand-ins at their configured mesh (divs 40: 102,400 triangles)
    ("s4_d40", lambda: scenes.s4_soldier_standin(divs=40)[0], 64, 36, 4, 50),
    ("s5_d40", lambda: scenes.s4_soldier_standin(divs=40, fog=True)[0], 64, 36, 4, 50),
]

KATS = [("erf", 512), ("beckmann11", 512), ("beckmann_dist", 512), ("beckmann_pdf", 512), ("cosine_pdf", 256),
        ("orennayar_pdf", 256), ("dielectric", 256), ("metal", 256), ("triangle", 1024), ("aabb", 1024),
        ("camera", 256), ("lights", 256), ("light_list", 256), ("merl", 2048), ("merl_same", 4096),
        # scene KATs: a constructed half of edge blocks and a pseudo-random half (README.md)
        ("sphere", 1024), ("moving_sphere", 1024), ("rect", 1024), ("box", 1024), ("xform", 1024), ("medium", 1024),
        ("isotropic", 1024), ("texture_checker", 1024), ("texture_noise", 1024), ("texture_image", 1024),
        # the mesh walk: bvh_node::hit over the ten meshes of kat_mesh.scene (README.md)
        ("mesh", 1024)]


# The MERL KATs' out == in records are decided by the last-ulp rounding of glibc's
# dbl-64 sin / cos / sincos / acos / atan2 (include/srr/merl.h): they are pinned to
# the oracle port as built on glibc 2.35 with the FMA ifunc variants (__sin_fma,
# __cos_fma, __ieee754_acos_fma, __ieee754_atan2_fma), which the device restates.
# Another glibc, or a CPU without FMA (the ifunc then picks the SSE2 builds), gives
# other cells; such a host must not regenerate them.
MERL_LIBM_PIN = {"glibc": "glibc 2.35", "fma_ifunc": True}
MERL_KATS = ("merl", "merl_same")


def host_libm():
    """The glibc version and whether its ifunc resolvers select the FMA variants
    (glibc picks them when the CPU has FMA and AVX2)."""
    flags = set()
    with open("/proc/cpuinfo") as f:
        for line in f:
            if line.startswith("flags"):
                flags = set(line.split(":", 1)[1].split())
                break
    return {"glibc": os.confstr("CS_GNU_LIBC_VERSION"), "fma_ifunc": "fma" in flags and "avx2" in flags}


def run(*args):
    out = subprocess.run([HARNESS, *map(str, args)], check=True, capture_output=True, text=True)
    return out.stdout


MESH_SCENE = os.path.join(HERE, "kat_mesh.scene")
N_KAT_MESHES = 10


def mesh_scene_text():
    """The ten fixture meshes of the `mesh` KAT (README.md): `bvh` objects over
    triangles, vertices on the quarter-integer lattice except for the two teapots."""
    import math
    import tempfile

    import numpy as np

    def h(i, j):  # height of the 8 x 8 field's vertex (i, j): quarters in [0, 1.75]
        return 0.25 * (((i * 7 + j * 13 + i * j * 5) ^ (i + 3 * j)) % 8)

    def grid(z):
        tris = []
        for j in range(8):
            for i in range(8):
                a, b, c, d = ((i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1))
                v = lambda p: (float(p[0]), float(p[1]), float(z(*p)))  # noqa: E731
                tris += [(v(a), v(b), v(c)), (v(a), v(c), v(d))]
        return tris

    def teapot(scale, off):
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "t.f32")
            run("teapot", scale, 3, path)
            p = np.fromfile(path, np.float32).reshape(-1, 12)[:, :9].reshape(-1, 3, 3)
        p = (p + np.float32(off)).astype(np.float32)
        return [tuple(tuple(float(x) for x in vtx) for vtx in t) for t in p]

    field = grid(h)
    fan = []
    for k in range(96):  # rim points of radius about 64, snapped to the lattice, heights in [-2, 2]
        rim = [(round(4 * 64 * math.cos(2 * math.pi * q / 96)) / 4, round(4 * 64 * math.sin(2 * math.pi * q / 96)) / 4,
                0.25 * ((q * 5) % 17 - 8)) for q in (k, (k + 1) % 96)]
        fan.append(((0.0, 0.0, 0.0), rim[0], rim[1]))
    zero_area = [((float(k), 1.0, 0.5), (float(k), 1.0, 0.5), (k + 1.0, 2.0, 0.75)) if k % 2 == 0 else
                 ((float(k), 0.0, 0.25), (k + 1.0, 1.0, 0.5), (k + 2.0, 2.0, 0.75)) for k in range(8)]
    meshes = [
        [((0.0, 0.0, 0.0), (4.0, 0.0, 0.5), (0.0, 4.0, 1.0))],  # (tilted: a flat triangle's box is never entered)
        [((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0)), ((4.0, 0.0, 0.0), (4.0, 4.0, 1.0), (0.0, 4.0, 0.0))],
        [((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0)), ((4.0, 0.0, 0.0), (4.0, 4.0, 1.0), (0.0, 4.0, 0.0)),
         ((4.0, 0.0, 0.0), (8.0, 0.0, 0.5), (4.0, 4.0, 1.0))],
        [((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0)), ((4.0, 0.0, 0.0), (4.0, 4.0, 1.0), (0.0, 4.0, 0.0)),
         ((4.0, 0.0, 0.0), (8.0, 0.0, 0.5), (4.0, 4.0, 1.0)), ((8.0, 0.0, 0.5), (8.0, 4.0, 0.25), (4.0, 4.0, 1.0)),
         ((0.0, 4.0, 0.0), (4.0, 4.0, 1.0), (2.0, 8.0, 0.75))],
        field,
        grid(lambda i, j: 2.0),
        field[:32] + field[:32] + zero_area,
        fan,
        teapot(1e-3, 1000.0),
        teapot(60.0, 0.0),
    ]
    f32 = lambda x: repr(float(np.float32(x)))  # noqa: E731  (shortest decimal that reads back as the float32)
    out = ["srr_scene 1", "# the `mesh` KAT's fixture meshes (README.md): obj 100000 + m is mesh m",
           "tex 0 const 0.5 0.5 0.5", "mat 0 lambertian 0"]
    nid = 0
    roots = []
    for m, tris in enumerate(meshes):
        ids = []
        for t in tris:
            pts = " ".join(f32(x) for vtx in t for x in vtx)
            if m < 8:  # texture coordinates (0,0) (1,0) (0,1): the record's u, v are the barycentrics
                out.append(f"obj {nid} triangle_uv {pts} 0 0.0 0.0 0.0 1.0 0.0 0.0 0.0 1.0 0.0")
            else:
                out.append(f"obj {nid} triangle {pts} 0")
            ids.append(nid)
            nid += 1
        out.append(f"obj {100000 + m} bvh 0.0 1.0 {len(ids)} " + " ".join(map(str, ids)))
        roots.append(100000 + m)
    out.append(f"obj 200000 list {len(roots)} " + " ".join(map(str, roots)))
    out += ["world 200000", "camera 0.0 0.0 -100.0 0.0 0.0 0.0 0.0 1.0 0.0 40.0 1.0 0.0 10.0 0.0 1.0",
            "obj 200001 xz_rect 0.0 1.0 0.0 1.0 500.0 -1", "obj 200002 list 1 200001", "lights 200002"]
    return "\n".join(out) + "\n"


def make_mesh_kat(n):
    """kat_mesh.scene, the reference's records over it, and its topology dumps."""
    with open(MESH_SCENE, "w") as f:
        f.write(mesh_scene_text())
    run("kat", "mesh", n, 1234567, os.path.join(HERE, "kat_mesh.bin"), MESH_SCENE)
    dumps = []
    for m in range(N_KAT_MESHES):
        tmp = os.path.join(HERE, f".bvh_kat_mesh_{m}.tmp")
        run("bvh", MESH_SCENE, 100000 + m, tmp)
        with open(tmp) as f:
            dumps.append(f"mesh {m}\n" + f.read())
        os.remove(tmp)
    with open(os.path.join(HERE, "bvh_kat_mesh.txt"), "w") as f:
        f.write("".join(dumps))


def only_kats(names):
    """Generate the named KATs alone and add their entries to golden.json."""
    sizes = dict(KATS)
    unknown = [k for k in names if k not in sizes or k in MERL_KATS]
    if unknown:
        sys.exit(f"--kats: cannot generate {unknown} alone")
    path = os.path.join(HERE, "golden.json")
    with open(path) as f:
        meta = json.load(f)
    for name in names:
        if name == "mesh":
            make_mesh_kat(sizes[name])
        else:
            run("kat", name, sizes[name], 1234567, os.path.join(HERE, f"kat_{name}.bin"))
        meta["kats"][name] = sizes[name]
    with open(path, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


def main():
    if not os.path.exists(HARNESS):
        sys.exit("build the reference harness first: make -C oracle ref")
    if len(sys.argv) > 1:
        if sys.argv[1] != "--kats" or len(sys.argv) < 3:
            sys.exit("usage: make_golden.py [--kats NAME ...]")
        return only_kats(sys.argv[2:])
    libm = host_libm()
    meta = {"renders": {}, "kats": {}, "merl_libm": MERL_LIBM_PIN}
    for name, fac, nx, ny, spp, md in RENDERS:
        txt = os.path.join(HERE, f"{name}.scene")
        with open(txt, "w") as f:
            f.write(fac().text())
        stats = json.loads(run("render", txt, nx, ny, spp, md, os.path.join(HERE, name)).strip().splitlines()[-1])
        os.remove(os.path.join(HERE, f"{name}.ppm"))
        meta["renders"][name] = dict(nx=nx, ny=ny, spp=spp, max_depth=md, world_rays=stats["world_rays"])
        print(name, stats)
    for name, n in KATS:
        if name in MERL_KATS and libm != MERL_LIBM_PIN:
            print(f"kat_{name}.bin NOT regenerated: this host's libm {libm} is not the pinned {MERL_LIBM_PIN}")
            meta["kats"][name] = n
            continue
        if name == "mesh":
            make_mesh_kat(n)
        else:
            run("kat", name, n, 1234567, os.path.join(HERE, f"kat_{name}.bin"))
        meta["kats"][name] = n
    run("teapot", 60.0, 10, os.path.join(HERE, "teapot_s60_d10.f32"))
    for n in (64, 1024, 4096):
        run("sobol", n, os.path.join(HERE, f"sobol_{n}.f64"))
    # reference BVH topology of S2's teapot (object 11 = bvh_group)
    run("bvh", os.path.join(HERE, "s2.scene"), 11, os.path.join(HERE, "bvh_s2_teapot.txt"))
    with open(os.path.join(HERE, "golden.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
