"""Edge classes of the scene KAT records (tests/golden/kat_{sphere, moving_sphere,
rect, box, xform, medium, isotropic, texture_checker, texture_noise,
texture_image, mesh, world, bounce}.bin), worked out from the committed records alone: the inputs,
the reference's outputs and float32 arithmetic in numpy (the mesh KAT also reads its
committed scene text, kat_mesh.scene, and places lattice points in exact float64).
No device code and no restatement code is involved.  Layouts: tests/golden/README.md.

classify(name, rec) -> {class name: boolean mask over the records}; a record may
be in several classes.  HIT[name] is the column of the record's hit flag.
"""
import functools
import os

import numpy as np

F = np.float32
HIT = {"sphere": 12, "moving_sphere": 18, "rect": 15, "box": 14, "xform": 27, "medium": 18, "mesh": 10, "world": 11}
NEW_KATS = ("sphere", "moving_sphere", "rect", "box", "xform", "medium", "isotropic", "texture_checker",
            "texture_noise", "texture_image", "mesh", "world", "bounce")
MESH_SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_mesh.scene")


def _dot(a, b):  # vec3.h dot: ((x x' + y y') + z z') in float32
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _lcg_steps(rec, c_in, c_out, most=64):
    """How many LCG draws (mathf.h:14-19) lead from the state in columns c_in to
    the state in columns c_out (-1: more than `most`)."""
    s = rec[:, c_in].astype(np.uint64) | (rec[:, c_in + 1].astype(np.uint64) << np.uint64(24))
    want = rec[:, c_out].astype(np.uint64) | (rec[:, c_out + 1].astype(np.uint64) << np.uint64(24))
    k = np.full(len(rec), -1)
    k[s == want] = 0
    for i in range(1, most + 1):
        s = (np.uint64(0x5DEECE66D) * s + np.uint64(0xB16)) & np.uint64(0xFFFFFFFFFFFF)
        k[(k < 0) & (s == want)] = i
    return k


def _sphere(rec):
    c, r, o, d, tmin, tmax = rec[:, 0:3], rec[:, 3], rec[:, 4:7], rec[:, 7:10], rec[:, 10], rec[:, 11]
    hit, t, n = rec[:, 12] == 1, rec[:, 13], rec[:, 17:20]
    oc = o - c
    a, b = _dot(d, d), _dot(oc, d)
    cc = _dot(oc, oc) - r * r
    disc = b * b - a * cc
    sq = np.sqrt(np.where(disc > 0, disc, F(0)))
    r1, r2 = (-b - sq) / a, (-b + sq) / a
    pos = disc > 0
    length = np.sqrt(a.astype(np.float64))
    return {
        "first root": hit & (t == r1),
        "second root": hit & (t == r2) & (t != r1),
        "miss, disc == 0": ~hit & (disc == 0),
        "miss, disc < 0": ~hit & (disc < 0),
        "miss, disc > 0 (range)": ~hit & pos,
        "root == tmin": pos & ((r1 == tmin) | (r2 == tmin)),
        "root == tmax": pos & ((r1 == tmax) | (r2 == tmax)),
        "tmax between the roots": pos & (r1 < tmax) & (tmax < r2),
        "pole, |y/r| == 1": hit & (np.abs(n[:, 1]) == 1),
        "pole, |y/r| > 1": hit & (np.abs(n[:, 1]) > 1),
        "seam, z = +0": hit & (n[:, 2] == 0) & ~np.signbit(n[:, 2]) & (n[:, 0] < 0),
        "seam, z = -0": hit & (n[:, 2] == 0) & np.signbit(n[:, 2]) & (n[:, 0] < 0),
        "negative radius": hit & (r < 0),
        "|d| < 0.03": hit & (length < 0.03),
        "|d| > 30": hit & (length > 30),
    }


def _moving_sphere(rec):
    t0, t1, tm = rec[:, 6], rec[:, 7], rec[:, 15]
    hit = rec[:, 18] == 1
    return {
        "time == t0": tm == t0,
        "time == t1": tm == t1,
        "time < t0": tm < t0,
        "time > t1": tm > t1,
        "time inside": (tm > t0) & (tm < t1),
        "c0 == c1": (rec[:, 0:3] == rec[:, 3:6]).all(axis=1),
        "time == t0, hit": (tm == t0) & hit,
        "time == t1, hit": (tm == t1) & hit,
        "time outside, hit": ((tm < t0) | (tm > t1)) & hit,
    }


def _rect_planes(kax, a0, a1, lo0, hi0, lo1, hi1, k, o, d):
    """aarect.h:96-103 in float32: t and the in-plane point, per record."""
    idx = np.arange(len(o))
    with np.errstate(all="ignore"):
        t = (k - o[idx, kax]) / d[idx, kax]
        x = o[idx, a0] + t * d[idx, a0]
        y = o[idx, a1] + t * d[idx, a1]
    return t, x, y


def _rect(rec):
    kind = rec[:, 0].astype(int)
    kax = np.where(kind == 0, 2, np.where(kind == 1, 1, 0))
    a0 = np.where(kind == 2, 1, 0)
    a1 = np.where(kind == 0, 1, 2)
    lo0, hi0, lo1, hi1, k = (rec[:, i] for i in range(2, 7))
    tmin, tmax = rec[:, 13], rec[:, 14]
    hit = rec[:, 15] == 1
    t, x, y = _rect_planes(kax, a0, a1, lo0, hi0, lo1, hi1, k, rec[:, 7:10], rec[:, 10:13])
    fin = np.isfinite(t)
    edge = fin & ((x == lo0) | (x == hi0) | (y == lo1) | (y == hi1))
    degenerate = (lo0 == hi0) | (lo1 == hi1)
    special = (t == tmin) | (t == tmax) | edge | degenerate | ~fin
    out = {"flipped, hit": hit & (rec[:, 1] != 0), "not flipped, hit": hit & (rec[:, 1] == 0)}
    for kd, nm in enumerate(("xy", "xz", "yz")):
        m = kind == kd
        out[f"{nm}: t == tmin, hit"] = m & hit & (t == tmin)
        out[f"{nm}: t == tmax, hit"] = m & hit & (t == tmax)
        out[f"{nm}: on an edge, hit"] = m & hit & edge
        out[f"{nm}: t = +-inf, miss"] = m & ~hit & np.isinf(t)
        out[f"{nm}: t = NaN, hit"] = m & hit & np.isnan(t) & np.isnan(rec[:, 16])
        out[f"{nm}: lo == hi, hit, u or v NaN"] = m & hit & degenerate & (np.isnan(rec[:, 17]) | np.isnan(rec[:, 18]))
        out[f"{nm}: plain hit"] = m & hit & ~special
        out[f"{nm}: plain miss"] = m & ~hit & ~special
    return out


def _box(rec):
    p0, p1, o, d = rec[:, 0:3], rec[:, 3:6], rec[:, 6:9], rec[:, 9:12]
    hit, t = rec[:, 14] == 1, rec[:, 15]
    n = len(rec)
    same = np.zeros(n, int)
    nan_face = np.zeros(n, bool)
    for kax, a0, a1 in ((2, 0, 1), (1, 0, 2), (0, 1, 2)):  # box.h:22-27: the xy, xz, yz pairs
        for k in (p1[:, kax], p0[:, kax]):
            ax = np.full(n, kax)
            tf, x, y = _rect_planes(ax, np.full(n, a0), np.full(n, a1), p0[:, a0], p1[:, a0], p0[:, a1], p1[:, a1], k, o, d)
            inb = ~((x < p0[:, a0]) | (x > p1[:, a0]) | (y < p0[:, a1]) | (y > p1[:, a1]))
            same += (np.isfinite(tf) & inb & (tf == t)).astype(int)
            nan_face |= np.isnan(tf)
    inside = ((o > p0) & (o < p1)).all(axis=1)
    return {
        "origin outside, one face, hit": hit & ~inside & (same == 1) & ~nan_face,
        "origin inside, hit": hit & inside & ~nan_face,
        "origin inside, miss (tmax before the wall)": ~hit & inside,
        "through an edge (two faces at t)": hit & (same == 2) & ~nan_face,
        "through a corner (three faces at t)": hit & (same == 3) & ~nan_face,
        "in a face's plane (NaN t), hit": hit & nan_face,
        "miss": ~hit & ~inside & ~nan_face,
    }


def _xform(rec):
    kinds = rec[:, [7, 11, 15]].astype(int)
    ang = rec[:, [8, 12, 16]]
    hit = rec[:, 27] == 1
    rot = (kinds == 2) | (kinds == 3)
    out = {}
    for a in (0.0, 90.0, -90.0, 180.0, 360.0, 1e-4, 15.0, -18.0):
        out[f"angle {a:g}"] = (rot & (ang == F(a))).any(axis=1)
        out[f"angle {a:g}, hit"] = out[f"angle {a:g}"] & hit
    tr = kinds == 1
    lvl = np.arange(3)[None, :]
    first = lambda m: np.where(m.any(axis=1), np.where(m, lvl, 9).min(axis=1), 9)  # noqa: E731
    last = lambda m: np.where(m.any(axis=1), np.where(m, lvl, -1).max(axis=1), -1)  # noqa: E731
    flip = kinds == 4
    out.update({
        "zero offset": (tr & (rec[:, [8, 12, 16]] == 0) & (rec[:, [9, 13, 17]] == 0) & (rec[:, [10, 14, 18]] == 0)).any(axis=1),
        "translate outside a rotation": tr.any(axis=1) & rot.any(axis=1) & (first(tr) < last(rot)),
        "rotation outside a translate": tr.any(axis=1) & rot.any(axis=1) & (first(rot) < last(tr)),
        "flip outside a rotation, hit": hit & flip.any(axis=1) & rot.any(axis=1) & (first(flip) < last(rot)),
        "flip inside a rotation, hit": hit & flip.any(axis=1) & rot.any(axis=1) & (first(rot) < last(flip)),
        "rotate_y, hit": hit & (kinds == 2).any(axis=1),
        "rotate_x, hit": hit & (kinds == 3).any(axis=1),
        "three deep, hit": hit & (kinds != 0).all(axis=1),
        "around a sphere, hit": hit & (rec[:, 0] == 0),
        "around a box, hit": hit & (rec[:, 0] == 1),
        "miss": ~hit,
    })
    return out


def _medium(rec):
    bt = rec[:, 0]
    a, b, dens = rec[:, 1:4].astype(np.float64), rec[:, 4:7].astype(np.float64), rec[:, 7]
    o, d = rec[:, 8:11].astype(np.float64), rec[:, 11:14].astype(np.float64)
    tmin, tmax = rec[:, 14].astype(np.float64), rec[:, 15].astype(np.float64)
    hit = rec[:, 18] == 1
    draws = _lcg_steps(rec, 16, 20, most=4)
    # the line's entry and exit through the boundary, in double (a rough geometry, only to name the case)
    with np.errstate(all="ignore"):
        oc = o - a
        qa, qb = (d * d).sum(1), (oc * d).sum(1)
        disc = qb * qb - qa * ((oc * oc).sum(1) - b[:, 0] ** 2)
        sq = np.sqrt(np.maximum(disc, 0))
        es, xs = (-qb - sq) / qa, (-qb + sq) / qa
        t0, t1 = (a - o) / d, (b - o) / d
        eb, xb = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
    sphere = bt == 0
    e, x = np.where(sphere, es, eb), np.where(sphere, xs, xb)
    crossed = np.where(sphere, disc > 1e-9 * qb * qb, xb > eb)
    size = np.where(sphere, 2 * np.abs(b[:, 0]), np.sqrt(((b - a) ** 2).sum(1)))
    chord = (x - e) * np.sqrt(qa)
    return {
        "boundary missed, one draw": (draws == 1) & ~crossed & ~hit,
        "exit within 1e-4 of the entry, one draw": (draws == 1) & crossed & (x - e < 1e-4),
        "no overlap with [tmin, tmax], one draw": (draws == 1) & crossed & (x - e > 2e-4) & ((x <= tmin) | (e >= tmax)),
        "scattered": hit & (draws == 2),
        "passed through, two draws": ~hit & (draws == 2),
        "origin inside": crossed & (e < 0) & (x > 0) & (draws == 2),
        "tmax inside the medium": crossed & (e < tmax) & (tmax < x) & (draws == 2),
        "grazing": crossed & (chord < 0.3 * size) & (x - e > 2e-4) & (draws == 2),
        "sphere boundary, scattered": hit & sphere,
        "box boundary, scattered": hit & ~sphere,
        "density < 1e-3": (dens < 1e-3) & (draws == 2),
        "density >= 1": (dens >= 1) & (draws == 2),
    }


def _isotropic(rec):
    draws = _lcg_steps(rec, 3, 11, most=60)
    rej = np.where(draws > 0, draws // 3 - 1, -1)
    return {"no candidate rejected": rej == 0, "one rejected": rej == 1, "two rejected": rej == 2,
            "three or more rejected": rej >= 3, "draws in threes": (draws > 0) & (draws % 3 == 0)}


def _texture_checker(rec):
    p = rec[:, 1:4]
    x = (F(10) * p).astype(np.float64)
    k = np.rint(x / np.pi)
    near = (np.abs(x - k * np.pi) < 1e-5) & (k != 0)
    zero = p == 0
    clear = ~near.any(axis=1) & ~zero.any(axis=1)
    neg = (np.sin(x) < 0).sum(axis=1)
    first = (rec[:, 4:7] == np.array([0.2, 0.3, 0.1], F)).all(axis=1)
    return {
        "10 p at a multiple of pi": near.any(axis=1),
        "a component +0": (zero & ~np.signbit(p)).any(axis=1),
        "a component -0": (zero & np.signbit(p)).any(axis=1),
        "one negative sine": clear & (neg == 1),
        "two negative sines": clear & (neg == 2),
        "no or three negative sines": clear & ((neg == 0) | (neg == 3)),
        "checker of checkers": rec[:, 0] == 1,
        "checker of checkers, odd": (rec[:, 0] == 1) & ~first,
        "plain, even": (rec[:, 0] == 0) & first,
        "plain, odd": (rec[:, 0] == 0) & ~first,
    }


def _texture_noise(rec):
    with np.errstate(all="ignore"):
        v = rec[:, 0:1] * rec[:, 1:4]  # scale * p, float32
        top = np.abs(v.astype(np.float64)) * 64
        small = np.abs(v) < 2 ** 20
        whole = v == np.floor(v)
        below = small & ~whole & (np.ceil(v) - v < 1e-4 * np.maximum(1, np.abs(v)))
        above = small & ~whole & (v - np.floor(v) < 1e-4 * np.maximum(1, np.abs(v)))
    return {
        "on the lattice": (small & whole).all(axis=1),
        "just below the lattice": below.any(axis=1),
        "just above the lattice": above.any(axis=1),
        "negative p": (rec[:, 1:4] < 0).all(axis=1) & (top < 2 ** 24).all(axis=1),
        "seventh octave in [2^24, 2^31)": (top.max(axis=1) >= 2 ** 24) & (top.max(axis=1) < 2 ** 31),
        "FLAGGED: seventh octave >= 2^31": ((v.astype(np.float64) * 64) >= 2 ** 31).any(axis=1),
    }


def _texture_image(rec):
    u, v = rec[:, 0], rec[:, 1]
    nx, ny = 7, 5
    one = F(1)
    around = np.array([0.0, 1.0, np.nextafter(F(0), one), np.nextafter(F(0), -one), np.nextafter(one, F(0)),
                       np.nextafter(one, F(2))], F)
    with np.errstate(all="ignore"):
        j = (one - v).astype(np.float64) * ny - 0.001
        jr = np.rint(j)
        ux = (u * F(nx)).astype(np.float64)
        vy = ((one - v) * F(ny)).astype(np.float64)
        below, above = (j < jr) & (jr - j < 1e-5), (j >= jr) & (j - jr < 1e-5)
    return {
        "u at or an ulp from 0 or 1": np.isin(u, around),
        "v at or an ulp from 0 or 1": np.isin(v, around),
        "u or v = -0.3 or 1.7": np.isin(u, np.array([-0.3, 1.7], F)) | np.isin(v, np.array([-0.3, 1.7], F)),
        "(1-v) ny - 0.001 just below an integer": below,
        "(1-v) ny - 0.001 at or just above an integer": above,
        "u NaN": np.isnan(u),
        "v NaN": np.isnan(v),
        "FLAGGED: u nx >= 2^31": ux >= 2 ** 31,
        "FLAGGED: (1-v) ny >= 2^31": vy >= 2 ** 31,
    }


@functools.lru_cache(maxsize=None)
def mesh_scene():
    """The meshes of kat_mesh.scene: per `bvh` command, its triangles in the
    command's order, float32 [n][3 vertices][3]."""
    tri, meshes = {}, []
    with open(MESH_SCENE) as f:
        for line in f:
            w = line.split("#")[0].split()
            if len(w) > 2 and w[0] == "obj" and w[2] in ("triangle", "triangle_uv"):
                tri[int(w[1])] = np.array([float(x) for x in w[3:12]], F).reshape(3, 3)
            elif len(w) > 2 and w[0] == "obj" and w[2] == "bvh":
                meshes.append(np.stack([tri[int(k)] for k in w[6:6 + int(w[5])]]))
    return meshes


def _root_slab(lo, hi, o, d, tmin, tmax, shift=None):
    """aabb::hit (aabb.h:33-49) in float32 on the box [lo, hi], per record."""
    o = o.copy()
    if shift is not None:  # (axis, ulps): the origin moved by that many ulps on the axis
        a, k = shift
        for _ in range(abs(k)):
            o[:, a] = np.nextafter(o[:, a], F(np.inf if k > 0 else -np.inf))
    ok = np.ones(len(o), bool)
    tmin, tmax = tmin.copy(), tmax.copy()
    with np.errstate(all="ignore"):
        for a in range(3):
            inv = F(1) / d[:, a]
            t0, t1 = (lo[a] - o[:, a]) * inv, (hi[a] - o[:, a]) * inv
            sw = inv < 0
            t0, t1 = np.where(sw, t1, t0), np.where(sw, t0, t1)
            tmin = np.where(t0 > tmin, t0, tmin)
            tmax = np.where(t1 < tmax, t1, tmax)
            ok &= ~(tmax <= tmin)
    return ok, tmin


def _mesh_lines(rec):
    """Per record, against every triangle of its mesh, in float64 on the line o + t d
    (exact for the lattice meshes and lattice rays): Moller-Trumbore numerators with
    det > 0 -- nu, nv, det, the parameter t -- as lists of [records of mesh m][triangles]."""
    out = {}
    mesh = rec[:, 0].astype(int)
    for m, tris in enumerate(mesh_scene()):
        idx = np.flatnonzero(mesh == m)
        if not len(idx):
            continue
        T3 = tris.astype(np.float64)
        p0, e1, e2 = T3[:, 0], T3[:, 1] - T3[:, 0], T3[:, 2] - T3[:, 0]
        o, d = rec[idx, 1:4].astype(np.float64)[:, None, :], rec[idx, 4:7].astype(np.float64)[:, None, :]
        with np.errstate(all="ignore"):
            P = np.cross(d, e2[None])
            det = (e1[None] * P).sum(-1)
            sg = np.where(det < 0, -1.0, 1.0)
            Tv = o - p0[None]
            nu = (Tv * P).sum(-1) * sg
            Q = np.cross(Tv, e1[None])
            nv = (d * Q).sum(-1) * sg
            nt = (e2[None] * Q).sum(-1) * sg
            det = det * sg
            t = nt / det
            nrm = np.cross(e1, e2)
            sin = np.abs((d * nrm[None]).sum(-1)) / (np.linalg.norm(d, axis=-1) * np.linalg.norm(nrm, axis=-1)[None])
        out[m] = dict(idx=idx, nu=nu, nv=nv, det=det, t=t, sin=sin, facing=(d * nrm[None]).sum(-1))
    return out


def mesh_front_hit_sure(rec):
    """Records whose winning triangle (column tri) the line meets well inside
    (barycentrics 1e-4 from every edge, in float64): the front test of triangle::hit
    accepted it, so the record's p, n, u, v are the front test's."""
    sure = np.zeros(len(rec), bool)
    tri = rec[:, 12].astype(int)
    for m, L in _mesh_lines(rec).items():
        i = L["idx"]
        k = np.clip(tri[i], 0, L["nu"].shape[1] - 1)
        r = np.arange(len(i))
        with np.errstate(all="ignore"):
            u, v = L["nu"][r, k] / L["det"][r, k], L["nv"][r, k] / L["det"][r, k]
            sure[i] = (tri[i] >= 0) & (u > 1e-4) & (v > 1e-4) & (u + v < 1 - 1e-4)
    return sure


def _mesh(rec):
    n = len(rec)
    mesh, o, d, tmin, tmax = rec[:, 0].astype(int), rec[:, 1:4], rec[:, 4:7], rec[:, 7], rec[:, 8]
    med, hit, tri, p = rec[:, 9] != 0, rec[:, 10] == 1, rec[:, 12].astype(int), rec[:, 13:16]
    fin_d = np.isfinite(d).all(axis=1)
    z = lambda: np.zeros(n, bool)  # noqa: E731
    shared, apex, first_t, second_t, graze, back, retest = z(), z(), np.full(n, np.inf), np.full(n, np.inf), z(), z(), z()
    in_plane, root_miss, root_near, at_entry = z(), z(), z(), z()
    zero = (d == 0) & fin_d[:, None]
    sure = mesh_front_hit_sure(rec)
    for m, L in _mesh_lines(rec).items():
        i, nu, nv, det, t = L["idx"], L["nu"], L["nv"], L["det"], L["t"]
        with np.errstate(all="ignore"):
            closed = (det > 0) & (nu >= 0) & (nv >= 0) & (nu + nv <= det) & (t > 0)
            edge = closed & ((nu == 0) | (nv == 0) | (nu + nv == det))
            strict = (det > 0) & (nu > 0) & (nv > 0) & (nu + nv < det) & (t > 0)
        te = np.where(edge, t, np.inf)
        tie = (edge & (te == te.min(axis=1, keepdims=True))).sum(axis=1)
        if m != 6:  # (mesh 6 lists its triangles twice: a tie there is the duplicates' class)
            shared[i] = (tie >= 2) & (tie < 90)
        apex[i] = tie >= 90
        ts = np.sort(np.where(strict, t, np.inf), axis=1)
        first_t[i] = ts[:, 0]
        if ts.shape[1] > 1:
            second_t[i] = ts[:, 1]
        r = np.arange(len(i))
        k = np.clip(tri[i], 0, nu.shape[1] - 1)
        graze[i] = hit[i] & (L["sin"][r, k] < 1e-3)
        back[i] = med[i] & hit[i] & (L["facing"][r, k] > 0)
        retest[i] = med[i] & hit[i] & ~sure[i] & np.isfinite(rec[i, 11])
        tris = mesh_scene()[m]
        lo_t, hi_t = tris.min(axis=1), tris.max(axis=1)  # each triangle's box
        lo, hi = lo_t.min(axis=0), hi_t.max(axis=0)      # the root's
        for a in range(3):
            planes = np.unique(np.concatenate([lo_t[:, a], hi_t[:, a]]))
            in_plane[i] |= zero[i, a] & np.isin(o[i, a], planes)
        ok, entry = _root_slab(lo, hi, o[i], d[i], tmin[i], tmax[i])
        fin = fin_d[i] & ~np.isnan(tmax[i])
        root_miss[i] = fin & ~ok
        at_entry[i] = fin & (tmax[i] == entry) & (entry > tmin[i])
        near = np.zeros(len(i), bool)
        for a in range(3):
            for k2 in (-4, -3, -2, -1, 1, 2, 3, 4):
                near |= _root_slab(lo, hi, o[i], d[i], tmin[i], tmax[i], shift=(a, k2))[0]
        root_near[i] = fin & ~ok & near
    seen, on_surface = {}, z()
    for q in range(n):
        on_surface[q] = seen.get((mesh[q], o[q].tobytes()), False)
        if hit[q] and np.isfinite(p[q]).all():
            seen[(mesh[q], p[q].tobytes())] = True
    with np.errstate(all="ignore"):
        length = np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))
    big = F(np.finfo(np.float32).max)
    nan_bound = np.isnan(tmax)
    out = {
        "through a shared edge or vertex": shared,
        "through a shared edge or vertex, hit": shared & hit,
        "duplicated triangle, hit": (mesh == 6) & hit & (tri < 64),
        "the fan's apex: 96 triangles tie": apex & hit,
        "one component of d is +-0": zero.sum(axis=1) == 1,
        "two components of d are +-0": zero.sum(axis=1) == 2,
        "a component -0": (zero & np.signbit(d)).any(axis=1),
        "zero component with the origin in a box plane": in_plane,
        "zero component with the origin in a box plane, hit": in_plane & hit,
        "origin on an earlier hit point": on_surface,
        "origin on an earlier hit point, hit": on_surface & hit,
        "tmax before the first hit": np.isfinite(first_t) & (tmax > 0) & (tmax < first_t) & ~root_miss,
        "tmax between two hits": np.isfinite(second_t) & (tmax > first_t) & (tmax < second_t),
        "tmax at the root box's entry": at_entry,
        "tmin = -FLT_MAX, tmax = FLT_MAX": (tmin == -big) & (tmax == big),
        "tmin after an earlier hit": tmin > F(0.001),
        "NaN tmax": nan_bound,
        "NaN tmax, hit": nan_bound & hit,
        "NaN in d": ~fin_d,
        "medium ray arriving at a back face, hit": back,
        "medium ray, the front test not sure to have hit": retest,
        "|d| < 0.03, hit": hit & (length < 0.03),
        "|d| > 30, hit": hit & (length > 30),
        "grazing (within 1e-3 rad of the hit triangle's plane)": (mesh == 7) & graze,
        "root box missed": root_miss,
        "root box missed by at most 4 ulps of the origin": root_near,
    }
    for m in range(10):
        out[f"mesh {m}"] = mesh == m
        # (mesh 8's triangles are below triangle::hit's det threshold, and aabb::hit never enters mesh 5's
        # zero-thickness boxes unless a slab is NaN: neither is ever hit by a finite ray)
        if m not in (5, 8):
            out[f"mesh {m}, hit"] = (mesh == m) & hit
    return out


def mesh_nan_waves(rec):
    """Wave-aligned groups of 64 records that hold a NaN bound (tmax) without a
    finite one beside it (none expected)."""
    nanb = np.isnan(rec[:, 8])
    return [g for g in range(0, len(rec), 64) if nanb[g:g + 64].any() and nanb[g:g + 64].all()]


WORLD_SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_world.scene")
WORLD_T_ONLY_CAP = 0.08  # at most this share of the world KAT's records compares hit and t alone


@functools.lru_cache(maxsize=None)
def world_scene():
    """kat_world.scene: per world (obj 100000 + w) its top-level children as (kind,
    values) in list order, and every rect plane (axis, k) under it."""
    objs, worlds = {}, []
    with open(WORLD_SCENE) as f:
        for line in f:
            w = line.split("#")[0].split()
            if len(w) > 2 and w[0] == "obj":
                objs[int(w[1])] = w[2:]

    def rects(i, out):
        o = objs[i]
        if o[0] in ("xy_rect", "xz_rect", "yz_rect"):
            out.append(({"xy_rect": 2, "xz_rect": 1, "yz_rect": 0}[o[0]], float(o[5])))
        elif o[0] == "list":
            for k in o[2:2 + int(o[1])]:
                rects(int(k), out)
        elif o[0] == "bvh":
            for k in o[4:4 + int(o[3])]:
                rects(int(k), out)
        elif o[0] == "flip":
            rects(int(o[1]), out)
        return out

    def prims(i, out):  # the primitives under i that no wrapper moves: (kind, values); a box is kept whole
        o = objs[i]
        if o[0] == "list":
            for k in o[2:2 + int(o[1])]:
                prims(int(k), out)
        elif o[0] == "bvh":
            for k in o[4:4 + int(o[3])]:
                prims(int(k), out)
        elif o[0] in ("sphere", "moving_sphere", "xy_rect", "xz_rect", "yz_rect", "box", "triangle"):
            out.append((o[0], [float(x) for x in o[1:-1]]))
        return out

    w = 0
    while 100000 + w in objs:
        kids = [int(k) for k in objs[100000 + w][2:]]
        tops = [(objs[k][0], [float(x) for x in objs[k][1:-1]] if objs[k][0] in ("sphere", "moving_sphere") else None)
                for k in kids]
        worlds.append(dict(tops=tops, rect_planes=rects(100000 + w, []), prims=prims(100000 + w, []),
                           bvh_prims=[prims(k, []) for k in kids if objs[k][0] == "bvh"]))
        w += 1
    return worlds


def _prim_box(kind, v):
    """The reference's bounding_box(0, 1) of an unwrapped primitive, in float32 (sphere.h:31-34,
    moving_sphere.h:53-59, aarect.h:11-14, :41-44, :72-75, box.h:10-13, triangle.h:53-70)."""
    v = [F(x) for x in v]
    if kind == "sphere":
        c, r = np.array(v[:3], F), v[3]
        return c - r, c + r
    if kind == "moving_sphere":
        c0, c1, r = np.array(v[:3], F), np.array(v[3:6], F), v[8]
        return np.minimum(c0 - r, c1 - r), np.maximum(c0 + r, c1 + r)  # (t0 = 0, t1 = 1: the centers themselves)
    if kind == "box":
        return np.array(v[:3], F), np.array(v[3:6], F)
    if kind == "triangle":
        p = np.array(v[:9], F).reshape(3, 3)
        return p.min(axis=0), p.max(axis=0)
    ax, (a0, a1) = {"xy_rect": (2, (0, 1)), "xz_rect": (1, (0, 2)), "yz_rect": (0, (1, 2))}[kind]
    lo, hi = np.zeros(3, F), np.zeros(3, F)
    lo[a0], hi[a0], lo[a1], hi[a1] = v[0], v[1], v[2], v[3]
    lo[ax], hi[ax] = F(float(v[4]) - 0.0001), F(float(v[4]) + 0.0001)
    return lo, hi


def _line_hits(prims, o, d, time):
    """Parameters t at which the lines o + t d (float64, per record) meet the unwrapped
    primitives, [records][candidates] with inf where there is none: both roots of a sphere
    (a moving one at the record's time), a rect's or box face's plane crossing inside its
    bounds, a triangle's plane crossing inside it."""
    cols = []
    with np.errstate(all="ignore"):
        for kind, v in prims:
            if kind in ("sphere", "moving_sphere"):
                if kind == "sphere":
                    c, r = np.array(v[:3])[None, :], v[3]
                else:
                    c = np.array(v[:3]) + ((time[:, None] - v[6]) / (v[7] - v[6])) * (np.array(v[3:6]) - np.array(v[:3]))
                    r = v[8]
                oc = o - c
                a, b, cc = (d * d).sum(1), (oc * d).sum(1), (oc * oc).sum(1) - r * r
                disc = b * b - a * cc
                sq = np.sqrt(np.where(disc > 0, disc, 0))
                cols += [np.where(disc > 0, (-b - sq) / a, np.inf), np.where(disc > 0, (-b + sq) / a, np.inf)]
            elif kind == "triangle":
                p0, p1, p2 = np.array(v[0:3]), np.array(v[3:6]), np.array(v[6:9])
                e1, e2 = p1 - p0, p2 - p0
                P = np.cross(d, e2[None])
                det = (e1[None] * P).sum(1)
                T = o - p0
                u = (T * P).sum(1) / det
                Q = np.cross(T, e1[None])
                vv = (d * Q).sum(1) / det
                t = (e2[None] * Q).sum(1) / det
                cols.append(np.where((u > 0) & (vv > 0) & (u + vv < 1), t, np.inf))
            else:
                if kind == "box":
                    faces = [(ax, v[s * 3 + ax], [(a, v[a], v[3 + a]) for a in range(3) if a != ax])
                             for ax in range(3) for s in (0, 1)]
                else:
                    ax, (a0, a1) = {"xy_rect": (2, (0, 1)), "xz_rect": (1, (0, 2)), "yz_rect": (0, (1, 2))}[kind]
                    faces = [(ax, v[4], [(a0, v[0], v[1]), (a1, v[2], v[3])])]
                for ax, k, bounds in faces:
                    t = (k - o[:, ax]) / d[:, ax]
                    ok = np.isfinite(t)
                    for a, lo, hi in bounds:
                        x = o[:, a] + t * d[:, a]
                        ok &= (x > lo) & (x < hi)
                    cols.append(np.where(ok, t, np.inf))
    return np.stack(cols, axis=1)


def world_t_only(rec):
    """Records of the world KAT that compare hit and t alone: the is_medium ones (the
    boundary walk, list_hit, yields no more)."""
    return np.asarray(rec)[:, 10] != 0


def _sgroup_plane(c, r, hi):  # csrc/scene.cpp group_sphere_runs: the item box of a static sphere on one axis, as a float
    r = abs(r)
    lo, up = c - r, c + r
    w = 1e-5 * (max(abs(lo), abs(up)) + r) + 1e-30
    v = up + w if hi else lo - w
    f = F(v)
    if (float(f) < v) if hi else (float(f) > v):
        f = np.nextafter(f, F(np.inf if hi else -np.inf))
    return f


def _world(rec):
    n = len(rec)
    world, o, d, time, tmin, tmax = rec[:, 0].astype(int), rec[:, 1:4], rec[:, 4:7], rec[:, 7], rec[:, 8], rec[:, 9]
    med, hit, t, obj, p = rec[:, 10] != 0, rec[:, 11] == 1, rec[:, 12], rec[:, 13].astype(int), rec[:, 14:17]
    z = lambda: np.zeros(n, bool)  # noqa: E731
    big = F(np.finfo(np.float32).max)
    fin_d = np.isfinite(d).all(axis=1)
    zero = (d == 0) & fin_d[:, None]
    run_w, bvh_w = np.isin(world, (1, 2, 3)), world >= 4
    tang = {10: z(), 1000: z(), 100000: z()}
    tang_pos, tang_neg = {k: z() for k in tang}, {k: z() for k in tang}
    dup_ray, ulp_sides, mov_aim = z(), z(), z()
    tiny, inside, dup_hit, root_tmin, root_tmax, between, late, in_plane = z(), np.zeros(n, int), z(), z(), z(), z(), z(), z()
    rect_near, rect_between, mov_hit, rect_plane = z(), z(), z(), z()
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    for w, W in enumerate(world_scene()):
        idx = np.flatnonzero((world == w) & fin_d)
        for a, kk in W["rect_planes"]:
            rect_plane[idx] |= zero[idx, a] & (o[idx, a] == F(kk))
        if w not in (1, 2, 3) or not len(idx):
            continue
        sph = [(pos, kind, v) for pos, (kind, v) in enumerate(W["tops"]) if v is not None]
        first_pos = min(pos for pos, _, _ in sph)
        firsts = []  # per sphere: its first root above tmin and below tmax, float64
        for pos, kind, v in sph:
            if kind == "sphere":
                c, r = np.array(v[:3]), v[3]
                cc = np.broadcast_to(c, (len(idx), 3))
            else:
                c0, c1, t0, t1, r = np.array(v[:3]), np.array(v[3:6]), v[6], v[7], v[8]
                if t0 == t1:
                    continue
                cc = c0 + ((time[idx, None].astype(np.float64) - t0) / (t1 - t0)) * (c1 - c0)
            oc = o64[idx] - cc
            with np.errstate(all="ignore"):
                a_ = (d64[idx] ** 2).sum(1)
                b_ = (oc * d64[idx]).sum(1)
                c_ = (oc ** 2).sum(1) - r * r
                disc = b_ * b_ - a_ * c_
                sq = np.sqrt(np.where(disc > 0, disc, 0))
                r1, r2 = (-b_ - sq) / a_, (-b_ + sq) / a_
                impact = np.sqrt(np.maximum((oc ** 2).sum(1) - b_ * b_ / a_, 0))
                dist = np.sqrt((oc ** 2).sum(1))
                near = np.abs(impact - abs(r)) <= np.maximum(4e-7 * abs(r), 2.4e-7 * dist)  # a few ulps of r, or of the origin's coordinates
                for k in tang:
                    tang[k][idx] |= near & (dist > 0.3 * k) & (dist < 3 * k) & (abs(r) < 100)
                if r == 0.02:
                    tiny[idx] |= (impact < 0.03) & (dist >= 999)
                inside[idx] += (dist < abs(r)) & (abs(r) < 100)
                # float32 roots by sphere::hit's own arithmetic, for the equality classes (static spheres)
                if kind == "sphere":
                    ocf = o[idx] - c.astype(F)
                    af, bf = _dot(d[idx], d[idx]), _dot(ocf, d[idx])
                    cf = _dot(ocf, ocf) - F(r) * F(r)
                    df = bf * bf - af * cf
                    sf = np.sqrt(np.where(df > 0, df, F(0)))
                    f1, f2 = (-bf - sf) / af, (-bf + sf) / af
                    for k in tang:  # the float32 discriminant of sphere::hit on either side of 0
                        at_k = near & (dist > 0.3 * k) & (dist < 3 * k) & (abs(r) < 100)
                        tang_pos[k][idx] |= at_k & (df > 0)
                        tang_neg[k][idx] |= at_k & ~(df > 0)
                    for f in (f1, f2):
                        ulp_sides[idx] |= (df > 0) & (np.nextafter(f, F(0)) == tmin[idx]) & (np.nextafter(f, big) == tmax[idx])
                    root_tmin[idx] |= (df > 0) & ((f1 == tmin[idx]) | (f2 == tmin[idx]))
                    root_tmax[idx] |= (df > 0) & ((f1 == tmax[idx]) | (f2 == tmax[idx]))
                    for ax in range(3):
                        for hi in (False, True):
                            in_plane[idx] |= zero[idx, ax] & (o[idx, ax] == _sgroup_plane(v[ax], r, hi))
                ok = disc > 0
                v1 = np.where(ok & (r1 > tmin[idx]), r1, np.where(ok & (r2 > tmin[idx]), r2, np.inf))
            firsts.append((pos, kind, tuple(v), v1))
            if kind == "moving_sphere":
                mov_hit[idx] |= hit[idx] & (obj[idx] == pos)
                mov_aim[idx] |= np.isfinite(v1)
        V = np.stack([f[3] for f in firsts], axis=1)
        order = np.sort(V, axis=1)
        with np.errstate(all="ignore"):
            between[idx] = np.isfinite(order[:, 1]) & (tmax[idx] < big) & (order[:, 0] < tmax[idx]) & (tmax[idx] < order[:, 1])
        pos_of = np.array([f[0] for f in firsts])
        for j, (pos, kind, v, v1) in enumerate(firsts):
            # from the inputs alone: this sphere's first root is the nearest of the run's roots below tmax,
            # and a sphere earlier in the list has a farther one
            with np.errstate(all="ignore"):
                in_range = np.where(V < tmax[idx, None], V, np.inf)
                nearest = np.isfinite(in_range[:, j]) & (in_range[:, j] == in_range.min(axis=1))
                earlier_farther = (np.isfinite(in_range[:, :j]) & (in_range[:, :j] > in_range[:, j:j + 1])).any(axis=1)
            late[idx] |= nearest & earlier_farther
            twins = [i for i in range(len(firsts)) if i != j and firsts[i][1] == kind and firsts[i][2] == v]
            if twins:
                dup_ray[idx] |= np.isfinite(v1) & (v1 < tmax[idx])
                dup_hit[idx] |= np.isfinite(v1) & (v1 < tmax[idx]) & hit[idx] & np.isin(obj[idx], pos_of[[j] + twins])
        if w == 2:  # the xy_rect at z = 0 before the run: x in [-8, 8], y in [-3, 8]
            with np.errstate(all="ignore"):
                tr = -o64[idx, 2] / d64[idx, 2]
                px, py = o64[idx, 0] + tr * d64[idx, 0], o64[idx, 1] + tr * d64[idx, 1]
                on = (tr > 0.001) & (tr < tmax[idx]) & (px > -8) & (px < 8) & (py > -3) & (py < 8)
                below = (V < tr[:, None]).sum(1)
                some = np.isfinite(V).sum(1)
            rect_near[idx] = on & (below == 0) & (some > 0)
            rect_between[idx] = on & (below > 0) & (below < some)
        assert first_pos >= 0
    # object BVHs whose children no wrapper moves (world 4; world 5's triangles and duplicated spheres)
    W4, W5 = world_scene()[4], world_scene()[5]
    root_ulp, before_first, between_hits, back_tri, dup_child = z(), z(), z(), z(), z()
    i4 = np.flatnonzero((world == 4) & fin_d)
    for bp in W4["bvh_prims"]:  # the reference's root box of each of the four BVHs: the union of its children's
        boxes = [_prim_box(kind, v) for kind, v in bp]
        lo, hi = np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)
        for a in range(3):
            root_ulp[i4] |= zero[i4, a] & ((o[i4, a] == np.nextafter(lo[a], F(-np.inf))) | (o[i4, a] == np.nextafter(hi[a], F(np.inf))))
    ts = np.sort(_line_hits(W4["prims"], o64[i4], d64[i4], time[i4].astype(np.float64)), axis=1)
    ts = np.where(ts > 0.001, ts, np.inf)
    ts = np.sort(ts, axis=1)
    with np.errstate(all="ignore"):
        before_first[i4] = ~med[i4] & np.isfinite(ts[:, 0]) & (tmax[i4] > 0.001) & (tmax[i4] < ts[:, 0])
        between_hits[i4] = ~med[i4] & np.isfinite(ts[:, 1]) & (tmax[i4] > ts[:, 0]) & (tmax[i4] < ts[:, 1]) & (ts[:, 0] < ts[:, 1])
    for w, W in ((4, W4), (5, W5)):
        iw = np.flatnonzero((world == w) & fin_d & med)
        for kind, v in W["prims"]:
            if kind != "triangle":
                continue
            th = _line_hits([(kind, v)], o64[iw], d64[iw], time[iw].astype(np.float64))[:, 0]
            nrm = np.cross(np.array(v[3:6]) - np.array(v[0:3]), np.array(v[6:9]) - np.array(v[0:3]))
            back_tri[iw] |= np.isfinite(th) & (th > 0) & ((d64[iw] * nrm[None]).sum(1) > 0)
    i5 = np.flatnonzero((world == 5) & fin_d)
    twice = [pv for pv in W5["prims"] if pv[0] == "sphere" and sum(q == pv for q in W5["prims"]) == 2]
    if len(i5) and twice:
        th = _line_hits(twice, o64[i5], d64[i5], time[i5].astype(np.float64))
        dup_child[i5] = (np.isfinite(th) & (th > tmin[i5, None]) & (th < tmax[i5, None])).any(axis=1)
    seen, on_surface, along_n = {}, z(), z()
    for q in range(n):
        was = seen.get((world[q], o[q].tobytes()))
        on_surface[q] = was is not None
        if was is not None:  # d parallel to the normal of a hit recorded at this point
            for nn in was:
                c = np.cross(d64[q], nn)
                along_n[q] |= bool((c * c).sum() <= 1e-10 * (d64[q] ** 2).sum() * (nn ** 2).sum())
        if hit[q] and np.isfinite(p[q]).all():
            seen.setdefault((world[q], p[q].tobytes()), []).append(rec[q, 17:20].astype(np.float64))
    with np.errstate(all="ignore"):
        length = np.sqrt((d64 ** 2).sum(axis=1))
        edge_pt = o64 + 8 * d64  # the constructed box-edge rays meet the edge at t = 8
    lo5, hi5 = np.array([-5.0, -1.0, 2.0]), np.array([-3.0, 1.0, 4.0])
    with np.errstate(all="ignore"):
        on_bound = ((edge_pt == lo5) | (edge_pt == hi5)).sum(1)
        in_box = ((edge_pt >= lo5) & (edge_pt <= hi5)).all(1)
    nan_t = np.isnan(tmax)
    fin_t = ~nan_t & (tmax < big)
    dup5 = np.isin(obj, (38, 39, 42, 43))  # world 5's duplicated spheres: leaves 38, 39 and their copies 42, 43
    out = {f"sphere run: near-tangent from about {k}": m & run_w for k, m in tang.items()}
    out.update({f"sphere run: near-tangent from about {k}, float32 disc > 0": m & run_w for k, m in tang_pos.items()})
    out.update({f"sphere run: near-tangent from about {k}, float32 disc <= 0": m & run_w for k, m in tang_neg.items()})
    out.update({
        "sphere run: a 0.02-radius sphere from >= 1e3 away": tiny,
        "sphere run: a 0.02-radius sphere from >= 1e3 away, hit": tiny & hit,
        "sphere run: origin inside one sphere": run_w & (inside == 1),
        "sphere run: origin inside two spheres": run_w & (inside == 2),
        "sphere run: origin inside three or more spheres": run_w & (inside >= 3),
        "sphere run: the line meets a duplicated pair in range": dup_ray,
        "sphere run: a duplicated pair is hit": dup_hit,
        "sphere run: tmin and tmax an ulp to either side of a root": ulp_sides,
        "sphere run: one zero component, the origin in a node box's face plane": in_plane & run_w & (zero.sum(axis=1) == 1),
        "sphere run: two zero components, the origin in a node box's face plane": in_plane & run_w & (zero.sum(axis=1) == 2),
        "sphere run: |d| < 0.03": run_w & fin_d & (length < 0.03),
        "sphere run: |d| > 30": run_w & fin_d & (length > 30),
        "sphere run: the line meets a moving sphere at time 0": mov_aim & (time == 0),
        "sphere run: the line meets a moving sphere at time 1": mov_aim & (time == 1),
        "sphere run: the line meets a moving sphere inside the shutter": mov_aim & (time > 0) & (time < 1),
        "sphere run: a root == tmin": root_tmin,
        "sphere run: a root == tmax": root_tmax,
        "sphere run: tmax between two spheres' roots": between,
        "sphere run: the nearest sphere is later in the list than a farther one the line meets": late,
        "sphere run: the rect before the run is nearer than every root": rect_near,
        "sphere run: the rect before the run lies between two roots": rect_between,
        "sphere run: zero component with the origin in a node box's face plane": in_plane & run_w,
        "sphere run: NaN in d": run_w & ~fin_d,
        "sphere run: NaN tmax": run_w & nan_t,
        "sphere run: |d| < 0.03, hit": run_w & hit & (length < 0.03),
        "sphere run: |d| > 30, hit": run_w & hit & (length > 30),
        "sphere run: a moving sphere wins at time 0": mov_hit & (time == 0),
        "sphere run: a moving sphere wins at time 1": mov_hit & (time == 1),
        "sphere run: a moving sphere wins inside the shutter": mov_hit & (time > 0) & (time < 1),
        "object BVH: a duplicated child wins (equal t in two leaves)": (world == 5) & hit & ~med & dup5,
        "object BVH: through a box edge inside a leaf": (world == 5) & in_box & (on_bound == 2),
        "object BVH: the line meets a duplicated child in range": dup_child,
        "object BVH: root box missed by an ulp of the origin, that component of d zero": root_ulp,
        "object BVH: tmax before the first hit": before_first,
        "object BVH: tmax between the first two hits": between_hits,
        "object BVH: one zero component": bvh_w & (zero.sum(axis=1) == 1),
        "object BVH: two zero components": bvh_w & (zero.sum(axis=1) == 2),
        "object BVH: is_medium, the line meets a triangle child from behind": back_tri,
        "origin on an earlier hit point, d along its normal": on_surface & along_n,
        "origin on an earlier hit point, d not along its normal": on_surface & ~along_n,
        "object BVH: a zero component, miss": bvh_w & zero.any(axis=1) & ~hit,
        "object BVH: a zero component, hit": bvh_w & zero.any(axis=1) & hit,
        "object BVH: finite tmax, miss": bvh_w & fin_t & ~hit,
        "object BVH: finite tmax, hit": bvh_w & fin_t & hit,
        "object BVH: NaN tmax": bvh_w & nan_t,
        "object BVH: a ray in a rect's plane": bvh_w & rect_plane,
        "object BVH: is_medium, hit": bvh_w & med & hit,
        "object BVH: is_medium, tmin = -FLT_MAX": bvh_w & med & (tmin == -big),
        "origin on an earlier hit point": on_surface,
        "origin on an earlier hit point, hit": on_surface & hit,
        "time inside the shutter": (time > 0) & (time <= 1),
    })
    for w in range(7):
        out[f"world {w}"] = world == w
        out[f"world {w}, hit"] = (world == w) & hit
    return out


# The world KAT's classes are held to the number of records its generator constructs for them
# (oracle/ref/kat.inc kat_world_record: blocks of 32, a block split k ways gives 32 / k, rounded
# down; 64 origin-reuse records in two halves); every other class to test_kat_edges' 8.
# The sign of the float32 discriminant of a near-tangent ray is decided by rounding, not by
# construction: each sign must be present at each distance.
WORLD_MIN = {
    "sphere run: near-tangent from about 10": 10, "sphere run: near-tangent from about 1000": 10,
    "sphere run: near-tangent from about 100000": 10,
    **{f"sphere run: near-tangent from about {k}, float32 disc {sg} 0": 1 for k in (10, 1000, 100000) for sg in (">", "<=")},
    "sphere run: a 0.02-radius sphere from >= 1e3 away": 32,
    "sphere run: origin inside one sphere": 8, "sphere run: origin inside two spheres": 8,
    "sphere run: origin inside three or more spheres": 16,
    "sphere run: the line meets a duplicated pair in range": 32,
    "sphere run: a root == tmin": 8, "sphere run: a root == tmax": 8, "sphere run: tmax between two spheres' roots": 8,
    "sphere run: tmin and tmax an ulp to either side of a root": 8,
    "sphere run: the nearest sphere is later in the list than a farther one the line meets": 32,
    "sphere run: the rect before the run is nearer than every root": 16,
    "sphere run: the rect before the run lies between two roots": 16,
    "sphere run: zero component with the origin in a node box's face plane": 32,
    "sphere run: one zero component, the origin in a node box's face plane": 18,
    "sphere run: two zero components, the origin in a node box's face plane": 14,
    "sphere run: NaN in d": 16, "sphere run: NaN tmax": 16,
    "sphere run: |d| < 0.03": 10, "sphere run: |d| > 30": 8,
    "sphere run: the line meets a moving sphere at time 0": 8, "sphere run: the line meets a moving sphere at time 1": 16,
    "sphere run: the line meets a moving sphere inside the shutter": 8,
    "object BVH: the line meets a duplicated child in range": 16, "object BVH: through a box edge inside a leaf": 16,
    "object BVH: root box missed by an ulp of the origin, that component of d zero": 32,
    "object BVH: tmax before the first hit": 16, "object BVH: tmax between the first two hits": 16,
    "object BVH: one zero component": 8, "object BVH: two zero components": 8, "object BVH: NaN tmax": 8,
    "object BVH: a ray in a rect's plane": 8,
    "object BVH: is_medium, the line meets a triangle child from behind": 32,
    "object BVH: is_medium, tmin = -FLT_MAX": 16,
    "origin on an earlier hit point": 64,
    "origin on an earlier hit point, d along its normal": 32, "origin on an earlier hit point, d not along its normal": 32,
}
BOUNCE_SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_bounce.scene")
# the function whose inputs a class stresses, for a failure message (csrc/kernels.hip)
BOUNCE_FAMILIES = ("terminal", "diffuse", "Beckmann", "specular")
# every record with a mixture loop must be walked (tests/test_kat_edges.py): this class stays empty
BOUNCE_WALK_MISSES = "mixture loop: the LCG walk does NOT reach the state after in the reference's attempts"


@functools.lru_cache(maxsize=None)
def bounce_scene():
    """kat_bounce.scene: ({list l: [(kind, floats) per member, flips followed]}, {mat m: (kind, floats)})."""
    objs, mats = {}, {}
    for line in open(BOUNCE_SCENE):
        t = line.split("#")[0].split()
        if len(t) > 2 and t[0] == "obj":
            objs[int(t[1])] = t[2:]
        if len(t) > 2 and t[0] == "mat":
            mats[int(t[1])] = (t[2], [float(x) for x in t[3:]])
    lists = {}
    for oid, t in objs.items():
        if oid >= 200000 and oid < 300000 and t[0] == "list":
            mem = []
            for k in t[2:2 + int(t[1])]:
                m = objs[int(k)]
                while m[0] == "flip":
                    m = objs[int(m[1])]
                mem.append((m[0], [float(x) for x in m[1:-1]]))
            lists[oid - 200000] = mem
    return lists, mats


def _bounce_light_points(kind, f):
    """bsdf_dead()'s test points of a sampling light, its radius and the coordinate scale of its margin."""
    if kind == "xz_rect":
        x0, x1, z0, z1, k = f
        return np.array([[x, k, z] for x in (x0, x1) for z in (z0, z1)]), 0.0, max(abs(v) for v in f)
    if kind == "sphere":
        return np.array([f[:3]]), abs(f[3]), max(abs(v) for v in f[:3]) + abs(f[3])
    if kind == "triangle":
        return np.array(f[:9]).reshape(3, 3), 0.0, max(abs(v) for v in f[:9])
    return None


def bounce_lcg_walk(rec, i):
    """The mixture loop of diffuse or Beckmann record i replayed on the LCG alone (mathf.h:14-19,
    pdf.h:175-189, hitable_list.h:63-67): (attempts, the last attempt's branch 'light' / 'bsdf',
    the member index of its light or -1), or None when the walk does not reach the state after
    within 5000 attempts.  A light attempt draws the index and two more if the member samples
    (xz_rect, sphere, triangle); a cosine / Oren-Nayar BSDF attempt draws two, a Beckmann one none."""
    lists, _ = bounce_scene()
    mem = lists[int(rec[i, 0])]
    beck = 6 <= rec[i, 1] <= 8
    step = lambda s: (0x5DEECE66D * s + 0xB16) & 0xFFFFFFFFFFFF  # noqa: E731
    s = int(rec[i, 19]) | (int(rec[i, 20]) << 24)
    want = int(rec[i, 37]) | (int(rec[i, 38]) << 24)
    s = step(s)
    for a in range(1, 5001):
        s = step(s)
        which, idx = "bsdf", -1
        if (s >> 16) / 4294967296.0 < 0.5:
            s = step(s)
            which, idx = "light", int((s >> 16) / 4294967296.0 * len(mem))
            if mem[idx][0] in ("xz_rect", "sphere", "triangle"):
                s = step(step(s))
        elif not beck:
            s = step(step(s))
        if s == want and a == int(rec[i, 36]):
            return a, which, idx
    return None


def _bounce(rec):
    lists, mats = bounce_scene()
    n_rec = len(rec)
    l, m = rec[:, 0].astype(int), rec[:, 1].astype(int)
    p, n, d = rec[:, 2:5].astype(np.float64), rec[:, 5:8].astype(np.float64), rec[:, 13:16].astype(np.float64)
    time, depth, max_depth = rec[:, 16], rec[:, 17], rec[:, 18]
    scattered, stime, col, att = rec[:, 25] == 1, rec[:, 32], rec[:, 33:36], rec[:, 36]
    kind = np.array([mats[x][0] for x in m])
    limit = depth >= max_depth
    lamb, oren, beck = kind == "lambertian", kind == "orennayar", kind == "beckmann"
    light = kind == "diffuse_light"
    term = limit | light
    diff, bk = (lamb | oren) & ~term, beck & ~term
    spec = ~term & ~diff & ~bk
    n_lights = np.array([len(lists[x]) for x in l])
    sampling = np.array([sum(k in ("xz_rect", "sphere", "triangle") for k, _ in lists[x]) for x in l])
    dn = (rec[:, 13] * rec[:, 5] + rec[:, 14] * rec[:, 6]) + rec[:, 15] * rec[:, 7]  # dot(d, n) in float32
    front = dn < 0
    dlen = np.sqrt((d * d).sum(axis=1))
    w = n / np.sqrt((n * n).sum(axis=1))[:, None]
    # the nearest light point beyond the tangent plane in margins of bsdf_dead (kernels.hip), per light kind
    ratio = {k: np.full(n_rec, np.inf) for k in ("xz_rect", "sphere", "triangle")}
    straddle, in_plane, inside, centre, edge_on = (np.zeros(n_rec, bool) for _ in range(5))
    for i in range(n_rec):
        ps = np.abs(p[i]).max() + 1.0
        for k, f in lists[l[i]]:
            lp = _bounce_light_points(k, f)
            if lp is None:
                continue
            pts, r, scale = lp
            s = (pts - p[i]) @ w[i] * (1.0 if front[i] else -1.0)  # the side the BSDF samples do not take is positive
            ratio[k][i] = min(ratio[k][i], (s.min() - r) / (1e-3 * (ps + scale)))
            straddle[i] |= (s.min() - r < 0) and (s.max() + r > 0)
            if k == "xz_rect":
                in_plane[i] |= rec[i, 3] == np.float32(f[4])
            if k == "sphere":
                dist = np.sqrt(((pts[0] - p[i]) ** 2).sum())
                inside[i] |= 0 < dist < r
                centre[i] |= dist == 0
            if k == "triangle":
                nn = np.cross(pts[1] - pts[0], pts[2] - pts[0])
                to = pts.mean(axis=0) - p[i]
                edge_on[i] |= abs(nn @ to) / np.sqrt(to @ to) < 1e-4  # triangle::hit's determinant towards the centroid
    near = np.minimum(np.minimum(ratio["xz_rect"], ratio["sphere"]), ratio["triangle"])
    dl = diff & (n_lights > 0)
    out = {f"family: {f}": x for f, x in zip(BOUNCE_FAMILIES, (term, diff, bk, spec))}
    names = {"xz_rect": "a rect light's corner", "sphere": "a sphere light's pole", "triangle": "a triangle light's vertex"}
    for k, nm in names.items():
        mine = dl & (ratio[k] == near)
        out[f"bsdf_dead: tangent plane within 12 margins of {nm}"] = mine & (np.abs(near) <= 12)
        out[f"bsdf_dead: {nm} inside the margin"] = mine & (near > 0) & (near < 1)
        out[f"bsdf_dead: {nm} 1 to 2.5 margins beyond the plane"] = mine & (near >= 1) & (near <= 2.5)
        out[f"bsdf_dead: {nm} 2.5 to 12 margins beyond the plane"] = mine & (near > 2.5) & (near <= 12)
        out[f"bsdf_dead: {nm} on the samples' side by up to 12 margins"] = mine & (near <= 0) & (near >= -12)
    loops = (dl | (bk & (n_lights > 0))) & scattered  # the records with a mixture loop
    walk = {i: bounce_lcg_walk(rec, i) for i in np.flatnonzero(loops)}
    last_bsdf = np.zeros(n_rec, bool)
    last_none = np.zeros(n_rec, bool)
    walked = np.zeros(n_rec, bool)
    for i, wk in walk.items():
        walked[i] = wk is not None
        if wk:
            last_bsdf[i] = wk[1] == "bsdf"
            last_none[i] = wk[1] == "light" and lists[l[i]][wk[2]][0] not in ("xz_rect", "sphere", "triangle")
    nx = np.abs(rec[:, 5])
    p9 = np.float32(0.9)
    axis = (np.abs(rec[:, 5:8]) == 1).sum(axis=1) == 1
    axis &= (rec[:, 5:8] == 0).sum(axis=1) == 2
    perp = (dn == 0) & axis
    # refract's discriminant (material.h:21-32) in float32, for dielectric records
    diel = (kind == "dielectric") & ~term
    ri = np.array([mats[x][1][0] if mats[x][0] == "dielectric" else 1.0 for x in m], F)
    with np.errstate(all="ignore"):
        d32 = rec[:, 13:16]
        ln = np.sqrt((d32[:, 0] * d32[:, 0] + d32[:, 1] * d32[:, 1]) + d32[:, 2] * d32[:, 2])
        uv = d32 / ln[:, None]
        inside_d = dn > 0
        outward = np.where(inside_d[:, None], -rec[:, 5:8], rec[:, 5:8])
        dt = _dot(uv, outward)
        nint = np.where(inside_d, ri, (1.0 / ri.astype(np.float64)).astype(F))
        disc = (1.0 - (nint * nint * (F(1) - dt * dt)).astype(np.float64)).astype(F)
        cos_in = np.abs(dn.astype(np.float64)) / (dlen * np.sqrt((n * n).sum(axis=1)))
        sn = (rec[:, 29] * rec[:, 5] + rec[:, 30] * rec[:, 6]) + rec[:, 31] * rec[:, 7]  # dot(scattered dir, n)
    ulp1 = F(2.0 ** -24)
    metal = (kind == "metal") & ~term
    fuzz = np.array([mats[x][1][3] if mats[x][0] == "metal" else 0.0 for x in m])
    checker_p = (np.sin(10 * rec[:, 2].astype(np.float64)) * np.sin(10 * rec[:, 3].astype(np.float64)) *
                 np.sin(10 * rec[:, 4].astype(np.float64)))
    out.update({
        "bsdf_dead: a light straddles the tangent plane": dl & straddle,
        "bsdf_dead: the hit point in an xz_rect light's plane, another sampling light in the list": dl & in_plane & (sampling > 1),
        "sphere light: the hit point inside it": dl & inside,
        "sphere light: the hit point at its centre": dl & centre,
        "triangle light: edge-on, within triangle::hit's determinant threshold": dl & edge_on,
        "mixture loop: exactly 1 attempt": dl & (att == 1),
        "mixture loop: 2 to 8 attempts": dl & (att >= 2) & (att <= 8),
        "mixture loop: 9 to 32 attempts": dl & (att >= 9) & (att <= 32),
        "mixture loop: 33 to 64 attempts": dl & (att >= 33) & (att <= 64),
        "mixture loop: more than 64 attempts": dl & (att > 64),
        "mixture loop: the LCG walk reaches the state after in the reference's attempts": walked,
        BOUNCE_WALK_MISSES: loops & ~walked,
        "mixture loop: a BSDF-branch attempt of a front-face diffuse hit succeeds (a light's pdf)": dl & front & last_bsdf,
        "mixture loop: a BSDF-branch attempt of a back-face Oren-Nayar hit succeeds": dl & oren & ~front & last_bsdf,
        "mixture loop: a non-sampling member's (1, 0, 0) succeeds": last_none,
        "skip_attempt: a list with non-sampling members, 2 or more attempts": dl & (sampling < n_lights) & (att >= 2),
        "light list 3 (a non-sampling member first), diffuse": dl & (l == 3),
        "light list 4 (non-sampling members only), back-face Oren-Nayar or Beckmann": (l == 4) & (oren | beck) & ~front & ~term,
        "light list 5 (empty), diffuse": diff & (l == 5),
        "light list 5 (empty), Beckmann": bk & (l == 5),
        "light list 6 (rects above and below), diffuse": dl & (l == 6),
        "light list 7 (five lights), diffuse": dl & (l == 7),
        "light list 8 (seven non-sampling members), diffuse": dl & (l == 8),
        "co == +0 (d perpendicular to an axis-aligned normal), lambertian": perp & ~np.signbit(dn) & lamb & ~term,
        "co == -0 (d perpendicular to an axis-aligned normal), lambertian": perp & np.signbit(dn) & lamb & ~term,
        "d perpendicular to the normal, not lambertian": perp & ~lamb & ~term,
        **{f"{nm}, front face": x & front for nm, x in (("lambertian", lamb & ~term), ("Oren-Nayar", oren & ~term), ("Beckmann", bk))},
        **{f"{nm}, back face": x & (dn > 0) for nm, x in (("lambertian", lamb & ~term), ("Oren-Nayar", oren & ~term), ("Beckmann", bk))},
        "onb_from_w: |n.x| == 0.9f": ~term & ~spec & (nx == p9),
        "onb_from_w: |n.x| an ulp below 0.9f": ~term & ~spec & (nx == np.nextafter(p9, F(0))),
        "onb_from_w: |n.x| an ulp above 0.9f": ~term & ~spec & (nx == np.nextafter(p9, F(1))),
        **{f"normal along {'-+'[sg > 0]}{'xyz'[a]}": ~term & axis & (rec[:, 5 + a] == sg) for a in range(3) for sg in (-1, 1)},
        "|d| < 0.1": ~term & (dlen < 0.1),
        "|d| > 100": ~term & (dlen > 100),
        "|d| > 100, diffuse": dl & (dlen > 100),
        "dielectric: normal incidence": diel & (cos_in > 0.999999),
        "dielectric: total reflection": diel & (disc <= 0) & (ri > 1),
        # (ulps of the discriminant's subtrahend ni^2 (1 - dt^2), a float just below 1: 2^-24)
        "dielectric: discriminant within 4 ulps above 0": diel & (disc > 0) & (disc <= 4 * ulp1) & (ri > 1),
        "dielectric: discriminant within 4 ulps at or below 0": diel & (disc <= 0) & (disc >= -4 * ulp1) & (ri > 1),
        "dielectric: from inside": diel & (dn > 0),
        "dielectric: from outside": diel & (dn < 0),
        "dielectric: index 1.0": diel & (ri == 1),
        "dielectric: index 1.0, grazing (discriminant 0)": diel & (ri == 1) & (disc == 0),
        "metal: fuzz 0": metal & (fuzz == 0),
        "metal: fuzz above 1": metal & (fuzz > 1),
        "metal: the reflected ray ends below the surface": metal & front & (sn < 0),
        "isotropic, checker albedo, sines < 0": (kind == "isotropic") & ~term & (checker_p < 0),
        "isotropic, checker albedo, sines >= 0": (kind == "isotropic") & ~term & (checker_p >= 0),
        "diffuse_light from the front": light & front,
        "diffuse_light from the back": light & (dn > 0),
        "depth == maxDepth on a scattering material": limit & ~light,
        "time == 0, diffuse": dl & (time == 0),
        "time == 1, diffuse": dl & (time == 1),
        "time inside the shutter, diffuse": dl & (time > 0) & (time < 1),
        "time != 0, specular (the new ray's time is 0)": spec & (time != 0) & (stime == 0),
        "NaN in the colour": np.isnan(col).any(axis=1),
    })
    return out


def bounce_waves_mixed(rec):
    """The first record of a group of 64 consecutive records that lacks one of the four families (-1: none)."""
    c = _bounce(np.asarray(rec, F))
    fam = np.stack([c[f"family: {f}"] for f in BOUNCE_FAMILIES])
    for i in range(0, len(rec) - 63):
        if not fam[:, i:i + 64].any(axis=1).all():
            return i
    return -1


# The bounce KAT's classes are held to test_kat_edges' 8; the two long loops to the 4 that the issue sets for them.
BOUNCE_MIN = {"mixture loop: 33 to 64 attempts": 4, "mixture loop: more than 64 attempts": 4, BOUNCE_WALK_MISSES: 0}
MIN_COUNTS = {"world": WORLD_MIN, "bounce": BOUNCE_MIN}
MAX_RECORDS = {"bounce": 2048}  # (every other KAT: test_kat_edges' 1024)

_CLASSIFIERS = {"bounce": _bounce, "world": _world, "mesh": _mesh, "sphere": _sphere, "moving_sphere": _moving_sphere, "rect": _rect, "box": _box, "xform": _xform,
                "medium": _medium, "isotropic": _isotropic, "texture_checker": _texture_checker,
                "texture_noise": _texture_noise, "texture_image": _texture_image}


def classify(name, rec):
    return _CLASSIFIERS[name](np.asarray(rec, F))


def classes_of(name, rec, i):
    """The class names of record i (for a failure message); '' for other KATs."""
    if name not in _CLASSIFIERS:
        return ""
    return "; ".join(k for k, m in classify(name, rec).items() if m[i])
