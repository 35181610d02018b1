"""Edge classes of the scene KAT records (tests/golden/kat_{sphere, moving_sphere,
rect, box, xform, medium, isotropic, texture_checker, texture_noise,
texture_image, mesh}.bin), worked out from the committed records alone: the inputs,
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
HIT = {"sphere": 12, "moving_sphere": 18, "rect": 15, "box": 14, "xform": 27, "medium": 18, "mesh": 10}
NEW_KATS = ("sphere", "moving_sphere", "rect", "box", "xform", "medium", "isotropic", "texture_checker",
            "texture_noise", "texture_image", "mesh")
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


_CLASSIFIERS = {"mesh": _mesh, "sphere": _sphere, "moving_sphere": _moving_sphere, "rect": _rect, "box": _box, "xform": _xform,
                "medium": _medium, "isotropic": _isotropic, "texture_checker": _texture_checker,
                "texture_noise": _texture_noise, "texture_image": _texture_image}


def classify(name, rec):
    return _CLASSIFIERS[name](np.asarray(rec, F))


def classes_of(name, rec, i):
    """The class names of record i (for a failure message); '' for other KATs."""
    if name not in _CLASSIFIERS:
        return ""
    return "; ".join(k for k, m in classify(name, rec).items() if m[i])
