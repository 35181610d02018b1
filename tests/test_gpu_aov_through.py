"""First-diffuse-hit AOVs on the GPU (srr_render_aov_through).

Albedo and stats: bit-exact against the CPU oracle's image of the scene's SPECULAR TWIN:
metal and dielectric stay, every other material becomes a diffuse_light of its albedo.
The specular bounces of the twin draw what they draw in the beauty frame, an emitter never
scatters, and color() folds the attenuations back to front, so the oracle's image of the
twin (same max_depth) IS the mean through-specular albedo, its per-path ray counts sum to
world_rays and (rays > 1) counts the chained paths.  A diffuse_light emits to its front
only while the defined albedo does not depend on the face, so only pixels all of whose
twin paths are lit are compared (as test_gpu_aov.test_albedo_of_a_textured_scene_in_batches).

Normal and depth: against a float64 numpy restatement of a closed room of rects whose back
wall is a fuzz-0 mirror, reflected analytically."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_bind as ob
import test_gpu_aov as first_hit
from srr import capi, scenes
from srr.scene import Scene

NX = NY = 24
SPP = 4
EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "simple-raytracing-render_amd", "render_main")
_bits = first_hit._bits


def specular_twin(text: str) -> str:
    """`mat` lines of metal and dielectric stay; every other one -> diffuse_light of its albedo."""
    out = []
    for line in text.split("\n"):
        t = line.split()
        if t[:1] == ["mat"] and t[2] not in ("metal", "dielectric"):
            line = f"mat {t[1]} diffuse_light {t[3]}"
        out.append(line)
    return "\n".join(out)


def box_text(fuzz=0.0, tint=(1.0, 1.0, 1.0)):
    """Scenes (a) and (b): a closed Cornell box seen from inside (every wall faces the camera, so
    the twin shows every terminal hit), its back wall and a floor plate metal(tint, fuzz) -- two
    mirrors at right angles give chains of two and more metal bounces --, a glass sphere, and a
    glass box, whose flat faces reflect totally from inside."""
    s = Scene()
    red = s.lambertian(s.constant_texture(scenes.RED))
    white = s.lambertian(s.constant_texture(scenes.WHITE))
    green = s.lambertian(s.constant_texture(scenes.GREEN))
    light = s.diffuse_light(s.constant_texture(15.0))
    mirror = s.metal(tint, fuzz)
    glass = s.dielectric(1.5)
    s.set_world(s.hitable_list([
        s.flip_normals(s.yz_rect(0, 555, 0, 555, 555, green)), s.yz_rect(0, 555, 0, 555, 0, red),
        s.flip_normals(s.xz_rect(0, 555, 0, 555, 555, white)), s.xz_rect(0, 555, 0, 555, 0, white),
        s.flip_normals(s.xy_rect(0, 555, 0, 555, 555, mirror)), s.xy_rect(0, 555, 0, 555, 0, white),
        s.flip_normals(s.xz_rect(213, 343, 227, 332, 554, light)),
        s.xz_rect(100, 455, 300, 540, 1, mirror),
        s.sphere((170, 120, 300), 90, glass),
        s.box((330, 40, 250), (450, 200, 370), glass)]))
    s.camera((278, 278, 20), (278, 200, 555), (0, 1, 0), 70.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    s.set_lights(s.hitable_list([s.flip_normals(s.xz_rect(213, 343, 227, 332, 554))]))
    return s.text()


def s3_metal_text():
    """Scene (c): the world of scenes.s3_cornell_teapot_microfacet("metal") -- the Cornell box, a
    metal(0.9, 0) teapot mesh, a glass sphere -- from its own parts.  The project's camera stands
    outside the open front, through which the teapot's reflections leave and 22 % of the pixels
    hold an unlit path; here a front wall closes the box and the camera stands inside."""
    s = Scene()
    objs, white = scenes._cornell(s, sphere_mat=s.dielectric(1.5))
    objs.append(scenes._teapot_instance(s, s.metal(0.9, 0.0), 10))
    objs.append(s.xy_rect(0, 555, 0, 555, 0, white))
    s.set_world(s.hitable_list(objs))
    s.camera((278, 278, 10), (278, 200, 555), (0, 1, 0), 70.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    s.set_lights(s.hitable_list([s.flip_normals(s.xz_rect(213, 343, 227, 332, 554))]))
    return s.text()


SCENES = {"a": lambda: box_text(), "b": lambda: box_text(0.3, (0.9, 0.6, 0.3)), "c": s3_metal_text}
# ... and the project's S3-metal scene itself, compared where its twin is lit (no 10 % condition:
# its camera looks through the open front, through which reflections leave)
PROJECT_SCENES = {"s3_metal": lambda: scenes.s3_cornell_teapot_microfacet("metal")[0].text()}
_cache = {}


def twin_of(name, max_depth=50):
    """(scene text, the oracle's render of its specular twin), computed once and read-only."""
    key = (name, max_depth)
    if key not in _cache:
        text = (SCENES.get(name) or PROJECT_SCENES[name])()
        twin = ob.render(specular_twin(text), NX, NY, SPP, max_depth)
        for a in twin.values():
            a.setflags(write=False)
        _cache[key] = (text, twin)
    return _cache[key]


def lit_pixels(twin):
    return (twin["paths"] != 0).any(axis=2).all(axis=1)


# ------------------------------------------------------------ CPU: the oracle alone
@pytest.mark.parametrize("name", sorted(SCENES))
def test_specular_twin_leaves_out_few_pixels(name):
    _, twin = twin_of(name)
    lit = lit_pixels(twin)
    print(f"scene {name}: {100 * (1 - lit.mean()):.2f} % of the pixels left out, "
          f"{(twin['rays'] > 1).mean():.3f} of the paths chained, longest {twin['rays'].max() - 1}")
    assert lit.mean() >= 0.9
    assert (twin["rays"] > 2).any()  # chains of two and more


def test_specular_twin_without_specular_materials_is_the_emissive_twin():
    text = scenes.s1_cornell()[0].text()
    assert specular_twin(text) == first_hit.emissive_twin(text)
    assert specular_twin(SCENES["a"]()) != first_hit.emissive_twin(SCENES["a"]())


# ------------------------------------------------------------ GPU
def _render(text, max_depth=50, **kw):
    return capi.Renderer(text).render_aov(NX, NY, SPP, max_depth=max_depth, through_specular=True, **kw)


def _check_against_twin(got, twin, lit, max_depth):
    st = got["stats"]
    np.testing.assert_array_equal(_bits(got["albedo"][lit]), _bits(twin["img"][lit]))
    assert st["paths"] == NX * NY * SPP
    assert st["world_rays"] == int(twin["rays"].sum()) == int(twin["stats"][0])
    assert st["chained_paths"] == int((twin["rays"] > 1).sum())
    assert st["longest_chain"] == int(twin["rays"].max()) - 1 <= max_depth


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES) + sorted(PROJECT_SCENES))
def test_albedo_and_stats_are_the_oracles_specular_twin(name):
    text, twin = twin_of(name)
    lit = lit_pixels(twin)
    assert lit.mean() > 0.5
    got = _render(text)
    _check_against_twin(got, twin, lit, 50)
    first = capi.Renderer(text).render_aov(NX, NY, SPP)
    assert (_bits(got["albedo"][lit]) != _bits(first["albedo"][lit])).any()  # and they are other guides


def _front_to_back(text, name):
    """Scene (b)'s mean albedo with every path's product taken front to back, ((a_0 a_1) ...) e,
    from the oracle: all its metal has one colour c, so a path of m metal bounces is c^m e.  The
    twin with c = (2, 2, 2) gives 2^m e exactly, hence m and e per path."""
    c = np.float32([0.9, 0.6, 0.3])
    _, twin = twin_of(name)
    two = ob.render(specular_twin(box_text(0.3, (2.0, 2.0, 2.0))), NX, NY, SPP, 50)["paths"]
    one = ob.render(specular_twin(box_text(0.3, (1.0, 1.0, 1.0))), NX, NY, SPP, 50)["paths"]
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(one.max(axis=2) > 0, np.log2(two.max(axis=2) / one.max(axis=2)), 0.0)
    assert (m == np.round(m)).all()
    m = m.astype(np.int64)
    back, front = one.copy(), np.ones_like(one)
    for k in range(int(m.max())):
        on = (m > k)[..., None]
        back = np.where(on, c * back, back)
        front = np.where(on, front * c, front)
    front = front * one
    np.testing.assert_array_equal(_bits(back), _bits(twin["paths"]))  # the restatement restates the oracle
    fold = lambda paths: sum(paths[:, s] for s in range(SPP)) * np.float32(1.0 / np.float32(SPP))  # noqa: E731
    return fold(back), fold(front), m


@pytest.mark.gpu
def test_the_fold_runs_back_to_front():
    """Scene (b), tinted metal: paths of two and more metal bounces tell a_0 * (a_1 * e) from
    (a_0 * a_1) * e.  The wrong order, built from the oracle, differs from the twin on some lit
    pixel, so this test would see it."""
    text, twin = twin_of("b")
    lit = lit_pixels(twin)
    back, front, m = _front_to_back(text, "b")
    assert (m >= 2).any()
    np.testing.assert_array_equal(_bits(back), _bits(twin["img"]))
    assert (_bits(front[lit]) != _bits(twin["img"][lit])).any(axis=1).sum() >= 1
    got = _render(text)
    np.testing.assert_array_equal(_bits(got["albedo"][lit]), _bits(back[lit]))


@pytest.mark.gpu
@pytest.mark.parametrize("max_depth", [0, 1, 2, 3])
def test_depth_limit(max_depth):
    """A path of the shallow twin is the deep twin's path or that path cut at a specular hit,
    black in the twin and (0, 0, 0) by definition: the pixels lit in the deep twin are pixels
    the twin shows at every depth."""
    text, deep = twin_of("a")
    _, twin = twin_of("a", max_depth)
    lit = lit_pixels(deep)
    got = _render(text, max_depth)
    _check_against_twin(got, twin, lit, max_depth)
    if max_depth == 0:  # nothing is followed: a specular first hit is black, its depth the first hit's
        first = capi.Renderer(text).render_aov(NX, NY, SPP, max_depth=0)
        spec = (deep["rays"] > 1).all(axis=1)
        assert spec.sum() > 20 and (_bits(got["albedo"][spec]) == 0).all() and (_bits(got["normal"][spec]) == 0).all()
        np.testing.assert_array_equal(_bits(got["depth"]), _bits(first["depth"]))
        assert got["stats"]["chained_paths"] == 0 and got["stats"]["longest_chain"] == 0


@pytest.mark.gpu
def test_without_specular_materials_it_is_the_first_hit():
    text = scenes.s1_cornell()[0].text()
    first = capi.Renderer(text).render_aov(NX, NY, SPP)
    got = _render(text)
    for k in ("albedo", "normal", "depth"):
        np.testing.assert_array_equal(_bits(got[k]), _bits(first[k]), err_msg=k)
    st = got["stats"]
    assert st["chained_paths"] == 0 and st["longest_chain"] == 0 and st["world_rays"] == st["paths"] == NX * NY * SPP


# ------------------------------------------------------------ normal and depth
MIRROR = 4  # first_hit.WALLS[4]: the back wall z = 555


def mirror_room_text():
    s = Scene()
    white = s.lambertian(s.constant_texture((0.73, 0.73, 0.73)))
    s.set_world(s.hitable_list([
        s.flip_normals(s.yz_rect(0, 555, 0, 555, 555, white)), s.yz_rect(0, 555, 0, 555, 0, white),
        s.flip_normals(s.xz_rect(0, 555, 0, 555, 555, white)), s.xz_rect(0, 555, 0, 555, 0, white),
        s.flip_normals(s.xy_rect(0, 555, 0, 555, 555, s.metal((0.8, 0.8, 0.8), 0.0))),
        s.xy_rect(0, 555, 0, 555, 0, white)]))
    s.camera(first_hit.LOOKFROM, first_hit.LOOKAT, (0, 1, 0), first_hit.VFOV, 1.0, 0.0, 10.0, 0.0, 1.0)
    s.set_lights(s.hitable_list([s.flip_normals(s.xz_rect(213, 343, 227, 332, 554))]))
    return s.text()


def _nearest_wall(o, d):
    """float64: per ray (o[n,3], d[n,3]) the nearest wall, its t, and whether the two nearest
    walls lie within 1e-4 relative of each other."""
    ts = np.full((len(first_hit.WALLS), len(d)), np.inf)
    for k, (ax, kk, _) in enumerate(first_hit.WALLS):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (kk - o[:, ax]) / d[:, ax]
            p = o + t[:, None] * d
        a0, a1 = [a for a in range(3) if a != ax]
        ok = (t > 0.001) & (p[:, a0] >= 0) & (p[:, a0] <= 555) & (p[:, a1] >= 0) & (p[:, a1] <= 555)
        ts[k, ok] = t[ok]
    order = np.argsort(ts, axis=0)
    t0, t1 = np.take_along_axis(ts, order[:1], 0)[0], np.take_along_axis(ts, order[1:2], 0)[0]
    with np.errstate(invalid="ignore"):  # (a ray that leaves through its own origin's edge: inf - inf)
        return order[0], t0, (t1 - t0) <= 1e-4 * t0


def mirror_room_restatement(nx, ny, s_begin, spp):
    """first_hit.room_restatement with the back wall a perfect mirror: per pixel the mean normal
    and depth of the wall seen in it, and whether any segment of any sample passes within 1e-4
    relative of an edge (such pixels may be left out)."""
    o = np.array(first_hit.LOOKFROM)
    focus = 10.0
    hh = np.tan(np.radians(first_hit.VFOV) / 2)
    hw = 1.0 * hh
    w = o - np.array(first_hit.LOOKAT)
    w /= np.linalg.norm(w)
    u = np.cross((0.0, 1.0, 0.0), w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    ll = o - hw * focus * u - hh * focus * v - focus * w
    sob = capi.sobol_points(s_begin + spp)
    row, col = np.mgrid[0:ny, 0:nx]
    i, j = col.ravel().astype(np.float64), (ny - 1 - row.ravel()).astype(np.float64)
    n = nx * ny
    nrm, dep, near = np.zeros((n, 3)), np.zeros(n), np.zeros(n, bool)
    seen_mirror = np.zeros(n, bool)
    for s in range(s_begin, s_begin + spp):
        su, sv = (sob[s, 0] + i) / nx, (sob[s, 1] + j) / ny
        d = ll + su[:, None] * (2 * hw * focus * u) + sv[:, None] * (2 * hh * focus * v) - o
        d /= np.linalg.norm(d, axis=1)[:, None]
        first, t0, near0 = _nearest_wall(np.broadcast_to(o, d.shape), d)
        assert np.isfinite(t0).all()  # a closed room: every ray hits a wall
        near |= near0
        hit_m = first == MIRROR
        seen_mirror |= hit_m
        p = o + t0[:, None] * d
        p[:, 2] = np.where(hit_m, 555.0, p[:, 2])
        d2 = d * np.array([1.0, 1.0, -1.0])  # d - 2 dot(d, n) n for n = (0, 0, -1)
        second, t1, near1 = _nearest_wall(p, d2)
        assert np.isfinite(t1[hit_m]).all() and (second[hit_m] != MIRROR).all()
        near |= hit_m & near1
        last = np.where(hit_m, second, first)
        for k, (ax, _, sign) in enumerate(first_hit.WALLS):
            nrm[last == k, ax] += sign
        dep += t0 + np.where(hit_m, t1, 0.0)
    return nrm / spp, dep / spp, near, seen_mirror


# Pixels left out.  A segment is left out when it passes within 1e-4 t of a wall's edge at
# distance t, where a pixel is 2 tan(35 deg) t / 32 = 0.044 t wide: for a pixel that an edge
# crosses, 2e-4 / 0.044 = 0.5 % of its samples per segment.  With 4 samples of two segments that is
# at most 4 % of such pixels, and the room's edges in view (the mirror's 4, the 4 that run towards
# the camera) and their 8 images behind the mirror cross at most 16 x 32 of the 1024 pixels: 2 % of
# all pixels at the most, the first-hit test's cap, although a path here has two segments.
NEAR_CAP = 0.02


def test_mirror_room_restatement_leaves_out_few_pixels():
    _, _, near, seen = mirror_room_restatement(32, 32, 0, SPP)
    print(f"left out {near.mean():.4f}, mirror in {seen.mean():.3f} of the pixels")
    assert near.mean() <= NEAR_CAP
    assert seen.mean() > 0.3


@pytest.mark.gpu
def test_normal_and_depth_behind_a_mirror():
    nx = ny = 32
    got = capi.Renderer(mirror_room_text()).render_aov(nx, ny, SPP, capi.AOV_NORMAL | capi.AOV_DEPTH,
                                                       through_specular=True)
    assert set(got) == {"normal", "depth", "stats"}
    nrm, dep, near, seen = mirror_room_restatement(nx, ny, 0, SPP)
    keep = ~near
    assert keep.mean() >= 1 - NEAR_CAP
    err_z = np.abs(got["depth"][keep] - dep[keep]) / dep[keep]
    err_n = np.abs(got["normal"][keep] - nrm[keep])
    print(f"depth: max relative error {err_z.max():.3g} (behind the mirror {err_z[seen[keep]].max():.3g}); "
          f"normal: max absolute error {err_n.max():.3g}")
    assert err_z.max() <= 1e-5
    assert err_n.max() <= 1e-6
    assert got["stats"]["longest_chain"] == 1
    # the mirror shows the walls behind the camera: no pixel keeps the mirror's own normal (0, 0, -1)
    assert (got["normal"][keep & seen][:, 2] > -1).all()


# ------------------------------------------------------------ batching, sample ranges
@pytest.mark.gpu
def test_batches_and_sample_ranges():
    text, _ = twin_of("b")
    r = capi.Renderer(text)
    kw = dict(through_specular=True)
    whole = r.render_aov(NX, NY, 8, **kw)
    for batch in (96, 1000, 2500):  # 96: one sample of 96 pixels a batch; 1000: 576 pixels x 1; 2500: 576 x 4
        part = r.render_aov(NX, NY, 8, batch_paths=batch, **kw)
        for k in ("albedo", "normal", "depth"):
            np.testing.assert_array_equal(_bits(part[k]), _bits(whole[k]), err_msg=f"{k} batch {batch}")
        assert part["stats"] == whole["stats"], batch
    # [4, 8) after [0, 4), refolded by hand: the 8-sample sums are those of [0, 4) plus samples 4..7
    # in order.  Single samples are exact (sum * 1.0), so fold them one by one.
    a03 = r.render_aov(NX, NY, 4, **kw)
    ones = [r.render_aov(NX, NY, 1, sample_begin=s, **kw) for s in range(4, 8)]
    a47 = r.render_aov(NX, NY, 4, sample_begin=4, **kw)
    f32 = np.float32
    for k in ("albedo", "normal", "depth"):
        s = a03[k] / f32(0.25)  # the sum: an exact scaling
        t = np.zeros_like(s)
        for one in ones:
            s = s + one[k]
            t = t + one[k]
        np.testing.assert_array_equal(_bits(s * f32(0.125)), _bits(whole[k]), err_msg=k)
        np.testing.assert_array_equal(_bits(t * f32(0.25)), _bits(a47[k]), err_msg=k)
    assert sum(o["stats"]["world_rays"] for o in ones) + a03["stats"]["world_rays"] == whole["stats"]["world_rays"]


# ------------------------------------------------------------ refusals, isolation
@pytest.mark.gpu
def test_refusals():
    L = capi.lib()
    text = SCENES["a"]()
    r = capi.Renderer(text)
    buf = np.zeros(3 * 64, np.float32).ctypes.data  # refusals never write; a host pointer will do

    def call(which=7, flags=0, a=buf, n=buf, z=buf, h=r.h, stats=None, fn=L.srr_render_aov_through, **kw):
        p = capi.make_params(8, 8, 4, flags=flags, **kw)
        return fn(h, ctypes.byref(p), which, a, n, z, stats)
    for fn in (L.srr_render_aov_through, L.srr_render_aov_through_host):
        for flag in (capi.FLAG_CONTINUE, capi.FLAG_KEEP_PATHS, capi.FLAG_COUNT_VISITS, capi.FLAG_SUMS):
            assert call(flags=flag, fn=fn) == EINVAL, flag
        assert call(which=0, fn=fn) == EINVAL
        assert call(which=8, fn=fn) == EINVAL and call(which=15, fn=fn) == EINVAL
        assert call(which=capi.AOV_ALBEDO, a=None, fn=fn) == EINVAL
        assert call(which=capi.AOV_NORMAL, n=None, fn=fn) == EINVAL
        assert call(which=capi.AOV_DEPTH, z=None, fn=fn) == EINVAL
        assert call(which=7, z=None, fn=fn) == EINVAL
        assert call(max_depth=-1, fn=fn) == EINVAL and call(max_depth=65, fn=fn) == EINVAL
        small = capi.AovStats(ctypes.sizeof(capi.AovStats) - 1)
        assert call(stats=ctypes.byref(small), fn=fn) == EINVAL
        assert call(stats=ctypes.byref(capi.AovStats(0)), fn=fn) == EINVAL
    multi = capi.Renderer(text, devices=[0, 0])
    assert call(h=multi.h) == EINVAL
    big = (ctypes.c_char * 64)()  # a caller built against a larger struct: its size is kept
    ctypes.cast(big, ctypes.POINTER(capi.AovStats))[0].struct_size = 64
    host = np.zeros(64, np.float32).ctypes.data
    assert call(which=capi.AOV_DEPTH, a=None, n=None, z=host, stats=ctypes.cast(big, ctypes.POINTER(capi.AovStats)),
                fn=L.srr_render_aov_through_host) == 0
    st = ctypes.cast(big, ctypes.POINTER(capi.AovStats))[0]
    assert st.struct_size == 64 and st.paths == 8 * 8 * 4 and st.world_rays > st.paths
    out = r.render_aov(8, 8, 4, capi.AOV_DEPTH, through_specular=True)  # unselected buffers may be NULL
    assert set(out) == {"depth", "stats"} and (out["depth"] > 0).any()


@pytest.mark.gpu
def test_continue_and_adaptive_state_around_the_call():
    text = SCENES["a"]()
    nx, ny = 24, 20
    kw = dict(through_specular=True)
    whole = capi.Renderer(text).render(nx, ny, 8, 50)["mean"]
    r = capi.Renderer(text)
    r.render(nx, ny, 4, 50)
    r.render_aov(48, 40, 6, **kw)  # another frame size: more pixels than the running sums hold
    r.render_aov(nx, ny, 4, sample_begin=2, max_depth=3, **kw)
    got = r.render(nx, ny, 4, 50, sample_begin=4, flags=capi.FLAG_CONTINUE)["mean"]
    np.testing.assert_array_equal(_bits(got), _bits(whole))
    # an adaptive frame's state stays valid: the variance and the resumed frame are those of a
    # renderer that made no AOV call in between
    ad_kw = dict(batch_spp=8, min_spp=8, rel_tol=0.05)
    r2, r3 = capi.Renderer(text), capi.Renderer(text)
    ad = r2.render_adaptive(nx, ny, 16, 50, **ad_kw)
    r3.render_adaptive(nx, ny, 16, 50, **ad_kw)
    r2.render_aov(48, 40, 6, **kw)
    np.testing.assert_array_equal(_bits(r2.adaptive_variance(ad["count"])), _bits(r3.adaptive_variance(ad["count"])))
    more, want = r2.render_adaptive_resume(nx, ny, 24, 50, **ad_kw), r3.render_adaptive_resume(nx, ny, 24, 50, **ad_kw)
    np.testing.assert_array_equal(_bits(more["mean"]), _bits(want["mean"]))
    np.testing.assert_array_equal(more["count"], want["count"])


@pytest.mark.gpu
def test_progressive_takes_the_guides_through_specular():
    from srr.progressive import Progressive
    text = SCENES["a"]()
    shape = (NY, NX, 3)
    r = capi.Renderer(text)
    noisy = r.render(NX, NY, 8, 50)["mean"]
    a = r.render_aov(NX, NY, 4, through_specular=True)
    want = capi.denoise(noisy.reshape(shape), a["albedo"].reshape(shape), a["normal"].reshape(shape),
                        a["depth"].reshape(NY, NX)).reshape(-1, 3)
    pr = Progressive(capi.Renderer(text), NX, NY, denoise=True, aov_spp=4, aov_through_specular=True)
    np.testing.assert_array_equal(_bits(pr.step(8)), _bits(want))
    plain = Progressive(capi.Renderer(text), NX, NY, denoise=True, aov_spp=4)
    assert (_bits(plain.step(8)) != _bits(want)).any()


# ------------------------------------------------------------ render_main
@pytest.mark.gpu
def test_render_main_writes_these_buffers(tmp_path):
    from srr import render_main
    text, _ = twin_of("a")
    scene, out, prefix = tmp_path / "a.scene", str(tmp_path / "o.ppm"), str(tmp_path / "aov")
    scene.write_text(text)
    base = [EXE, "--scene-text", str(scene), "--nx", str(NX), "--ny", str(NY), "--ns", "4", "--out", out]
    r = subprocess.run(base + ["--aov-through-specular", "--aov-out", prefix], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    got = _render(text)
    for k, img in render_main.aov_images(got).items():
        want = str(tmp_path / f"want_{k}.png")
        capi.write_png(want, NX, NY, img)
        assert open(f"{prefix}_{k}.png", "rb").read() == open(want, "rb").read(), k
    # usage errors, before any GPU work: nothing to guide, and more than one device
    for bad in (["--aov-through-specular"], ["--aov-through-specular", "--aov-out", prefix, "--gpus", "2"],
                ["--aov-through-specular", "--denoise", "--devices", "0,0"]):
        assert subprocess.run(base + bad, capture_output=True, text=True, timeout=60).returncode == 2, bad
    assert render_main.main(["--aov-through-specular"]) == 2
    assert render_main.main(["--aov-through-specular", "--denoise", "--gpus", "2"]) == 2
