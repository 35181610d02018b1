"""First-hit AOVs on the GPU (srr_render_aov).

Albedo: bit-exact against the CPU oracle.  A scene's text is rewritten so that every
material becomes a diffuse_light of its albedo texture (a metal's colour and a
dielectric's (1, 1, 1) get a new const texture): an emitter never scatters, so the
oracle's image of the rewritten scene IS the mean first-hit albedo -- as long as every
primary hit faces the camera (diffuse_light emits to its front only), which
test_emissive_twin_covers_every_primary_hit checks on the CPU.

Normal and depth: against a float64 numpy restatement of the pinhole camera and the
closest axis-aligned rect of a closed room."""
import ctypes

import numpy as np
import pytest

import oracle_bind as ob
from srr import capi, scenes
from srr.scene import Scene

NX = NY = 32
SPP = 4
EINVAL = -22


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def emissive_twin(text: str) -> str:
    """Every `mat` line -> diffuse_light of the material's albedo."""
    out, k = [], 0
    for line in text.split("\n"):
        t = line.split()
        if t[:1] == ["mat"]:
            if t[2] in ("metal", "dielectric"):
                rgb = t[3:6] if t[2] == "metal" else ["1.0", "1.0", "1.0"]
                tex = 1000000 + k
                k += 1
                out.append(f"tex {tex} const {' '.join(rgb)}")
            else:
                tex = t[3]
            line = f"mat {t[1]} diffuse_light {tex}"
        out.append(line)
    return "\n".join(out)


CORNELL = {"s1": scenes.s1_cornell, "s2": scenes.s2_cornell_teapot, "s3": scenes.s3_cornell_teapot_microfacet}


@pytest.fixture(scope="module", params=sorted(CORNELL))
def cornell(request):
    text = CORNELL[request.param]()[0].text()
    twin = ob.render(emissive_twin(text), NX, NY, SPP, 50)
    for a in twin.values():
        a.setflags(write=False)
    return text, twin


def test_emissive_twin_covers_every_primary_hit(cornell):
    """CPU: a path of the twin is black only where the original's primary ray missed
    (one world ray, no radiance): no primary hit shows its back to the camera."""
    text, twin = cornell
    orig = ob.render(text, NX, NY, SPP, 50)
    black = (twin["paths"] == 0).all(axis=2)
    missed = (orig["rays"] == 1) & (orig["paths"] == 0).all(axis=2)
    assert not (black & ~missed).any()
    assert (~black).mean() > 0.9  # and the frame is mostly hits


@pytest.mark.gpu
def test_albedo_is_the_oracles_emissive_twin(cornell):
    text, twin = cornell
    got = capi.Renderer(text).render_aov(NX, NY, SPP, capi.AOV_ALBEDO)
    assert set(got) == {"albedo"}
    np.testing.assert_array_equal(_bits(got["albedo"]), _bits(twin["img"]))


@pytest.mark.gpu
def test_albedo_of_a_textured_scene_in_batches():
    """S4 (generated image textures, orennayar floor, beckmann mesh, glass, an emissive
    sky sphere seen from inside) -- the emitters' back faces are what the twin cannot
    show, so compare only pixels whose twin paths are all lit; batch_paths splits the
    frame into pixel and sample chunks."""
    nx = ny = 24
    text = scenes.s4_soldier_standin()[0].text()
    twin = ob.render(emissive_twin(text), nx, ny, SPP, 50)
    lit = (twin["paths"] != 0).any(axis=2).all(axis=1)
    assert lit.mean() > 0.5
    r = capi.Renderer(text)
    whole = r.render_aov(nx, ny, SPP)
    np.testing.assert_array_equal(_bits(whole["albedo"][lit]), _bits(twin["img"][lit]))
    for batch in (100, 700):  # 100: sample chunks of 1 over pixel chunks of 100; 700: 576 pixels x 1 sample
        part = r.render_aov(nx, ny, SPP, batch_paths=batch)
        for k in ("albedo", "normal", "depth"):
            np.testing.assert_array_equal(_bits(part[k]), _bits(whole[k]), err_msg=f"{k} batch {batch}")


# ------------------------------------------------------------ normal and depth
LOOKFROM, LOOKAT, VFOV = (278.0, 278.0, 100.0), (278.0, 300.0, 555.0), 70.0
# (axis, k, normal sign as color() sees it) of the room's walls, all spanning 0..555
WALLS = [(0, 555.0, -1), (0, 0.0, 1), (1, 555.0, -1), (1, 0.0, 1), (2, 555.0, -1), (2, 0.0, 1)]


def room_text(front=True):
    s = Scene()
    white = s.lambertian(s.constant_texture((0.73, 0.73, 0.73)))
    w = [s.flip_normals(s.yz_rect(0, 555, 0, 555, 555, white)), s.yz_rect(0, 555, 0, 555, 0, white),
         s.flip_normals(s.xz_rect(0, 555, 0, 555, 555, white)), s.xz_rect(0, 555, 0, 555, 0, white),
         s.flip_normals(s.xy_rect(0, 555, 0, 555, 555, white))]
    if front:
        w.append(s.xy_rect(0, 555, 0, 555, 0, white))
    s.set_world(s.hitable_list(w))
    s.camera(LOOKFROM, LOOKAT, (0, 1, 0), VFOV, 1.0, 0.0, 10.0, 0.0, 1.0)
    s.set_lights(s.hitable_list([s.flip_normals(s.xz_rect(213, 343, 227, 332, 554))]))
    return s.text()


def room_restatement(nx, ny, s_begin, spp):
    """float64: per pixel the mean normal, mean depth, and whether any sample's two
    nearest walls lie within 1e-4 relative of each other (such pixels may be left out)."""
    o = np.array(LOOKFROM)
    focus = 10.0
    hh = np.tan(np.radians(VFOV) / 2)
    hw = 1.0 * hh
    w = o - np.array(LOOKAT)
    w /= np.linalg.norm(w)
    u = np.cross((0.0, 1.0, 0.0), w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    ll = o - hw * focus * u - hh * focus * v - focus * w
    sob = capi.sobol_points(s_begin + spp)
    row, col = np.mgrid[0:ny, 0:nx]
    i, j = col.ravel().astype(np.float64), (ny - 1 - row.ravel()).astype(np.float64)
    nrm, dep = np.zeros((nx * ny, 3)), np.zeros(nx * ny)
    near = np.zeros(nx * ny, bool)
    for s in range(s_begin, s_begin + spp):
        su, sv = (sob[s, 0] + i) / nx, (sob[s, 1] + j) / ny
        d = ll + su[:, None] * (2 * hw * focus * u) + sv[:, None] * (2 * hh * focus * v) - o
        ts = np.full((len(WALLS), nx * ny), np.inf)
        for k, (ax, kk, _) in enumerate(WALLS):
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (kk - o[ax]) / d[:, ax]
                p = o + t[:, None] * d
            a0, a1 = [a for a in range(3) if a != ax]
            ok = (t > 0.001) & (p[:, a0] >= 0) & (p[:, a0] <= 555) & (p[:, a1] >= 0) & (p[:, a1] <= 555)
            ts[k, ok] = t[ok]
        order = np.argsort(ts, axis=0)
        first = order[0]
        t0, t1 = np.take_along_axis(ts, order[:1], 0)[0], np.take_along_axis(ts, order[1:2], 0)[0]
        assert np.isfinite(t0).all()  # a closed room: every ray hits a wall
        near |= (t1 - t0) <= 1e-4 * t0
        for k, (ax, _, sign) in enumerate(WALLS):
            nrm[first == k, ax] += sign
        dep += t0 * np.linalg.norm(d, axis=1)
    return nrm / spp, dep / spp, near


def test_room_restatement_leaves_out_few_pixels():
    _, _, near = room_restatement(NX, NY, 0, SPP)
    assert near.mean() <= 0.02


@pytest.mark.gpu
def test_normal_and_depth_of_a_closed_room():
    got = capi.Renderer(room_text()).render_aov(NX, NY, SPP, capi.AOV_NORMAL | capi.AOV_DEPTH)
    assert set(got) == {"normal", "depth"}
    nrm, dep, near = room_restatement(NX, NY, 0, SPP)
    keep = ~near
    assert keep.mean() >= 0.98
    err_z = np.abs(got["depth"][keep] - dep[keep]) / dep[keep]
    err_n = np.abs(got["normal"][keep] - nrm[keep])
    print(f"depth: max relative error {err_z.max():.3g}; normal: max absolute error {err_n.max():.3g}")
    assert err_z.max() <= 1e-5
    assert err_n.max() <= 1e-6
    assert (np.abs(nrm[keep]).sum(axis=1) > 0.99).all()  # and they are unit axis vectors (or means of them)


@pytest.mark.gpu
def test_misses_are_zero():
    """A unit sphere under an open sky: the pixels around it miss."""
    s = Scene()
    white = s.lambertian(s.constant_texture((0.73, 0.73, 0.73)))
    s.set_world(s.hitable_list([s.sphere((0, 0, 0), 1.0, white)]))
    s.camera((0, 0, -6), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    s.set_lights(s.hitable_list([s.flip_normals(s.xz_rect(-1, 1, -1, 1, 5))]))
    got = capi.Renderer(s.text()).render_aov(16, 16, 2)
    hit = got["depth"] > 0
    assert hit[16 * 8 + 8] and not hit[0] and 0.05 < hit.mean() < 0.5
    for k in ("albedo", "normal"):
        assert (_bits(got[k][~hit]) == 0).all()
    assert (_bits(got["depth"][~hit]) == 0).all()
    np.testing.assert_array_equal(got["albedo"][16 * 8 + 8], np.float32([0.73, 0.73, 0.73]))
    # pixel (8, 8) looks at most 0.0625 * 2 tan(20 deg) * 6 = 0.27 off the axis in x and in y:
    # its hits lie within 0.39 of the sphere's near pole, at 5 <= depth < 6 - sqrt(1 - 0.39^2) + 0.1
    assert 5.0 <= got["depth"][16 * 8 + 8] < 5.18 and got["normal"][16 * 8 + 8][2] < -0.9


@pytest.mark.gpu
def test_sample_range():
    """Samples 4..7 on their own against the 8-sample and the first-4-sample calls:
    sum8 = sum(0..3) then + s4, s5, s6, s7 in order, so for pixels whose samples 4..7
    are all equal (flat walls: albedo, normal) the sums must agree bitwise; for every
    pixel mean(4..7) must match (8 mean8 - 4 mean03) / 4 to rounding."""
    r = capi.Renderer(room_text())
    a03 = r.render_aov(NX, NY, 4)
    a47 = r.render_aov(NX, NY, 4, sample_begin=4)
    a08 = r.render_aov(NX, NY, 8)
    f32 = np.float32
    for k in ("albedo", "normal", "depth"):
        s03, s47, s08 = a03[k] / f32(0.25), a47[k] / f32(0.25), a08[k] / f32(0.125)  # the sums: exact scalings
        if k == "albedo":  # every sample is (0.73, 0.73, 0.73): unfold by hand
            want = s03.copy()
            for _ in range(4):
                want = want + f32(0.73)
            np.testing.assert_array_equal(_bits(s08), _bits(want))
            np.testing.assert_array_equal(_bits(a47[k]), _bits(a03[k]))
        np.testing.assert_allclose(s08, s03.astype(np.float64) + s47, rtol=1e-6, atol=1e-6)
    assert (_bits(a47["depth"]) != _bits(a03["depth"])).mean() > 0.9  # other Sobol points: other rays


@pytest.mark.gpu
def test_refusals():
    L = capi.lib()
    text = scenes.s1_cornell()[0].text()
    r = capi.Renderer(text)
    buf = np.zeros(3 * 64, np.float32).ctypes.data  # refusals never write; a host pointer will do

    def call(which=7, flags=0, a=buf, n=buf, z=buf, h=r.h, **kw):
        p = capi.make_params(8, 8, 4, flags=flags, **kw)
        return L.srr_render_aov(h, ctypes.byref(p), which, a, n, z)
    for flag in (capi.FLAG_CONTINUE, capi.FLAG_KEEP_PATHS, capi.FLAG_COUNT_VISITS, capi.FLAG_SUMS):
        assert call(flags=flag) == EINVAL, flag
    assert call(which=0) == EINVAL
    assert call(which=8) == EINVAL and call(which=15) == EINVAL
    assert call(which=capi.AOV_ALBEDO, a=None) == EINVAL
    assert call(which=capi.AOV_NORMAL, n=None) == EINVAL
    assert call(which=capi.AOV_DEPTH, z=None) == EINVAL
    assert call(which=7, z=None) == EINVAL
    multi = capi.Renderer(text, devices=[0, 0])
    assert call(h=multi.h) == EINVAL
    out = r.render_aov(8, 8, 4, capi.AOV_DEPTH)  # unselected buffers may be NULL
    assert set(out) == {"depth"} and (out["depth"] > 0).any()


@pytest.mark.gpu
def test_continue_after_an_aov_call_is_the_uninterrupted_frame():
    text = scenes.s1_cornell()[0].text()
    nx, ny = 24, 20
    whole = capi.Renderer(text).render(nx, ny, 8, 50)["mean"]
    r = capi.Renderer(text)
    r.render(nx, ny, 4, 50)
    r.render_aov(48, 40, 6)  # another frame size: more pixels than the running sums hold
    r.render_aov(nx, ny, 4, sample_begin=2)
    got = r.render(nx, ny, 4, 50, sample_begin=4, flags=capi.FLAG_CONTINUE)["mean"]
    np.testing.assert_array_equal(_bits(got), _bits(whole))
