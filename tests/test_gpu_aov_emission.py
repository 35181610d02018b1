"""The emission buffer on the GPU (srr_render_aov_emission).

First hit: emitted() of the primary hit is what color() returns at max_depth = 0, so the
buffer is, bit for bit and on every pixel, the CPU oracle's beauty image at max_depth = 0.
Through specular: bit for bit the oracle's image of the scene's EMISSION TWIN at the same
max_depth -- metal, dielectric and diffuse_light stay, every other material becomes a
diffuse_light of a constant (0, 0, 0) texture: the specular bounces draw what they draw in the
beauty frame, a light emits to its front only in both, and color() folds the attenuations back
to front.  No lit-pixel mask: a black terminal hit is black in both.

The scene is test_gpu_aov_through.box_text's room with the camera tilted up, a light with a
checker texture on the left wall and a light that the camera sees only from behind; the CPU
tests assert what the GPU tests rely on (lit pixels, rim pixels, chains of two bounces)."""
import ctypes

import numpy as np
import pytest

import oracle_bind as ob
import test_gpu_aov as first_hit
from srr import capi, scenes
from srr.scene import Scene

NX = NY = 24
SPP = 4
EINVAL = -22
ALL = capi.AOV_ALBEDO | capi.AOV_NORMAL | capi.AOV_DEPTH | capi.AOV_EMISSION
_bits = first_hit._bits
f32 = np.float32


def room_text(fuzz=0.0, tint=(1.0, 1.0, 1.0)):
    s = Scene()
    red = s.lambertian(s.constant_texture(scenes.RED))
    white = s.lambertian(s.constant_texture(scenes.WHITE))
    green = s.lambertian(s.constant_texture(scenes.GREEN))
    light = s.diffuse_light(s.constant_texture(15.0))
    panel = s.diffuse_light(s.checker_texture(s.constant_texture((4.0, 1.0, 0.5)), s.constant_texture((0.5, 2.0, 6.0))))
    mirror = s.metal(tint, fuzz)
    glass = s.dielectric(1.5)
    s.set_world(s.hitable_list([
        s.flip_normals(s.yz_rect(0, 555, 0, 555, 555, green)), s.yz_rect(0, 555, 0, 555, 0, red),
        s.flip_normals(s.xz_rect(0, 555, 0, 555, 555, white)), s.xz_rect(0, 555, 0, 555, 0, white),
        s.flip_normals(s.xy_rect(0, 555, 0, 555, 555, mirror)), s.xy_rect(0, 555, 0, 555, 0, white),
        s.flip_normals(s.xz_rect(213, 343, 227, 332, 554, light)),
        s.yz_rect(150, 300, 200, 400, 1, panel),      # a textured light on the left wall
        s.xz_rect(380, 480, 250, 350, 300, light),    # unflipped, above the camera: seen from behind only
        s.xz_rect(100, 455, 300, 540, 1, mirror),
        s.sphere((170, 120, 300), 90, glass),
        s.box((330, 40, 250), (450, 200, 370), glass)]))
    s.camera((278, 278, 20), (278, 330, 555), (0, 1, 0), 80.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    s.set_lights(s.hitable_list([s.flip_normals(s.xz_rect(213, 343, 227, 332, 554))]))
    return s.text()


def emission_twin(text: str) -> str:
    """`mat` lines of metal, dielectric and diffuse_light stay; every other one -> a diffuse_light
    of a constant (0, 0, 0) texture."""
    out, black = [], None
    for line in text.split("\n"):
        t = line.split()
        if t[:1] == ["mat"] and t[2] not in ("metal", "dielectric", "diffuse_light"):
            if black is None:
                black = 2000000
                out.append(f"tex {black} const 0.0 0.0 0.0")
            line = f"mat {t[1]} diffuse_light {black}"
        out.append(line)
    return "\n".join(out)


ROOMS = {"plain": lambda: room_text(), "tinted": lambda: room_text(0.3, (0.9, 0.6, 0.3))}
_cache = {}


def _frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


def first_of(name):
    """(scene text, the oracle's max_depth-0 render), computed once and read-only."""
    if ("first", name) not in _cache:
        text = ROOMS[name]()
        _cache["first", name] = (text, _frozen(ob.render(text, NX, NY, SPP, 0)))
    return _cache["first", name]


def twin_of(name, max_depth=50):
    if (name, max_depth) not in _cache:
        text = ROOMS[name]()
        _cache[name, max_depth] = (text, _frozen(ob.render(emission_twin(text), NX, NY, SPP, max_depth)))
    return _cache[name, max_depth]


def _lit(paths):
    return (paths != 0).any(axis=2)  # [pixel, sample]


# ------------------------------------------------------------ CPU: the conditions of the scene
def test_the_scene_shows_lights_rims_and_textures():
    _, first = first_of("plain")
    lit = _lit(first["paths"])
    values = np.unique(first["paths"][lit], axis=0)
    rim = lit.any(axis=1) & ~lit.all(axis=1)
    print(f"first hit: {lit.any(axis=1).sum()} lit pixels, {rim.sum()} rim pixels, {len(values)} emission values")
    assert not np.isnan(first["paths"]).any()
    assert lit.any(axis=1).sum() >= 20
    assert rim.sum() >= 10
    assert len(values) >= 3
    assert (first["rays"] == 1).all()  # max_depth 0: the image is the first hit's emitted()


@pytest.mark.parametrize("name", sorted(ROOMS))
def test_the_scene_shows_lights_through_chains(name):
    _, first = first_of(name)
    _, twin = twin_of(name)
    lit = _lit(twin["paths"])
    chained = lit & (twin["rays"] > 1)
    differ = (_bits(twin["img"]) != _bits(first["img"])).any(axis=1)
    print(f"{name}: through specular {lit.any(axis=1).sum()} lit pixels, {chained.sum()} lit paths through a chain, "
          f"{(lit & (twin['rays'] > 2)).sum()} through two or more bounces, {differ.sum()} pixels differ from the first hit")
    assert not np.isnan(twin["paths"]).any()
    assert chained.sum() >= 20
    assert (lit & (twin["rays"] > 2)).sum() >= 1
    assert differ.sum() >= 1


def test_emission_twin_keeps_the_lights_and_the_specular_materials():
    text = ROOMS["plain"]()
    kinds = lambda t: [ln.split()[2] for ln in t.split("\n") if ln.startswith("mat ")]  # noqa: E731
    before, after = kinds(text), kinds(emission_twin(text))
    assert [b for b in before if b in ("metal", "dielectric")] == [a for a in after if a in ("metal", "dielectric")]
    assert all(a in ("metal", "dielectric", "diffuse_light") for a in after) and len(after) == len(before)
    assert after.count("diffuse_light") == before.count("diffuse_light") + before.count("lambertian")


# ------------------------------------------------------------ GPU
def _render(text, which=capi.AOV_EMISSION, through=False, max_depth=50, spp=SPP, **kw):
    return capi.Renderer(text).render_aov(NX, NY, spp, which, max_depth=max_depth, through_specular=through, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROOMS))
def test_first_hit_emission_is_the_frame_at_depth_zero(name):
    text, first = first_of(name)
    got = _render(text)
    assert set(got) == {"emission", "stats"}
    np.testing.assert_array_equal(_bits(got["emission"]), _bits(first["img"]))
    frame = capi.Renderer(text).render(NX, NY, SPP, 0)["mean"]
    np.testing.assert_array_equal(_bits(got["emission"]), _bits(frame))
    assert got["stats"] == dict(longest_chain=0, paths=NX * NY * SPP, world_rays=NX * NY * SPP, chained_paths=0)
    # p->max_depth does not matter to the first hit
    np.testing.assert_array_equal(_bits(_render(text, max_depth=0)["emission"]), _bits(got["emission"]))


@pytest.mark.gpu
@pytest.mark.parametrize("max_depth", [0, 1, 2, 50])
@pytest.mark.parametrize("name", sorted(ROOMS))
def test_through_specular_emission_is_the_oracles_emission_twin(name, max_depth):
    text, twin = twin_of(name, max_depth)
    r = capi.Renderer(text)
    got = r.render_aov(NX, NY, SPP, capi.AOV_EMISSION, max_depth=max_depth, through_specular=True)
    np.testing.assert_array_equal(_bits(got["emission"]), _bits(twin["img"]))
    old = r.render_aov(NX, NY, SPP, max_depth=max_depth, through_specular=True)
    assert got["stats"] == old["stats"]
    assert got["stats"]["world_rays"] == int(twin["rays"].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("through", [False, True])
def test_all_four_bits_leave_the_three_old_buffers_as_they_are(through):
    text, _ = twin_of("tinted")
    r = capi.Renderer(text)
    got = r.render_aov(NX, NY, SPP, ALL, through_specular=through)
    old = r.render_aov(NX, NY, SPP, through_specular=through)
    alone = r.render_aov(NX, NY, SPP, capi.AOV_EMISSION, through_specular=through)
    assert set(got) == {"albedo", "normal", "depth", "emission", "stats"}
    for k in ("albedo", "normal", "depth"):
        np.testing.assert_array_equal(_bits(got[k]), _bits(old[k]), err_msg=k)
    np.testing.assert_array_equal(_bits(got["emission"]), _bits(alone["emission"]))
    if through:
        assert got["stats"] == old["stats"]


@pytest.mark.gpu
def test_without_specular_materials_the_two_emissions_are_equal():
    text = scenes.s1_cornell()[0].text()
    a, b = _render(text), _render(text, through=True)
    np.testing.assert_array_equal(_bits(a["emission"]), _bits(b["emission"]))
    assert (a["emission"] > 0).any()
    assert b["stats"]["chained_paths"] == 0


@pytest.mark.gpu
def test_the_back_of_a_light_has_its_albedo_and_no_emission():
    """64 x 64 x 16: at 24 x 24 the rect above the camera is less than a pixel tall."""
    got = capi.Renderer(ROOMS["plain"]()).render_aov(64, 64, 16, ALL)
    back = (got["albedo"] == f32(15.0)).all(axis=1) & (_bits(got["emission"]) == 0).all(axis=1)
    front = (got["albedo"] == f32(15.0)).all(axis=1) & (got["emission"] == f32(15.0)).all(axis=1)
    print(f"{back.sum()} pixels on the back of a light, {front.sum()} on the front of one")
    assert back.sum() >= 1 and front.sum() >= 1


def _fold(paths, count):
    """Pixel i: the sequential float32 sum of paths[i, :count[i]] times float32(1.0 / float32(count[i]))."""
    out = np.zeros((paths.shape[0], 3), f32)
    for i, n in enumerate(count):
        s = np.zeros(3, f32)
        for k in range(int(n)):
            s = s + paths[i, k]
        out[i] = s * f32(1.0 / f32(n))
    return out


def _counts():
    count = (np.arange(NX * NY, dtype=np.int32) * 7 // 3) % SPP + 1
    assert set(count.tolist()) == {1, 2, 3, 4}
    return count


@pytest.mark.gpu
@pytest.mark.parametrize("through", [False, True])
def test_count_folds_the_first_samples_of_each_pixel(through):
    text, ref = twin_of("tinted") if through else first_of("tinted")
    count = _counts()
    want = _fold(ref["paths"], count)
    assert (_bits(want) != _bits(ref["img"])).any()  # the counts matter on this scene
    r = capi.Renderer(text)
    kw = dict(through_specular=through, count=count)
    got = r.render_aov(NX, NY, SPP, capi.AOV_EMISSION, **kw)
    np.testing.assert_array_equal(_bits(got["emission"]), _bits(want))
    # 64: one sample of 64 pixels a batch; 1200: all pixels x 2 samples, a pixel's samples span two batches
    for batch in (64, 1200):
        part = r.render_aov(NX, NY, SPP, capi.AOV_EMISSION, batch_paths=batch, **kw)
        np.testing.assert_array_equal(_bits(part["emission"]), _bits(want), err_msg=f"batch {batch}")
    # albedo, normal and depth ignore it
    four = r.render_aov(NX, NY, SPP, ALL, **kw)
    old = r.render_aov(NX, NY, SPP, through_specular=through)
    for k in ("albedo", "normal", "depth"):
        np.testing.assert_array_equal(_bits(four[k]), _bits(old[k]), err_msg=k)
    np.testing.assert_array_equal(_bits(four["emission"]), _bits(want))


@pytest.mark.gpu
def test_a_device_count_out_of_range_is_clamped():
    import torch
    text, first = first_of("plain")
    r = capi.Renderer(text)
    count = _counts()
    wild = count.copy()
    wild[count == 1] = 0
    wild[count == SPP] = SPP + 5
    wild[0] = -3
    want = _fold(first["paths"], np.clip(wild, 1, SPP))
    d_count = torch.from_numpy(wild).cuda()
    d_em = torch.zeros(NX * NY, 3, device="cuda")
    torch.cuda.synchronize()
    p = capi.make_params(NX, NY, SPP)
    r.render_aov_device(p, capi.AOV_EMISSION, d_emission_ptr=d_em.data_ptr(), d_count_ptr=d_count.data_ptr())
    np.testing.assert_array_equal(_bits(d_em.cpu().numpy()), _bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("through", [False, True])
def test_batches_and_sample_ranges(through):
    text, _ = twin_of("tinted")
    r = capi.Renderer(text)
    kw = dict(through_specular=through)
    whole = r.render_aov(NX, NY, 8, ALL, **kw)
    for batch in (64, 1000, 2500):
        part = r.render_aov(NX, NY, 8, ALL, batch_paths=batch, **kw)
        for k in ("albedo", "normal", "depth", "emission"):
            np.testing.assert_array_equal(_bits(part[k]), _bits(whole[k]), err_msg=f"{k} batch {batch}")
        assert part["stats"] == whole["stats"]
    # [4, 8): single samples are exact (sum * 1.0), so fold them by hand
    ones = [r.render_aov(NX, NY, 1, capi.AOV_EMISSION, sample_begin=s, **kw)["emission"] for s in range(4, 8)]
    a47 = r.render_aov(NX, NY, 4, capi.AOV_EMISSION, sample_begin=4, **kw)["emission"]
    t = np.zeros_like(a47)
    for one in ones:
        t = t + one
    np.testing.assert_array_equal(_bits(t * f32(0.25)), _bits(a47))


@pytest.mark.gpu
def test_refusals_and_the_frame_goes_on():
    L = capi.lib()
    text = ROOMS["plain"]()
    r = capi.Renderer(text)
    buf = np.zeros(3 * 64, np.float32).ctypes.data  # refusals never write; a host pointer will do
    ok_count = np.full(64, 2, np.int32)

    def call(which=ALL, through=0, flags=0, a=buf, n=buf, z=buf, e=buf, count=None, h=r.h, stats=None,
             fn=L.srr_render_aov_emission, **kw):
        p = capi.make_params(8, 8, 4, flags=flags, **kw)
        return fn(h, ctypes.byref(p), which, through, a, n, z, e, count, stats)
    for fn in (L.srr_render_aov_emission, L.srr_render_aov_emission_host):
        for flag in (capi.FLAG_CONTINUE, capi.FLAG_KEEP_PATHS, capi.FLAG_COUNT_VISITS, capi.FLAG_SUMS):
            assert call(flags=flag, fn=fn) == EINVAL, flag
            assert call(flags=flag, which=capi.AOV_EMISSION, fn=fn) == EINVAL, flag
        assert call(which=0, fn=fn) == EINVAL and call(which=16, fn=fn) == EINVAL and call(which=31, fn=fn) == EINVAL
        assert call(e=None, fn=fn) == EINVAL and call(which=capi.AOV_EMISSION, e=None, fn=fn) == EINVAL
        assert call(which=capi.AOV_EMISSION | capi.AOV_DEPTH, z=None, fn=fn) == EINVAL
        assert call(through=2, fn=fn) == EINVAL and call(through=-1, fn=fn) == EINVAL
        assert call(max_depth=65, fn=fn) == EINVAL
        assert call(stats=ctypes.byref(capi.AovStats(0)), fn=fn) == EINVAL
    multi = capi.Renderer(text, devices=[0, 0])
    assert call(h=multi.h) == EINVAL
    for bad in (0, 5):
        count = ok_count.copy()
        count[17] = bad
        for which in (ALL, capi.AOV_EMISSION):
            assert call(which=which, count=count.ctypes.data, fn=L.srr_render_aov_emission_host) == EINVAL, bad
    host = [np.zeros(3 * 64, np.float32) for _ in range(4)]
    assert call(a=host[0].ctypes.data, n=host[1].ctypes.data, z=host[2].ctypes.data, e=host[3].ctypes.data,
                count=ok_count.ctypes.data, fn=L.srr_render_aov_emission_host) == 0
    assert (host[0] > 0).any()
    # unselected buffers may be NULL; bit 8 clear: the old three alone, the emission pointer unread
    out = r.render_aov(8, 8, 4, capi.AOV_EMISSION | capi.AOV_DEPTH)
    assert set(out) == {"depth", "emission", "stats"} and (out["depth"] > 0).any()
    assert call(which=7, e=None, a=host[0].ctypes.data, n=host[1].ctypes.data, z=host[2].ctypes.data,
                fn=L.srr_render_aov_emission_host) == 0
    with pytest.raises(capi.SrrError):
        r.render_aov(8, 8, 4, count=ok_count)  # count= without the emission bit


@pytest.mark.gpu
def test_continue_after_the_call_is_the_uninterrupted_frame():
    text = ROOMS["plain"]()
    nx, ny = 24, 20
    whole = capi.Renderer(text).render(nx, ny, 8, 50)["mean"]
    r = capi.Renderer(text)
    r.render(nx, ny, 4, 50)
    r.render_aov(48, 40, 6, ALL, through_specular=True)  # another frame size: more pixels than the running sums hold
    r.render_aov(nx, ny, 4, capi.AOV_EMISSION, sample_begin=2, count=np.full(nx * ny, 3, np.int32))
    with pytest.raises(capi.SrrError):  # a refused call in between
        r.render_aov(nx, ny, 4, ALL, flags=capi.FLAG_CONTINUE)
    got = r.render(nx, ny, 4, 50, sample_begin=4, flags=capi.FLAG_CONTINUE)["mean"]
    np.testing.assert_array_equal(_bits(got), _bits(whole))
