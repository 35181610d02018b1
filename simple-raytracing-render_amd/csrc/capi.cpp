// The product's entry points of the C-ABI (include/srr_capi.h): scene building, renderers (the
// render driver itself is renderer.cpp and multi.cpp), AOVs, the denoiser, image and mesh files,
// MERL tables.  The test entry points (device KATs, libm sweeps) are in capi_kat.cpp, and
// capi_internal.h holds what the two files share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "adaptive_schedule.h"
#include "capi_internal.h"
#include "denoise.h"
#include "imageio.h"
#include "meshio.h"
#include "../../include/srr/merl.h"
#include "multi.h"
#include "renderer.h"

using namespace srr;

namespace {
thread_local std::string g_err;
}  // namespace

// a failed allocation, worded by the buffer it was for ("staging image: out of memory")
#define MEMCHK(x, code, what)                                                                  \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess) return fail(code, std::string(what) + ": " + hipGetErrorString(e_)); \
  } while (0)

int srr::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

extern "C" {

const char* srr_last_error(void) { return g_err.c_str(); }
const char* srr_version(void) { return "srr 0.1 (gfx950 wavefront path tracer)"; }

// ------------------------------------------------------------------ scene
srr_scene* srr_scene_create(void) { return new srr_scene(); }
void srr_scene_destroy(srr_scene* s) { delete s; }

int srr_scene_from_text(const char* text, srr_scene** out) {
  if (!text || !out) return fail(SRR_EINVAL, "null argument");
  std::unique_ptr<srr_scene> s(new srr_scene());
  std::string err;
  int rc = scene_from_text(text, s->s, err);
  if (rc < 0) return fail(rc, err);
  *out = s.release();
  return 0;
}

int srr_scene_text_handle(const srr_scene* s, int id) {
  if (!s) return fail(SRR_EINVAL, "null scene");
  for (auto& kv : s->s.text_ids)
    if (kv.first == id) return kv.second;
  return fail(SRR_EINVAL, "no such text object id");
}

// FNV-1a 64 over the flattened device tables (scene.h Flat): two scenes with the
// same digest upload byte-identical objects, transforms, primitives, BVHs (both
// layouts), triangles, media, materials, textures and image bytes, lights and camera.
// parts (optional, SRR_DIGEST_PARTS entries): one digest per table, in that order.
int srr_scene_digest(const srr_scene* s, uint64_t* out, uint64_t* parts) {
  if (!s || !out) return fail(SRR_EINVAL, "null argument");
  Flat f;
  std::string err;
  const int rc = flatten(s->s, f, err);
  if (rc < 0) return fail(rc, err);
  uint64_t h = 0xcbf29ce484222325ULL;
  int part = 0;
  auto mix = [](uint64_t& x, const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) x = (x ^ b[i]) * 0x100000001b3ULL;
  };
  auto blob = [&](const void* p, size_t n) {
    mix(h, &n, sizeof n);
    mix(h, p, n);
    if (const char* dd = getenv("SRR_DIGEST_DUMP")) {  // diagnostics: each table to <prefix>.<part>
      FILE* df = fopen((std::string(dd) + "." + std::to_string(part)).c_str(), "wb");
      if (df) { fwrite(p, 1, n, df); fclose(df); }
    }
    if (parts) {
      uint64_t x = 0xcbf29ce484222325ULL;
      mix(x, p, n);
      parts[part] = x;
    }
    ++part;
  };
  auto vec = [&blob](const auto& v) { blob(v.data(), v.size() * sizeof(v[0])); };
  vec(f.objs);
  blob(&f.n_world, sizeof f.n_world);
  vec(f.xforms);
  vec(f.spheres);
  vec(f.rects);
  vec(f.stris);
  vec(f.meshes);
  vec(f.nodes);
  vec(f.node4);
  vec(f.tri_pos);
  vec(f.tri_shade);
  vec(f.media);
  {  // object BVHs, with the sphere groups and their items (device_scene.h DSGroup) in the same part
    std::vector<uint8_t> b;
    auto put = [&b](const void* p, size_t n) { b.insert(b.end(), (const uint8_t*)p, (const uint8_t*)p + n); };
    put(f.obvhs.data(), f.obvhs.size() * sizeof(DObvh));
    put(f.sgroups.data(), f.sgroups.size() * sizeof(DSGroup));
    put(f.sg_items.data(), f.sg_items.size() * sizeof(DSGItem));
    vec(b);
  }
  vec(f.obvh_children);
  vec(f.mats);
  vec(f.texs);
  vec(f.images);
  vec(f.perlin_ranvec);
  vec(f.perlin_perm);
  vec(f.lights);
  blob(&f.cam, sizeof f.cam);
  *out = h;
  return 0;
}

int srr_scene_set_lcg(srr_scene* s, uint64_t state) {
  if (!s) return fail(SRR_EINVAL, "null scene");
  s->s.lcg = state & 0xFFFFFFFFFFFFULL;
  return 0;
}
uint64_t srr_scene_get_lcg(const srr_scene* s) { return s ? s->s.lcg : 0; }
double srr_scene_drand48(srr_scene* s) { return s ? s->s.drand48() : 0.0; }

#define SCN(s) \
  if (!(s)) return fail(SRR_EINVAL, "null scene");
#define TEXOK(s, t) \
  if (!(s)->s.valid_tex(t)) return fail(SRR_EINVAL, "bad texture handle " + std::to_string(t));
#define MATOK(s, m) \
  if (!(s)->s.valid_mat(m)) return fail(SRR_EINVAL, "bad material handle " + std::to_string(m));
#define OBJOK(s, o) \
  if (!(s)->s.valid_obj(o)) return fail(SRR_EINVAL, "bad hitable handle " + std::to_string(o));

int srr_constant_texture(srr_scene* s, float r, float g, float b) {
  SCN(s);
  HTex t;
  t.kind = TEX_CONST;
  t.c[0] = r; t.c[1] = g; t.c[2] = b;
  return s->s.add_tex(std::move(t));
}
int srr_image_texture(srr_scene* s, const unsigned char* rgb, int nx, int ny) {
  SCN(s);
  if (!rgb || nx <= 0 || ny <= 0) return fail(SRR_EINVAL, "bad image");
  HTex t;
  t.kind = TEX_IMAGE;
  t.nx = nx;
  t.ny = ny;
  t.px.assign(rgb, rgb + (size_t)nx * ny * 3);
  return s->s.add_tex(std::move(t));
}
int srr_image_texture_file(srr_scene* s, const char* path) {
  SCN(s);
  if (!path) return fail(SRR_EINVAL, "null path");
  srr::Image im;
  std::string err;
  if (srr::load_image(path, 0, im, err) < 0) return fail(SRR_EIO, err);
  // image_texture reads 3 bytes per texel from the buffer stbi_load returned,
  // whatever its channel count (texture.h:58-70): keep exactly the
  // bytes it can address.  Fewer than 3 channels would read past that buffer.
  if (im.n < 3) return fail(SRR_EINVAL, std::string(path) + ": image_texture needs 3 or 4 channels");
  HTex t;
  t.kind = TEX_IMAGE;
  t.nx = im.w;
  t.ny = im.h;
  t.px.assign(im.px.begin(), im.px.begin() + (size_t)im.w * im.h * 3);
  return s->s.add_tex(std::move(t));
}
int srr_image_texture_gen(srr_scene* s, int nx, int ny, uint32_t seed, int kind) {
  SCN(s);
  if (nx <= 0 || ny <= 0 || kind < 0 || kind > 2) return fail(SRR_EINVAL, "bad image_gen");
  HTex t;
  t.kind = TEX_IMAGE;
  t.nx = nx;
  t.ny = ny;
  t.px = gen_image(nx, ny, seed, kind);
  return s->s.add_tex(std::move(t));
}
int srr_checker_texture(srr_scene* s, int even, int odd) {
  SCN(s);
  TEXOK(s, even);
  TEXOK(s, odd);
  HTex t;
  t.kind = TEX_CHECKER;
  t.even = even;
  t.odd = odd;
  return s->s.add_tex(std::move(t));
}
int srr_noise_texture(srr_scene* s, float scale) {
  SCN(s);
  HTex t;
  t.kind = TEX_NOISE;
  t.c[0] = scale;
  return s->s.add_tex(std::move(t));
}

static int mat_with_tex(srr_scene* s, MatKind k, int tex, float a = 0, float b = 0) {
  SCN(s);
  TEXOK(s, tex);
  float p[4] = {a, b, 0, 0};
  return s->s.material(k, tex, p);
}
int srr_lambertian(srr_scene* s, int t) { return mat_with_tex(s, MAT_LAMBERTIAN, t); }
int srr_orennayar(srr_scene* s, int t, float sigma) { return mat_with_tex(s, MAT_ORENNAYAR, t, sigma); }
int srr_beckmann(srr_scene* s, int t, float rx, float ry) { return mat_with_tex(s, MAT_BECKMANN, t, rx, ry); }
int srr_diffuse_light(srr_scene* s, int t) { return mat_with_tex(s, MAT_DIFFUSE_LIGHT, t); }
int srr_isotropic(srr_scene* s, int t) { return mat_with_tex(s, MAT_ISOTROPIC, t); }
int srr_metal(srr_scene* s, float r, float g, float b, float fuzz) {
  SCN(s);
  float p[4] = {r, g, b, fuzz};
  return s->s.material(MAT_METAL, -1, p);
}
int srr_dielectric(srr_scene* s, float ri) {
  SCN(s);
  float p[4] = {ri, 0, 0, 0};
  return s->s.material(MAT_DIELECTRIC, -1, p);
}

int srr_sphere(srr_scene* s, const float c[3], float r, int m) {
  SCN(s);
  MATOK(s, m);
  return s->s.sphere(c, r, m);
}
int srr_moving_sphere(srr_scene* s, const float c0[3], const float c1[3], float t0, float t1, float r, int m) {
  SCN(s);
  MATOK(s, m);
  return s->s.moving_sphere(c0, c1, t0, t1, r, m);
}
int srr_xy_rect(srr_scene* s, float x0, float x1, float y0, float y1, float k, int m) {
  SCN(s);
  MATOK(s, m);
  return s->s.rect(H_XY, x0, x1, y0, y1, k, m);
}
int srr_xz_rect(srr_scene* s, float x0, float x1, float z0, float z1, float k, int m) {
  SCN(s);
  MATOK(s, m);
  return s->s.rect(H_XZ, x0, x1, z0, z1, k, m);
}
int srr_yz_rect(srr_scene* s, float y0, float y1, float z0, float z1, float k, int m) {
  SCN(s);
  MATOK(s, m);
  return s->s.rect(H_YZ, y0, y1, z0, z1, k, m);
}
int srr_box(srr_scene* s, const float p0[3], const float p1[3], int m) {
  SCN(s);
  MATOK(s, m);
  return s->s.box(p0, p1, m);
}
int srr_triangle(srr_scene* s, const float p[9], int m, const float* uv9, const float* n9) {
  SCN(s);
  MATOK(s, m);
  if (!p) return fail(SRR_EINVAL, "null vertices");
  return s->s.triangle(p, m, uv9, n9);
}
int srr_flip_normals(srr_scene* s, int c) {
  SCN(s);
  OBJOK(s, c);
  return s->s.wrap(H_FLIP, c, nullptr);
}
int srr_translate(srr_scene* s, int c, const float off[3]) {
  SCN(s);
  OBJOK(s, c);
  return s->s.wrap(H_TRANSLATE, c, off);
}
int srr_rotate_y(srr_scene* s, int c, float a) {
  SCN(s);
  OBJOK(s, c);
  return s->s.rotate(H_ROTY, c, a);
}
int srr_rotate_x(srr_scene* s, int c, float a) {
  SCN(s);
  OBJOK(s, c);
  return s->s.rotate(H_ROTX, c, a);
}
int srr_constant_medium(srr_scene* s, int b, float density, int tex) {
  SCN(s);
  OBJOK(s, b);
  TEXOK(s, tex);
  return s->s.medium(b, density, tex);
}
int srr_hitable_list(srr_scene* s, const int* kids, int n) {
  SCN(s);
  if (n < 0 || (n > 0 && !kids)) return fail(SRR_EINVAL, "bad list");
  for (int i = 0; i < n; ++i) OBJOK(s, kids[i]);
  return s->s.list(kids, n);
}
int srr_bvh_node(srr_scene* s, const int* kids, int n, float t0, float t1) {
  SCN(s);
  if (n < 1 || !kids) return fail(SRR_EINVAL, "bvh_node needs n >= 1 children");
  for (int i = 0; i < n; ++i) OBJOK(s, kids[i]);
  return s->s.bvh(kids, n, t0, t1);
}
int srr_teapot(srr_scene* s, float scale, int divs, int m, int* first) {
  SCN(s);
  MATOK(s, m);
  if (divs < 1 || divs > 400) return fail(SRR_EINVAL, "teapot divs out of range");
  return s->s.teapot(scale, divs, m, first);
}
int srr_camera(srr_scene* s, const float lf[3], const float la[3], const float vup[3], float vfov, float aspect,
               float aperture, float focus, float t0, float t1) {
  SCN(s);
  s->s.camera(lf, la, vup, vfov, aspect, aperture, focus, t0, t1);
  return 0;
}
int srr_scene_set_world(srr_scene* s, int o) {
  SCN(s);
  OBJOK(s, o);
  s->s.world = o;
  return 0;
}
int srr_scene_set_lights(srr_scene* s, int o) {
  SCN(s);
  OBJOK(s, o);
  if (s->s.obj[o].kind != H_LIST) return fail(SRR_EINVAL, "lights must be a hitable_list (Raytracing_n.cpp:75)");
  s->s.lights = o;
  return 0;
}

// --------------------------------------------------------------- renderer
int srr_renderer_create(const srr_scene* sc, int device, srr_renderer** out) {
  if (!sc || !out) return fail(SRR_EINVAL, "null argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SRR_ENODEV, "no HIP device (the srr renderer has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(SRR_ENODEV, "device index out of range");
  std::string err;
  int rc = renderer_create(sc->s, device, out, err);
  if (rc < 0) return fail(rc, err);
  return 0;
}

void srr_renderer_destroy(srr_renderer* r) { delete r; }

int srr_renderer_create_multi(const srr_scene* sc, int n, const int* ids, srr_renderer** out) {
  if (!sc || !out || !ids) return fail(SRR_EINVAL, "null argument");
  std::string err;
  int rc = multi_create(sc->s, n, ids, out, err);
  if (rc < 0) return fail(rc, err);
  return 0;
}

int srr_renderer_devices(const srr_renderer* r, int* ids, int cap) {
  if (!r) return fail(SRR_EINVAL, "null renderer");
  if (r->multi) return multi_devices(r->multi, ids, cap);
  if (ids && cap > 0) ids[0] = r->device;
  return 1;
}

const char* srr_renderer_transport(const srr_renderer* r) {
  return !r ? "" : r->multi ? multi_transport(r->multi) : "none";
}

int64_t srr_multi_plan(const srr_params* p, int n, int32_t* index, int64_t* off) {
  std::string err;
  const int64_t rc = multi_plan(p, n, nullptr, index, off, err);
  if (rc < 0) return fail((int)rc, err);
  return rc;
}

int64_t srr_shard_pixels(const srr_params* p, int32_t* out) {
  if (!p || p->nx <= 0 || p->ny <= 0 || p->shard_count < 1 || p->shard_index < 0 ||
      p->shard_index >= p->shard_count)
    return fail(SRR_EINVAL, "bad params");
  // shard tiles round-robin, each tile row rotated by one: tile
  // t = tr * tiles_x + tc (tr = row / tile, tc = col / tile) belongs to shard
  // (t + tr) % shard_count.  Without the rotation a frame tiles_x tiles wide splits
  // into whole tile columns whenever shard_count divides tiles_x (C2 at 8 GPUs:
  // rank k renders columns k and k + 8, 4.7 % above the mean in world rays; with it
  // 1.4 %).  Pixels in PPM order within the shard, emitted row by row as runs of a
  // tile's columns.
  const int tile = p->shard_count == 1 ? p->nx : (p->tile > 0 ? p->tile : 32);
  const int tiles_x = (p->nx + tile - 1) / tile;
  int64_t n = 0;
  for (int row = 0; row < p->ny; ++row) {
    const int tr = row / tile, t0 = tr * tiles_x + tr;
    for (int tc = 0; tc < tiles_x; ++tc) {
      if ((t0 + tc) % p->shard_count != p->shard_index) continue;
      const int c1 = std::min(p->nx, (tc + 1) * tile);
      for (int col = tc * tile; col < c1; ++col) {
        if (out) out[n] = row * p->nx + col;
        ++n;
      }
    }
  }
  return n;
}

int srr_render_device(srr_renderer* r, const srr_params* p, float* d_mean, srr_stats* stats) {
  if (!r || !p || !d_mean) return fail(SRR_EINVAL, "null argument");
  if (p->spp < 1 || p->max_depth < 0 || p->max_depth > 64) return fail(SRR_EINVAL, "spp >= 1, 0 <= max_depth <= 64");
  if (p->sample_begin < 0 || p->sample_begin > INT32_MAX - p->spp)
    return fail(SRR_EINVAL, "sample_begin must be >= 0 and sample_begin + spp must fit in int32");
  if (r->multi) {
    std::string err;
    const int rc = multi_render_device(r, p, d_mean, stats, err);
    return rc < 0 ? fail(rc, err) : 0;
  }
  // the shard's pixel list is built and uploaded once per shard (srr_renderer::pix_key)
  const int key[5] = {p->nx, p->ny, p->shard_index, p->shard_count, p->tile};
  const bool held = std::equal(key, key + 5, r->pix_key);
  int64_t npix = held ? r->pix_n : srr_shard_pixels(p, nullptr);
  if (npix < 0) return (int)npix;
  std::vector<int32_t> pix;
  if (!held) {
    pix.resize(npix);
    srr_shard_pixels(p, pix.data());
  }
  // a new list overwrites the held one before anything can fail: forget its key
  // until the render succeeds (a failed call must not leave the old shard "held")
  if (!held) r->pix_key[0] = -1;
  std::string err;
  int rc = render_device(r, p, held ? nullptr : pix.data(), npix, d_mean, stats, err);
  if (rc < 0) return fail(rc, err);
  if (!held) {
    std::copy(key, key + 5, r->pix_key);
    r->pix_n = npix;
  }
  return 0;
}

int srr_render_device_async(srr_renderer* r, const srr_params* p, float* d_mean, int64_t* ticket) {
  if (!r || !p || !d_mean || !ticket) return fail(SRR_EINVAL, "null argument");
  if (p->spp < 1 || p->max_depth < 0 || p->max_depth > 64) return fail(SRR_EINVAL, "spp >= 1, 0 <= max_depth <= 64");
  if (p->sample_begin < 0 || p->sample_begin > INT32_MAX - p->spp)
    return fail(SRR_EINVAL, "sample_begin must be >= 0 and sample_begin + spp must fit in int32");
  if (r->multi) {
    std::string err;
    const int rc = multi_render_device_async(r, p, d_mean, ticket, err);
    return rc < 0 ? fail(rc, err) : 0;
  }
  const int key[5] = {p->nx, p->ny, p->shard_index, p->shard_count, p->tile};
  const bool held = std::equal(key, key + 5, r->pix_key);
  int64_t npix = held ? r->pix_n : srr_shard_pixels(p, nullptr);
  if (npix < 0) return (int)npix;
  std::vector<int32_t> pix;
  if (!held) {
    pix.resize(npix);
    srr_shard_pixels(p, pix.data());
  }
  // a new list overwrites the held one before anything can fail: forget its key
  // until the render succeeds (a failed call must not leave the old shard "held")
  if (!held) r->pix_key[0] = -1;
  std::string err;
  int rc = render_device_async(r, p, held ? nullptr : pix.data(), npix, d_mean, ticket, err);
  if (rc < 0) return fail(rc, err);
  if (!held) {
    std::copy(key, key + 5, r->pix_key);
    r->pix_n = npix;
  }
  return 0;
}

// srr_render_adaptive (resume = false) and srr_render_adaptive_resume
static int render_adaptive_entry(srr_renderer* r, const srr_params* p, const srr_adaptive_params* a, float* d_mean,
                                 int32_t* d_count, srr_adaptive_stats* stats, bool resume) {
  if (!r || !p || !a || !d_mean) return fail(SRR_EINVAL, "null argument");
  // every refusal comes before anything is staged or enqueued
  if (a->struct_size < sizeof(srr_adaptive_params))
    return fail(SRR_EINVAL, "srr_adaptive_params.struct_size " + std::to_string(a->struct_size) +
                                " is smaller than the " + std::to_string(sizeof(srr_adaptive_params)) +
                                " bytes this library reads");
  if (stats && stats->struct_size < sizeof(srr_adaptive_stats))
    return fail(SRR_EINVAL, "srr_adaptive_stats.struct_size " + std::to_string(stats->struct_size) +
                                " is smaller than the " + std::to_string(sizeof(srr_adaptive_stats)) +
                                " bytes this library writes");
  if (r->multi) return fail(SRR_EINVAL, "srr_render_adaptive: one-device renderers only");
  if (p->flags & (SRR_FLAG_CONTINUE | SRR_FLAG_KEEP_PATHS | SRR_FLAG_COUNT_VISITS | SRR_FLAG_WAVEFRONT | SRR_FLAG_SUMS))
    return fail(SRR_EINVAL, "srr_render_adaptive: fresh path-engine frames only (no CONTINUE, KEEP_PATHS, "
                            "COUNT_VISITS, WAVEFRONT, SUMS)");
  if (p->spp < 1 || p->max_depth < 0 || p->max_depth > 64) return fail(SRR_EINVAL, "spp >= 1, 0 <= max_depth <= 64");
  if (p->sample_begin != 0) return fail(SRR_EINVAL, "srr_render_adaptive: sample_begin must be 0");
  if (a->batch_spp < 1 || a->min_spp < 1) return fail(SRR_EINVAL, "srr_render_adaptive: batch_spp >= 1, min_spp >= 1");
  if (!(a->rel_tol >= 0.f) || !(a->abs_eps >= 0.f))  // (NaN fails both comparisons)
    return fail(SRR_EINVAL, "srr_render_adaptive: rel_tol and abs_eps must be >= 0");
  // the shard's pixel list is built and uploaded once per shard, as in srr_render_device
  const int key[5] = {p->nx, p->ny, p->shard_index, p->shard_count, p->tile};
  if (resume) {
    const AdaptiveState& A = r->adaptive;
    if (A.valid_npix <= 0)
      return fail(SRR_EINVAL, "srr_render_adaptive_resume: the renderer holds no adaptive state (a successful "
                              "srr_render_adaptive, resume or srr_adaptive_state_set must come first)");
    if (!A.sums_valid)
      return fail(SRR_EINVAL, "srr_render_adaptive_resume: the state's rgb sums have been overwritten since (by a "
                              "synchronous render or srr_accum_set)");
    if (!std::equal(key, key + 5, A.key))
      return fail(SRR_EINVAL, "srr_render_adaptive_resume: the adaptive state belongs to another frame or shard");
  }
  const bool held = std::equal(key, key + 5, r->pix_key);
  int64_t npix = held ? r->pix_n : srr_shard_pixels(p, nullptr);
  if (npix < 0) return (int)npix;
  if (resume && npix != r->adaptive.valid_npix)
    return fail(SRR_EINVAL, "srr_render_adaptive_resume: the adaptive state belongs to another frame or shard");
  if (npix == 0) {  // a shard without pixels: no pass
    if (stats) {
      const uint32_t size = stats->struct_size;
      *stats = srr_adaptive_stats{};
      stats->struct_size = size;
    }
    return 0;
  }
  std::vector<int32_t> pix;
  if (!held) {
    pix.resize(npix);
    srr_shard_pixels(p, pix.data());
    r->pix_key[0] = -1;  // forgotten until the render succeeds
  }
  std::string err;
  int rc = render_adaptive(r, p, a, held ? nullptr : pix.data(), npix, d_mean, d_count, stats, resume, err);
  if (rc < 0) return fail(rc, err);
  if (!held) {
    std::copy(key, key + 5, r->pix_key);
    r->pix_n = npix;
  }
  return 0;
}

int srr_render_adaptive(srr_renderer* r, const srr_params* p, const srr_adaptive_params* a, float* d_mean,
                        int32_t* d_count, srr_adaptive_stats* stats) {
  return render_adaptive_entry(r, p, a, d_mean, d_count, stats, false);
}

int srr_render_adaptive_resume(srr_renderer* r, const srr_params* p, const srr_adaptive_params* a, float* d_mean,
                               int32_t* d_count, srr_adaptive_stats* stats) {
  return render_adaptive_entry(r, p, a, d_mean, d_count, stats, true);
}

static int render_adaptive_host_entry(srr_renderer* r, const srr_params* p, const srr_adaptive_params* a, float* mean,
                                      int32_t* count, unsigned char* rgb8, srr_adaptive_stats* stats, bool resume) {
  if (!r || !p || !a) return fail(SRR_EINVAL, "null argument");
  if (r->multi) return fail(SRR_EINVAL, "srr_render_adaptive: one-device renderers only");
  const int64_t npix = srr_shard_pixels(p, nullptr);
  if (npix < 0) return (int)npix;
  DeviceMem<float> d;  // (neither is null for a shard without pixels)
  DeviceMem<int32_t> dc;
  HIPCHK(hipSetDevice(r->device));
  MEMCHK(d.grow(at_least_16_bytes<float>(3 * npix)), SRR_EIO, "adaptive staging image");
  MEMCHK(dc.grow(at_least_16_bytes<int32_t>(npix)), SRR_ENOMEM, "adaptive count buffer");
  int rc = render_adaptive_entry(r, p, a, d.get(), dc.get(), stats, resume);
  std::vector<float> h(3 * npix);
  if (rc == 0) {
    hipError_t e = hipMemcpy(h.data(), d.get(), h.size() * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && count) e = hipMemcpy(count, dc.get(), npix * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(SRR_EIO, hipGetErrorString(e));
  }
  if (rc < 0) return rc;
  if (mean) std::memcpy(mean, h.data(), h.size() * sizeof(float));
  if (rgb8) srr_tonemap(h.data(), npix, rgb8);
  return 0;
}

int srr_render_adaptive_host(srr_renderer* r, const srr_params* p, const srr_adaptive_params* a, float* mean,
                             int32_t* count, unsigned char* rgb8, srr_adaptive_stats* stats) {
  return render_adaptive_host_entry(r, p, a, mean, count, rgb8, stats, false);
}

int srr_render_adaptive_resume_host(srr_renderer* r, const srr_params* p, const srr_adaptive_params* a, float* mean,
                                    int32_t* count, unsigned char* rgb8, srr_adaptive_stats* stats) {
  return render_adaptive_host_entry(r, p, a, mean, count, rgb8, stats, true);
}

int srr_adaptive_state_get(srr_renderer* r, float* sums, float* mom, int32_t* count, int64_t* npix) {
  if (!r) return fail(SRR_EINVAL, "null renderer");
  if (r->multi) return fail(SRR_EINVAL, "srr_adaptive_state_get: one-device renderers only");
  const AdaptiveState& A = r->adaptive;
  if (A.valid_npix <= 0) return fail(SRR_EINVAL, "srr_adaptive_state_get: the renderer holds no adaptive state");
  if (sums && !A.sums_valid)
    return fail(SRR_EINVAL, "srr_adaptive_state_get: the state's rgb sums have been overwritten since (by a "
                            "synchronous render or srr_accum_set)");
  if (npix) *npix = A.valid_npix;
  std::string err;
  const int rc = adaptive_state_get(r, sums, mom, count, err);
  return rc < 0 ? fail(rc, err) : 0;
}

int srr_adaptive_state_set(srr_renderer* r, const srr_params* p, const float* sums, const float* mom,
                           const int32_t* count, int64_t npix) {
  if (!r || !p || !sums || !mom || !count) return fail(SRR_EINVAL, "null argument");
  if (r->multi) return fail(SRR_EINVAL, "srr_adaptive_state_set: one-device renderers only");
  const int64_t want = srr_shard_pixels(p, nullptr);
  if (want < 0) return (int)want;
  if (npix <= 0 || npix != want)
    return fail(SRR_EINVAL, "srr_adaptive_state_set: npix " + std::to_string(npix) + " is not the frame's " +
                                std::to_string(want) + " shard pixels");
  for (int64_t i = 0; i < npix; ++i)
    if (count[i] < 0)
      return fail(SRR_EINVAL, "srr_adaptive_state_set: count[" + std::to_string(i) + "] is negative");
  std::string err;
  const int rc = adaptive_state_set(r, p, sums, mom, count, npix, err);
  return rc < 0 ? fail(rc, err) : 0;
}

int srr_adaptive_converged(int32_t n, float s1, float s2, float rel_tol, float abs_eps) {
  return adaptive_converged_host(n, s1, s2, rel_tol, abs_eps);
}

int srr_adaptive_speculate(srr_renderer* r, int pass_spp_max, int64_t fill_paths) {
  if (!r) return fail(SRR_EINVAL, "null renderer");
  if (r->multi) return fail(SRR_EINVAL, "srr_adaptive_speculate: one-device renderers only");
  if (pass_spp_max < 0 || fill_paths < 0)
    return fail(SRR_EINVAL, "srr_adaptive_speculate: pass_spp_max >= 0, fill_paths >= 0");
  r->adaptive.pass_spp_max = pass_spp_max;
  r->adaptive.fill_paths = fill_paths;
  return 0;
}

int srr_adaptive_last_spec_stats(const srr_renderer* r, srr_adaptive_spec_stats* out) {
  if (!r || !out) return fail(SRR_EINVAL, "null argument");
  if (out->struct_size < sizeof(srr_adaptive_spec_stats))
    return fail(SRR_EINVAL, "srr_adaptive_spec_stats.struct_size " + std::to_string(out->struct_size) +
                                " is smaller than the " + std::to_string(sizeof(srr_adaptive_spec_stats)) +
                                " bytes this library writes");
  if (r->multi) return fail(SRR_EINVAL, "srr_adaptive_last_spec_stats: one-device renderers only");
  const AdaptiveState& A = r->adaptive;
  if (A.spec_windows < 0)
    return fail(SRR_EINVAL, "srr_adaptive_last_spec_stats: no adaptive call has succeeded on this renderer yet");
  out->windows = A.spec_windows;
  out->paths_traced = A.spec_traced;
  out->paths_discarded = A.spec_discarded;
  return 0;
}

int srr_adaptive_pass_width(int64_t n_active, int n, int budget, int batch_spp, int pass_spp_max,
                            int64_t fill_paths) {
  const int w = adaptive_pass_width(n_active, n, budget, batch_spp, pass_spp_max, fill_paths);
  if (w < 0)
    return fail(SRR_EINVAL, "srr_adaptive_pass_width: n_active >= 1, 0 <= n < budget, batch_spp >= 1, "
                            "pass_spp_max >= 0, fill_paths >= 0");
  return w;
}

int64_t srr_adaptive_fill_default(void) { return kAdaptiveFillDefault; }

float srr_variance_of_mean(int32_t n, float s1, float s2) { return variance_of_mean_host(n, s1, s2); }

static int adaptive_variance_check(const srr_renderer* r, const void* count, const void* var) {
  if (!r || !count || !var) return fail(SRR_EINVAL, "null argument");
  if (r->multi) return fail(SRR_EINVAL, "srr_adaptive_variance: one-device renderers only");
  if (r->adaptive.valid_npix <= 0)
    return fail(SRR_EINVAL, "srr_adaptive_variance: the renderer holds no adaptive frame's moments (the most recent "
                            "srr_render_adaptive, resume or srr_adaptive_state_set must have succeeded)");
  return 0;
}

int srr_adaptive_variance(srr_renderer* r, const int32_t* d_count, float* d_var) {
  // every refusal comes before anything is enqueued
  if (const int rc = adaptive_variance_check(r, d_count, d_var)) return rc;
  std::string err;
  const int rc = adaptive_variance(r, d_count, d_var, err);
  return rc < 0 ? fail(rc, err) : 0;
}

int srr_adaptive_variance_host(srr_renderer* r, const int32_t* count, float* var) {
  if (const int rc = adaptive_variance_check(r, count, var)) return rc;
  const size_t npix = (size_t)r->adaptive.valid_npix;
  DeviceMem<int32_t> dc;
  DeviceMem<float> dv;
  HIPCHK(hipSetDevice(r->device));
  MEMCHK(dc.grow(at_least_16_bytes<int32_t>(npix)), SRR_ENOMEM, "adaptive count buffer");
  MEMCHK(dv.grow(at_least_16_bytes<float>(npix)), SRR_ENOMEM, "adaptive variance buffer");
  hipError_t e = hipMemcpy(dc.get(), count, npix * sizeof(int32_t), hipMemcpyHostToDevice);
  int rc = e == hipSuccess ? srr_adaptive_variance(r, dc.get(), dv.get()) : fail(SRR_EIO, hipGetErrorString(e));
  if (rc == 0) {
    e = hipMemcpy(var, dv.get(), npix * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(SRR_EIO, hipGetErrorString(e));
  }
  return rc;
}

// ---- first-hit AOVs
static int aov_check(const srr_renderer* r, const srr_params* p, int which, const void* a, const void* n,
                     const void* z) {
  if (!r || !p) return fail(SRR_EINVAL, "null argument");
  if (r->multi) return fail(SRR_EINVAL, "srr_render_aov: one-device renderers only");
  if (p->flags & (SRR_FLAG_CONTINUE | SRR_FLAG_KEEP_PATHS | SRR_FLAG_COUNT_VISITS | SRR_FLAG_SUMS))
    return fail(SRR_EINVAL, "srr_render_aov: no CONTINUE, KEEP_PATHS, COUNT_VISITS, SUMS");
  if (which == 0 || (which & ~(SRR_AOV_ALBEDO | SRR_AOV_NORMAL | SRR_AOV_DEPTH)))
    return fail(SRR_EINVAL, "srr_render_aov: which must be a non-empty set of SRR_AOV_* bits");
  if (((which & SRR_AOV_ALBEDO) && !a) || ((which & SRR_AOV_NORMAL) && !n) || ((which & SRR_AOV_DEPTH) && !z))
    return fail(SRR_EINVAL, "srr_render_aov: a buffer selected in `which` is NULL");
  if (p->spp < 1 || p->max_depth < 0 || p->max_depth > 64) return fail(SRR_EINVAL, "spp >= 1, 0 <= max_depth <= 64");
  if (p->sample_begin < 0 || p->sample_begin > INT32_MAX - p->spp)
    return fail(SRR_EINVAL, "sample_begin must be >= 0 and sample_begin + spp must fit in int32");
  if (p->batch_paths < 0) return fail(SRR_EINVAL, "batch_paths must be >= 0");
  return 0;
}

int srr_render_aov(srr_renderer* r, const srr_params* p, int which, float* d_albedo, float* d_normal,
                   float* d_depth) {
  // every refusal comes before anything is allocated or enqueued
  if (const int rc = aov_check(r, p, which, d_albedo, d_normal, d_depth)) return rc;
  const int64_t npix = srr_shard_pixels(p, nullptr);
  if (npix < 0) return (int)npix;
  if (npix == 0) return 0;
  std::vector<int32_t> pix(npix);
  srr_shard_pixels(p, pix.data());
  std::string err;
  const int rc = render_aov(r, p, pix.data(), npix, (which & SRR_AOV_ALBEDO) ? d_albedo : nullptr,
                            (which & SRR_AOV_NORMAL) ? d_normal : nullptr, (which & SRR_AOV_DEPTH) ? d_depth : nullptr,
                            err);
  return rc < 0 ? fail(rc, err) : 0;
}

// the staged images d = albedo [3 npix], normal [3 npix], depth [npix] to the host buffers asked for
static int aov_copy_out(int which, const float* d, int64_t npix, float* albedo, float* normal, float* depth) {
  hipError_t e = hipSuccess;
  if (which & SRR_AOV_ALBEDO) e = hipMemcpy(albedo, d, 3 * npix * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess && (which & SRR_AOV_NORMAL))
    e = hipMemcpy(normal, d + 3 * npix, 3 * npix * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess && (which & SRR_AOV_DEPTH))
    e = hipMemcpy(depth, d + 6 * npix, npix * sizeof(float), hipMemcpyDeviceToHost);
  return e == hipSuccess ? 0 : fail(SRR_EIO, hipGetErrorString(e));
}

int srr_render_aov_host(srr_renderer* r, const srr_params* p, int which, float* albedo, float* normal, float* depth) {
  if (const int rc = aov_check(r, p, which, albedo, normal, depth)) return rc;
  const int64_t npix = srr_shard_pixels(p, nullptr);
  if (npix < 0) return (int)npix;
  if (npix == 0) return 0;
  DeviceMem<float> buf;  // albedo [3 npix], normal [3 npix], depth [npix]
  HIPCHK(hipSetDevice(r->device));
  MEMCHK(buf.grow(7 * npix), SRR_EIO, "AOV staging images");
  float* const d = buf.get();
  int rc = srr_render_aov(r, p, which, d, d + 3 * npix, d + 6 * npix);
  if (rc == 0) rc = aov_copy_out(which, d, npix, albedo, normal, depth);
  return rc;
}

// ---- through-specular AOVs: srr_render_aov's checks, then the stats struct's
static int aov_through_check(const srr_renderer* r, const srr_params* p, int which, const void* a, const void* n,
                             const void* z, const srr_aov_stats* stats) {
  if (const int rc = aov_check(r, p, which, a, n, z)) return rc;
  if (stats && stats->struct_size < sizeof(srr_aov_stats))
    return fail(SRR_EINVAL, "srr_render_aov_through: stats->struct_size is smaller than srr_aov_stats");
  return 0;
}

int srr_render_aov_through(srr_renderer* r, const srr_params* p, int which, float* d_albedo, float* d_normal,
                           float* d_depth, srr_aov_stats* stats) {
  // every refusal comes before anything is allocated or enqueued
  if (const int rc = aov_through_check(r, p, which, d_albedo, d_normal, d_depth, stats)) return rc;
  const int64_t npix = srr_shard_pixels(p, nullptr);
  if (npix < 0) return (int)npix;
  if (npix == 0) {
    if (stats) *stats = srr_aov_stats{stats->struct_size, 0, 0, 0, 0};
    return 0;
  }
  std::vector<int32_t> pix(npix);
  srr_shard_pixels(p, pix.data());
  std::string err;
  const int rc = render_aov_through(r, p, pix.data(), npix, (which & SRR_AOV_ALBEDO) ? d_albedo : nullptr,
                                    (which & SRR_AOV_NORMAL) ? d_normal : nullptr,
                                    (which & SRR_AOV_DEPTH) ? d_depth : nullptr, stats, err);
  return rc < 0 ? fail(rc, err) : 0;
}

int srr_render_aov_through_host(srr_renderer* r, const srr_params* p, int which, float* albedo, float* normal,
                                float* depth, srr_aov_stats* stats) {
  if (const int rc = aov_through_check(r, p, which, albedo, normal, depth, stats)) return rc;
  const int64_t npix = srr_shard_pixels(p, nullptr);
  if (npix < 0) return (int)npix;
  DeviceMem<float> buf;  // albedo [3 npix], normal [3 npix], depth [npix]
  HIPCHK(hipSetDevice(r->device));
  MEMCHK(buf.grow(7 * npix), SRR_EIO, "AOV staging images");
  float* const d = buf.get();
  int rc = srr_render_aov_through(r, p, which, d, d + 3 * npix, d + 6 * npix, stats);
  if (rc == 0 && npix > 0) rc = aov_copy_out(which, d, npix, albedo, normal, depth);
  return rc;
}

// ---- the emission AOV: the checks of the two calls above on the three old bits, then its own
static int aov_emission_check(const srr_renderer* r, const srr_params* p, int which, int through, const void* a,
                              const void* n, const void* z, const void* e, const srr_aov_stats* stats) {
  if (!r || !p) return fail(SRR_EINVAL, "null argument");
  if (which == 0 || (which & ~(SRR_AOV_ALBEDO | SRR_AOV_NORMAL | SRR_AOV_DEPTH | SRR_AOV_EMISSION)))
    return fail(SRR_EINVAL, "srr_render_aov_emission: which must be a non-empty set of SRR_AOV_* bits");
  if (through != 0 && through != 1) return fail(SRR_EINVAL, "srr_render_aov_emission: through_specular must be 0 or 1");
  if ((which & SRR_AOV_EMISSION) && !e)
    return fail(SRR_EINVAL, "srr_render_aov_emission: a buffer selected in `which` is NULL");
  const int old = which & ~SRR_AOV_EMISSION;
  // (with bit 8 alone the old checks run on a stand-in bit whose buffer is the emission's)
  if (const int rc = aov_through_check(r, p, old ? old : SRR_AOV_ALBEDO, old ? a : e, n, z, stats)) return rc;
  return 0;
}

int srr_render_aov_emission(srr_renderer* r, const srr_params* p, int which, int through_specular, float* d_albedo,
                            float* d_normal, float* d_depth, float* d_emission, const int32_t* d_count,
                            srr_aov_stats* stats) {
  // every refusal comes before anything is allocated or enqueued
  if (const int rc = aov_emission_check(r, p, which, through_specular, d_albedo, d_normal, d_depth, d_emission, stats))
    return rc;
  const int64_t npix = srr_shard_pixels(p, nullptr);
  if (npix < 0) return (int)npix;
  if (npix == 0) {
    if (stats) *stats = srr_aov_stats{stats->struct_size, 0, 0, 0, 0};
    return 0;
  }
  std::vector<int32_t> pix(npix);
  srr_shard_pixels(p, pix.data());
  std::string err;
  const bool em = (which & SRR_AOV_EMISSION) != 0;
  const int rc = render_aov_emission(r, p, pix.data(), npix, through_specular,
                                     (which & SRR_AOV_ALBEDO) ? d_albedo : nullptr,
                                     (which & SRR_AOV_NORMAL) ? d_normal : nullptr,
                                     (which & SRR_AOV_DEPTH) ? d_depth : nullptr, em ? d_emission : nullptr,
                                     em ? d_count : nullptr, stats, err);
  return rc < 0 ? fail(rc, err) : 0;
}

int srr_render_aov_emission_host(srr_renderer* r, const srr_params* p, int which, int through_specular, float* albedo,
                                 float* normal, float* depth, float* emission, const int32_t* count,
                                 srr_aov_stats* stats) {
  if (const int rc = aov_emission_check(r, p, which, through_specular, albedo, normal, depth, emission, stats))
    return rc;
  const int64_t npix = srr_shard_pixels(p, nullptr);
  if (npix < 0) return (int)npix;
  const bool em = (which & SRR_AOV_EMISSION) != 0;
  if (em && count)
    for (int64_t i = 0; i < npix; ++i)
      if (count[i] < 1 || count[i] > p->spp)
        return fail(SRR_EINVAL, "srr_render_aov_emission_host: count[" + std::to_string(i) + "] is outside 1..spp");
  DeviceMem<float> buf;  // albedo [3 npix], normal [3 npix], depth [npix], emission [3 npix]
  DeviceMem<int32_t> dc;
  HIPCHK(hipSetDevice(r->device));
  MEMCHK(buf.grow(10 * npix), SRR_EIO, "AOV staging images");
  float* const d = buf.get();
  if (em && count && npix > 0) {
    MEMCHK(dc.grow(at_least_16_bytes<int32_t>(npix)), SRR_EIO, "AOV staging counts");
    const hipError_t e = hipMemcpy(dc.get(), count, npix * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(SRR_EIO, hipGetErrorString(e));
  }
  int rc = srr_render_aov_emission(r, p, which, through_specular, d, d + 3 * npix, d + 6 * npix, d + 7 * npix,
                                   em && count ? dc.get() : nullptr, stats);
  if (rc == 0 && npix > 0 && (which & ~SRR_AOV_EMISSION))
    rc = aov_copy_out(which, d, npix, albedo, normal, depth);
  if (rc == 0 && npix > 0 && em) {
    const hipError_t e = hipMemcpy(emission, d + 7 * npix, 3 * npix * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(SRR_EIO, hipGetErrorString(e));
  }
  return rc;
}

// ---- the a-trous denoisers (denoise.hip): srr_denoise and srr_denoise_var
extern "C++" {
namespace {
// what tells the two filters' entries apart: the name in their messages, the label of
// their first strength, the kernels' policy
struct DnEntry {
  const char* fn;
  const char* k0;
  AtrousStop stop;
  bool emission = false;
};
const DnEntry kDnColour{"srr_denoise", "k_c", kColourStop}, kDnVar{"srr_denoise_var", "k_l", kVarianceStop};
// the emission-separated entries: the same filters, d_emission required
const DnEntry kDnColourE{"srr_denoise_emission", "k_c", kColourStop, true},
    kDnVarE{"srr_denoise_var_emission", "k_l", kVarianceStop, true};
float dn_k0(const srr_denoise_params& p) { return p.k_c; }
float dn_k0(const srr_denoise_var_params& p) { return p.k_l; }

struct DnBuffers {  // var and var_out: srr_denoise_var only (var_out may be NULL there too)
  const float *color, *var, *albedo, *normal, *depth;
  float *out, *var_out;
  const float* emission = nullptr;  // the _emission entries only
};

struct Image {  // a caller's buffer and, in the _host entries, its part of the staging allocation
  const float* p;
  size_t floats;
  float* dev = nullptr;
};
bool overlap(const Image& a, const Image& b) {
  return (uintptr_t)a.p < (uintptr_t)b.p + b.floats * sizeof(float) &&
         (uintptr_t)b.p < (uintptr_t)a.p + a.floats * sizeof(float);
}

template <class Params>
int denoise_check(const DnEntry& E, int device, int nx, int ny, const Params* dp, const DnBuffers& b) {
  const std::string fn = E.fn;
  if (!dp) return fail(SRR_EINVAL, fn + ": null params");
  if (dp->struct_size < sizeof(Params))
    return fail(SRR_EINVAL, fn + "_params.struct_size " + std::to_string(dp->struct_size) + " is smaller than the " +
                                std::to_string(sizeof(Params)) + " bytes this library reads");
  if (device < 0) return fail(SRR_EINVAL, fn + ": bad device");
  if (nx < 1 || ny < 1 || nx > 65536 || ny > 65536 || (int64_t)nx * ny > ((int64_t)1 << 28))
    return fail(SRR_EINVAL, fn + ": 1 <= nx, ny <= 65536 and nx*ny <= 2^28");
  if (dp->iterations < 1 || dp->iterations > 6) return fail(SRR_EINVAL, fn + ": iterations must be 1..6");
  for (const float k : {dn_k0(*dp), dp->k_n, dp->k_z})
    if (!(k >= 0.f) || !(k <= 3.402823466e38f))  // (NaN fails both comparisons)
      return fail(SRR_EINVAL, fn + ": " + E.k0 + ", k_n, k_z must be finite and >= 0");
  if (dp->flags & ~SRR_DENOISE_DEMODULATE) return fail(SRR_EINVAL, fn + ": unknown flags");
  const bool has_var = E.stop == kVarianceStop;
  if (!b.color || (has_var && !b.var) || !b.albedo || !b.normal || !b.depth || !b.out)
    return fail(SRR_EINVAL, fn + ": null buffer");
  if (E.emission && !b.emission) return fail(SRR_EINVAL, fn + ": null buffer");
  const size_t n = (size_t)nx * ny;
  const Image in[] = {{b.color, 3 * n},  {b.var, n},   {b.albedo, 3 * n},
                      {b.normal, 3 * n}, {b.depth, n}, {b.emission, 3 * n}};
  const Image outs[] = {{b.out, 3 * n}, {b.var_out, n}};
  for (const Image& o : outs)
    for (const Image& i : in)
      if (o.p && i.p && overlap(o, i))
        return fail(SRR_EINVAL, fn + (has_var ? ": an output" : ": the output") + " overlaps an input");
  if (b.var_out && overlap(outs[0], outs[1])) return fail(SRR_EINVAL, fn + ": the outputs overlap each other");
  return 0;
}

int denoise_variant() {  // SRR_DENOISE_VARIANT: measurements only
  static const int variant = [] {
    const char* e = getenv("SRR_DENOISE_VARIANT");
    if (e && !strcmp(e, "tile")) return (int)kDnTile;
    if (e && !strcmp(e, "gather")) return (int)kDnGather;
    return (int)kDnAuto;
  }();
  return variant;
}

// the filters' scratch, kept per device between calls: the two x images that the
// iterations ping-pong and the guides, float4 per pixel each
std::mutex g_dn_mu;
// (never destroyed: at process exit the HIP runtime may be gone before this library's statics)
std::map<int, DeviceMem<float4>>& g_dn_scratch = *new std::map<int, DeviceMem<float4>>;

template <class Params>
int denoise_device(const DnEntry& E, int device, int nx, int ny, const Params* dp, const DnBuffers& b) {
  // every refusal comes before the GPU is touched
  if (const int rc = denoise_check(E, device, nx, ny, dp, b)) return rc;
  const size_t n = (size_t)nx * ny;
  std::lock_guard<std::mutex> lock(g_dn_mu);
  HIPCHK(hipSetDevice(device));
  DeviceMem<float4>& W = g_dn_scratch[device];
  MEMCHK(W.grow(3 * n), SRR_ENOMEM, std::string(E.fn) + ": scratch images");
  float4* x[2] = {W.get(), W.get() + n};
  float4* guide = W.get() + 2 * n;
  const bool demod = (dp->flags & SRR_DENOISE_DEMODULATE) != 0;
  hipStream_t st = nullptr;  // the caller's inputs were written on the legacy stream or are complete
  launch_atrous_pack(E.stop, (int64_t)n, b.color, b.var, b.emission, demod ? b.albedo : nullptr, b.normal, b.depth,
                     x[0], guide, st);
  for (int k = 0; k < dp->iterations; ++k) {
    const bool last = k + 1 == dp->iterations;
    AtrousIter I{};
    I.nx = nx;
    I.ny = ny;
    I.step = 1 << k;
    I.k = E.stop == kColourStop ? dn_k0(*dp) * (float)(1 << (2 * k)) : dn_k0(*dp);
    I.kn = dp->k_n;
    I.kz = dp->k_z;
    I.x_in = x[k & 1];
    I.guide = guide;
    I.x_out = last ? nullptr : x[(k & 1) ^ 1];
    I.out = last ? b.out : nullptr;
    I.var_out = last ? b.var_out : nullptr;
    I.albedo = last && demod ? b.albedo : nullptr;
    I.emission = last ? b.emission : nullptr;
    launch_atrous_iter(E.stop, I, denoise_variant(), st);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// The _host entries: every image that has a host pointer gets its part of one device
// allocation, the first n_in of them are copied there, and the rest are copied back.
template <size_t N>
int stage_in(DeviceMem<float>& buf, const std::string& what, Image (&img)[N], size_t n_in) {
  size_t total = 0;
  for (const Image& i : img) total += i.p ? i.floats : 0;
  MEMCHK(buf.grow(total), SRR_EIO, what);
  float* d = buf.get();
  for (Image& i : img) {
    if (!i.p) continue;
    i.dev = d;
    d += i.floats;
    if (size_t(&i - img) >= n_in) continue;
    const hipError_t e = hipMemcpy(i.dev, i.p, i.floats * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(SRR_EIO, hipGetErrorString(e));
  }
  return 0;
}
template <size_t N>
int stage_out(Image (&img)[N], size_t n_in) {
  for (size_t j = n_in; j < N; ++j) {
    if (!img[j].p) continue;
    const hipError_t e =
        hipMemcpy(const_cast<float*>(img[j].p), img[j].dev, img[j].floats * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(SRR_EIO, hipGetErrorString(e));
  }
  return 0;
}

template <class Params>
int denoise_host(const DnEntry& E, int device, int nx, int ny, const Params* dp, const DnBuffers& h) {
  if (const int rc = denoise_check(E, device, nx, ny, dp, h)) return rc;
  const size_t n = (size_t)nx * ny;
  Image img[] = {{h.color, 3 * n}, {h.var, n},        {h.albedo, 3 * n}, {h.normal, 3 * n},
                 {h.depth, n},     {h.emission, 3 * n}, {h.out, 3 * n},    {h.var_out, n}};
  DeviceMem<float> buf;
  HIPCHK(hipSetDevice(device));
  if (const int rc = stage_in(buf, std::string(E.fn) + "_host: staging images", img, 6)) return rc;
  const int rc = denoise_device(
      E, device, nx, ny, dp,
      {img[0].dev, img[1].dev, img[2].dev, img[3].dev, img[4].dev, img[6].dev, img[7].dev, img[5].dev});
  return rc ? rc : stage_out(img, 6);
}
}  // namespace
}  // extern "C++"

int srr_denoise_defaults(srr_denoise_params* dp) {
  if (!dp) return fail(SRR_EINVAL, "null argument");
  // chosen by the sweep of DESIGN.md §4.2 (profiles/r08/denoise.txt)
  *dp = srr_denoise_params{(uint32_t)sizeof(srr_denoise_params), 3, 256.0f, 32.0f, 64.0f, 0};
  return 0;
}

int srr_denoise_var_defaults(srr_denoise_var_params* dp) {
  if (!dp) return fail(SRR_EINVAL, "null argument");
  // chosen by the sweep of DESIGN.md §4.3 (profiles/r12/denoise_var.txt)
  *dp = srr_denoise_var_params{(uint32_t)sizeof(srr_denoise_var_params), 3, 2.0f, 128.0f, 64.0f,
                               SRR_DENOISE_DEMODULATE};
  return 0;
}

int srr_denoise(int device, int nx, int ny, const srr_denoise_params* dp, const float* d_color,
                const float* d_albedo, const float* d_normal, const float* d_depth, float* d_out) {
  return denoise_device(kDnColour, device, nx, ny, dp, {d_color, nullptr, d_albedo, d_normal, d_depth, d_out, nullptr});
}

int srr_denoise_host(int device, int nx, int ny, const srr_denoise_params* dp, const float* color,
                     const float* albedo, const float* normal, const float* depth, float* out) {
  return denoise_host(kDnColour, device, nx, ny, dp, {color, nullptr, albedo, normal, depth, out, nullptr});
}

int srr_denoise_var(int device, int nx, int ny, const srr_denoise_var_params* dp, const float* d_color,
                    const float* d_var, const float* d_albedo, const float* d_normal, const float* d_depth,
                    float* d_out, float* d_var_out) {
  return denoise_device(kDnVar, device, nx, ny, dp, {d_color, d_var, d_albedo, d_normal, d_depth, d_out, d_var_out});
}

int srr_denoise_var_host(int device, int nx, int ny, const srr_denoise_var_params* dp, const float* color,
                         const float* var, const float* albedo, const float* normal, const float* depth, float* out,
                         float* var_out) {
  return denoise_host(kDnVar, device, nx, ny, dp, {color, var, albedo, normal, depth, out, var_out});
}

int srr_denoise_emission(int device, int nx, int ny, const srr_denoise_params* dp, const float* d_color,
                         const float* d_emission, const float* d_albedo, const float* d_normal, const float* d_depth,
                         float* d_out) {
  return denoise_device(kDnColourE, device, nx, ny, dp,
                        {d_color, nullptr, d_albedo, d_normal, d_depth, d_out, nullptr, d_emission});
}

int srr_denoise_emission_host(int device, int nx, int ny, const srr_denoise_params* dp, const float* color,
                              const float* emission, const float* albedo, const float* normal, const float* depth,
                              float* out) {
  return denoise_host(kDnColourE, device, nx, ny, dp, {color, nullptr, albedo, normal, depth, out, nullptr, emission});
}

int srr_denoise_var_emission(int device, int nx, int ny, const srr_denoise_var_params* dp, const float* d_color,
                             const float* d_var, const float* d_emission, const float* d_albedo,
                             const float* d_normal, const float* d_depth, float* d_out, float* d_var_out) {
  return denoise_device(kDnVarE, device, nx, ny, dp,
                        {d_color, d_var, d_albedo, d_normal, d_depth, d_out, d_var_out, d_emission});
}

int srr_denoise_var_emission_host(int device, int nx, int ny, const srr_denoise_var_params* dp, const float* color,
                                  const float* var, const float* emission, const float* albedo, const float* normal,
                                  const float* depth, float* out, float* var_out) {
  return denoise_host(kDnVarE, device, nx, ny, dp, {color, var, albedo, normal, depth, out, var_out, emission});
}

int srr_render_wait(srr_renderer* r, int64_t ticket, srr_stats* stats) {
  if (!r) return fail(SRR_EINVAL, "null renderer");
  std::string err;
  int rc = r->multi ? multi_render_wait(r, ticket, stats, err) : render_wait(r, ticket, stats, err);
  if (rc < 0) return fail(rc, err);
  return 0;
}

int srr_render(srr_renderer* r, const srr_params* p, float* mean, unsigned char* rgb8, srr_stats* stats) {
  if (!r || !p) return fail(SRR_EINVAL, "null argument");
  if (r->multi && p->shard_count > 1)
    return fail(SRR_EINVAL, "a multi-device renderer shards the frame itself: shard_count must be 0 or 1");
  int64_t npix = r->multi ? (p->nx > 0 && p->ny > 0 ? (int64_t)p->nx * p->ny : -1) : srr_shard_pixels(p, nullptr);
  if (npix < 0 && r->multi) return fail(SRR_EINVAL, "bad params");
  if (npix < 0) return (int)npix;
  DeviceMem<float> d;
  HIPCHK(hipSetDevice(r->device));
  MEMCHK(d.grow(3 * npix), SRR_EIO, "staging image");
  int rc = srr_render_device(r, p, d.get(), stats);
  std::vector<float> h(3 * npix);
  if (rc == 0) {
    hipError_t e = hipMemcpy(h.data(), d.get(), h.size() * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(SRR_EIO, hipGetErrorString(e));
  }
  if (rc < 0) return rc;
  if (mean) std::memcpy(mean, h.data(), h.size() * sizeof(float));
  if (rgb8) srr_tonemap(h.data(), npix, rgb8);
  return 0;
}

int srr_accum_get(srr_renderer* r, float* sums, int64_t* npix, int64_t* samples) {
  if (!r) return fail(SRR_EINVAL, "null renderer");
  if (r && r->multi) return fail(SRR_EINVAL, "progressive sums and kept paths are per device: use a one-device renderer");
  if (npix) *npix = r->acc_npix;
  if (samples) *samples = r->acc_samples;
  if (sums && r->acc_npix) {
    HIPCHK(hipSetDevice(r->device));
    HIPCHK(hipMemcpy(sums, r->acc.get(), 3 * r->acc_npix * sizeof(float), hipMemcpyDeviceToHost));
  }
  return 0;
}

int srr_accum_set(srr_renderer* r, const float* sums, int64_t npix, int64_t samples) {
  if (!r || !sums || npix <= 0 || samples < 0) return fail(SRR_EINVAL, "bad accumulator state");
  if (r && r->multi) return fail(SRR_EINVAL, "progressive sums and kept paths are per device: use a one-device renderer");
  HIPCHK(hipSetDevice(r->device));
  drain_async(r);  // frames in flight read the pixel list this may reallocate
  MEMCHK(ensure_pixels(r, npix), SRR_EIO, "pixel list and running sums");
  r->adaptive.sums_valid = false;  // an adaptive state's rgb sums are overwritten
  HIPCHK(hipMemcpy(r->acc.get(), sums, 3 * npix * sizeof(float), hipMemcpyHostToDevice));
  r->acc_npix = npix;
  r->acc_samples = samples;
  std::fill(r->acc_key, r->acc_key + 5, -1);  // any frame / shard of npix pixels may continue them
  return 0;
}

int srr_copy_paths(srr_renderer* r, float* radiance, unsigned char* rays) {
  if (r && r->multi) return fail(SRR_EINVAL, "progressive sums and kept paths are per device: use a one-device renderer");
  if (!r || !r->raw_all.get()) return fail(SRR_EINVAL, "render with SRR_FLAG_KEEP_PATHS first");
  HIPCHK(hipSetDevice(r->device));
  if (radiance) HIPCHK(hipMemcpy(radiance, r->raw_all.get(), r->kept_paths * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (rays) HIPCHK(hipMemcpy(rays, r->rays_all.get(), r->kept_paths, hipMemcpyDeviceToHost));
  return 0;
}

int srr_tonemap(const float* mean, int64_t n, unsigned char* rgb8) {  // Raytracing_n.cpp:850-862
  if (!mean || !rgb8) return fail(SRR_EINVAL, "null argument");
  for (int64_t i = 0; i < 3 * n; ++i) {
    float c = std::sqrt(mean[i]);
    int q = int(255.99 * c);
    q = q > 255 ? 255 : q;
    q = q < 0 ? 0 : q;
    rgb8[i] = (unsigned char)q;
  }
  return 0;
}

int srr_mesh_file_triangles(const char* path, int flip_uvs, int flip_winding, const float scale[3], float* pos9,
                            float* uv9, float* nrm9, int* flags_out) {
  if (!path || !scale) return fail(SRR_EINVAL, "null argument");
  srr::MeshData m;
  std::string err;
  if (srr::load_mesh_file(path, m, err) < 0) return fail(SRR_EIO, err);
  srr::apply_model_semantics(m, flip_uvs != 0, flip_winding != 0, scale);
  for (size_t t = 0; t < m.tris.size(); ++t)
    for (int j = 0; j < 3; ++j) {
      const srr::MeshData::Corner& c = m.tris[t][j];
      if (pos9) std::memcpy(pos9 + 9 * t + 3 * j, c.p, 12);
      if (uv9) std::memcpy(uv9 + 9 * t + 3 * j, c.uv, 12);
      if (nrm9) std::memcpy(nrm9 + 9 * t + 3 * j, c.n, 12);
    }
  if (flags_out) *flags_out = (m.has_normals ? 1 : 0) | (m.has_uvs ? 2 : 0);
  if (m.tris.size() > (size_t)INT32_MAX / 2) return fail(SRR_EINVAL, "mesh too large");
  return (int)m.tris.size();
}

int srr_model(srr_scene* s, const char* path, int flip_uvs, int flip_winding, int mat, const float scale[3],
              int* first_handle) {
  if (!s || !path || !scale) return fail(SRR_EINVAL, "null argument");
  srr::MeshData m;
  std::string err;
  if (srr::load_mesh_file(path, m, err) < 0) return fail(SRR_EIO, err);
  srr::apply_model_semantics(m, flip_uvs != 0, flip_winding != 0, scale);
  if (m.tris.empty()) return fail(SRR_EINVAL, std::string(path) + ": mesh 0 has no triangles");
  int first = -1;
  for (const auto& t : m.tris) {
    float p[9], uv[9], n[9];
    for (int j = 0; j < 3; ++j) {
      std::memcpy(p + 3 * j, t[j].p, 12);
      std::memcpy(uv + 3 * j, t[j].uv, 12);
      std::memcpy(n + 3 * j, t[j].n, 12);
    }
    int h = srr_triangle(s, p, mat, uv, m.has_normals ? n : nullptr);
    if (h < 0) return h;
    if (first < 0) first = h;
  }
  if (first_handle) *first_handle = first;
  return (int)m.tris.size();
}

int srr_write_ppm(const char* path, int nx, int ny, const unsigned char* rgb8) {
  FILE* f = fopen(path, "w");
  if (!f) return fail(SRR_EIO, std::string("cannot open ") + path);
  fprintf(f, "P3\n%d %d\n255\n", nx, ny);
  for (int i = 0; i < nx * ny; ++i) fprintf(f, "%d %d %d\n", rgb8[3 * i], rgb8[3 * i + 1], rgb8[3 * i + 2]);
  fclose(f);
  return 0;
}

int srr_write_png(const char* path, int nx, int ny, const unsigned char* rgb8) {
  if (!path || !rgb8) return fail(SRR_EINVAL, "null argument");
  std::vector<uint8_t> png;
  std::string err;
  int rc = srr::encode_png(rgb8, nx, ny, 3, png, err);
  if (rc < 0) return fail(rc, err);
  FILE* f = fopen(path, "wb");
  if (!f) return fail(SRR_EIO, std::string("cannot open ") + path);
  size_t w = fwrite(png.data(), 1, png.size(), f);
  fclose(f);
  return w == png.size() ? 0 : fail(SRR_EIO, std::string("short write to ") + path);
}

int srr_image_load(const char* path, int req_comp, int* x, int* y, int* comp, unsigned char** out) {
  if (!path || !x || !y || !out) return fail(SRR_EINVAL, "null argument");
  *out = nullptr;
  srr::Image im;
  std::string err;
  int rc = srr::load_image(path, req_comp, im, err);
  if (rc < 0) return fail(rc == -2 ? SRR_EIO : SRR_EINVAL, err);
  *x = im.w;
  *y = im.h;
  if (comp) *comp = im.file_n;
  *out = (unsigned char*)malloc(im.px.size());
  if (!*out) return fail(SRR_ENOMEM, "out of memory");
  std::memcpy(*out, im.px.data(), im.px.size());
  return im.n;
}

void srr_image_free(unsigned char* pixels) { free(pixels); }

// ---- MERL tables (brdf.h)
struct srr_merl {
  int device = 0;
  DeviceMem<double> table;  // 3 * merl::kCells doubles
};

int srr_merl_create(const double* table, int64_t n_doubles, int device, srr_merl** out) {
  if (!table || !out) return fail(SRR_EINVAL, "null argument");
  if (n_doubles != 3 * (int64_t)merl::kCells) return fail(SRR_EINVAL, "MERL table: dimensions don't match");
  HIPCHK(hipSetDevice(device));
  auto m = std::make_unique<srr_merl>();
  m->device = device;
  MEMCHK(m->table.grow((size_t)n_doubles), SRR_EIO, "MERL table");
  if (hipMemcpy(m->table.get(), table, (size_t)n_doubles * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    return fail(SRR_EIO, "MERL table upload failed");
  *out = m.release();
  return 0;
}

int srr_merl_load(const char* path, int device, srr_merl** out) {  // brdf::read_brdf (brdf.h:156-185)
  if (!path || !out) return fail(SRR_EINVAL, "null argument");
  FILE* f = fopen(path, "rb");
  if (!f) return fail(SRR_EIO, std::string("cannot open MERL table ") + path);
  int32_t dims[3] = {0, 0, 0};
  const bool hdr = fread(dims, sizeof(int32_t), 3, f) == 3;
  const int64_t n = (int64_t)dims[0] * dims[1] * dims[2];
  if (!hdr || n != merl::kCells) {
    fclose(f);
    return fail(SRR_EINVAL, "MERL table: dimensions don't match");
  }
  std::vector<double> t(3 * (size_t)n);
  const size_t got = fread(t.data(), sizeof(double), t.size(), f);
  fclose(f);
  if (got != t.size()) return fail(SRR_EINVAL, "MERL table: truncated file");
  return srr_merl_create(t.data(), (int64_t)t.size(), device, out);
}

void srr_merl_destroy(srr_merl* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  delete m;
}

int srr_merl_lookup(srr_merl* m, int64_t n, const double* angles, double* rgb, int32_t* cell) {
  if (!m || n < 0 || (n > 0 && (!angles || !rgb))) return fail(SRR_EINVAL, "bad MERL lookup arguments");
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(m->device));
  int rc = 0;
  DevBuf<double> d_ang(angles, 4 * (size_t)n, rc), d_rgb(3 * (size_t)n, rc);
  DevBuf<int32_t> d_cell(cell ? (size_t)n : 0, rc);
  if (rc) return rc;
  if (launch_merl_lookup(m->table.get(), n, d_ang.get(), d_rgb.get(), d_cell.get()) < 0) return fail(SRR_EIO, "MERL kernel launch failed");
  if (hipDeviceSynchronize() != hipSuccess || !d_rgb.download(rgb, 3 * (size_t)n) || (cell && !d_cell.download(cell, (size_t)n)))
    return fail(SRR_EIO, "MERL kernel failed");
  return 0;
}

int srr_teapot_vertices(float scale, int divs, float* out) {
  if (divs < 1 || divs > 400) return fail(SRR_EINVAL, "teapot divs out of range");
  std::vector<float> p;
  teapot_triangles(scale, divs, p);
  if (out) std::memcpy(out, p.data(), p.size() * sizeof(float));
  return (int)(p.size() / 9);
}

int64_t srr_bvh_topology(const srr_scene* s, int o, char* buf, int64_t cap) {
  if (!s || !s->s.valid_obj(o) || s->s.obj[o].kind != H_BVH) return fail(SRR_EINVAL, "not a bvh_node handle");
  const HBvh& B = s->s.bvhs[s->s.obj[o].bvh];
  std::map<int, int> pos;
  for (size_t q = 0; q < B.input.size(); ++q) pos[B.input[q]] = (int)q;
  std::string txt;
  char line[256];
  snprintf(line, sizeof line, "box %g %g %g %g %g %g\n", B.box.mn[0], B.box.mn[1], B.box.mn[2], B.box.mx[0],
           B.box.mx[1], B.box.mx[2]);
  txt += line;
  std::vector<int> stack{0};
  while (!stack.empty()) {
    int n = stack.back();
    stack.pop_back();
    const HBvh::Node& nd = B.nodes[n];
    if (nd.left < 0) {
      snprintf(line, sizeof line, "L %d %d\n", pos[B.leaves[~nd.left]], pos[B.leaves[~nd.right]]);
      txt += line;
    } else {
      txt += "N\n";
      stack.push_back(nd.right);
      stack.push_back(nd.left);
    }
  }
  if (buf && cap > 0) {
    int64_t m = std::min<int64_t>(cap - 1, (int64_t)txt.size());
    std::memcpy(buf, txt.data(), m);
    buf[m] = 0;
  }
  return (int64_t)txt.size() + 1;
}

int srr_sobol_points(int n, double* out) {
  if (n < 1 || !out) return fail(SRR_EINVAL, "bad args");
  sobol2((unsigned)n, out);
  return 0;
}

}  // extern "C"
