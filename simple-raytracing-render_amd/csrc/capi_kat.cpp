// The test entry points of the C-ABI (include/srr_capi.h): the device known-answer tests
// (KATs) srr_device_kat, srr_device_mesh_kat, srr_device_world_kat, srr_device_bounce_kat with
// their host-only *_kat_counts, the fold and compaction KAT srr_device_fold_kat, and the libm
// sweeps srr_device_libm.  Each builds its device
// tables with the host scene code a render uses (the fold KAT has none), holds device memory in DevBuf
// (capi_internal.h) and checks every argument before its first HIP call, so a refusal needs
// no GPU.  The product's entry points are in capi.cpp.
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "kernels.h"
#include "renderer.h"

using namespace srr;

namespace {
// ---------------------------------------------------------------- srr_device_kat
constexpr bool kat_is_scene(int kind) { return kind >= KAT_SPHERE; }  // tables flattened from host scenes (kat_scene)
constexpr bool kat_has_scene_per_record(int kind) { return kind >= KAT_SPHERE && kind <= KAT_MEDIUM; }

struct KatIn {  // the checked arguments of one call
  int kind, n, width;
  const float* records;
  const float* rec(int q) const { return records + (size_t)q * width; }
};

struct KatHost {  // what the host scene code builds for k_kat; one family below fills its part
  std::vector<float> aux;                 // 4 floats per record
  std::vector<DStandaloneTri> tris = std::vector<DStandaloneTri>(1);  // KAT_TRIANGLE: one per record
  std::vector<DCamera> cams = std::vector<DCamera>(1);                // KAT_CAMERA: one per record
  Flat light_list;                        // KAT_LIGHTS, KAT_LIGHT_LIST
  Flat scenes;                            // scene KATs: the records' scenes concatenated, or the one texture scene
  std::vector<int32_t> base;              // KatTables::base (one scene per record only)
  std::vector<uint8_t> images;            // KAT_TEX_IMAGE only
  std::vector<float> perlin_ranvec;
  std::vector<int32_t> perlin_perm;
};

// host-side parameters the scene builder would compute (material ctors)
void kat_material_aux(const KatIn& in, KatHost& H) {
  const bool beckmann = in.kind == KAT_BECK_DIST || in.kind == KAT_BECK_PDF;
  Scene hs;
  for (int q = 0; q < in.n; ++q) {
    const float* r = in.rec(q);
    const float prm[4] = {r[0], beckmann ? r[1] : 0, 0, 0};
    const HMat& m = hs.mat[hs.material(beckmann ? MAT_BECKMANN : MAT_ORENNAYAR, -1, prm)];
    H.aux[4 * q] = m.p[0];
    H.aux[4 * q + 1] = m.p[1];
  }
}

// triangle(p0, p1, p2, mat, uv0, uv1, uv2) with face normals (kat.inc)
void kat_triangles(const KatIn& in, KatHost& H) {
  H.tris.resize(in.n);
  Scene hs;
  for (int q = 0; q < in.n; ++q) {
    const float uv9[9] = {0.1f, 0.2f, 0, 0.7f, 0.1f, 0, 0.3f, 0.9f, 0};
    const int h = hs.triangle(in.rec(q), -1, uv9, nullptr);
    const HTri& t = hs.tris[hs.obj[h].tri];
    DStandaloneTri& d = H.tris[q];
    std::memcpy(d.p, t.p, 36);
    std::memcpy(d.sh.n, t.n, 36);
    for (int k = 0; k < 3; ++k) d.sh.uv[2 * k] = t.uv[3 * k], d.sh.uv[2 * k + 1] = t.uv[3 * k + 1];
    d.sh.mat = -1;
  }
}

// camera(lookfrom, lookat, (0,1,0), vfov, aspect, aperture, focus, 0, 1) per record, built
// by the host scene code exactly as a scene's camera (camera.h:33-48)
void kat_cameras(const KatIn& in, KatHost& H) {
  H.cams.resize(in.n);
  for (int q = 0; q < in.n; ++q) {
    const float* r = in.rec(q);
    const float vup[3] = {0, 1, 0};
    Scene cs;
    cs.camera(r, r + 3, vup, r[6], r[7], r[8], r[9], 0.0f, 1.0f);
    const HCamera& c = cs.cam;
    DCamera& d = H.cams[q];
    std::memcpy(d.origin, c.origin, 12);
    std::memcpy(d.llc, c.llc, 12);
    std::memcpy(d.horizontal, c.horizontal, 12);
    std::memcpy(d.vertical, c.vertical, 12);
    std::memcpy(d.u, c.u, 12);
    std::memcpy(d.v, c.v, 12);
    d.time0 = c.time0;
    d.time1 = c.time1;
    d.lens_radius = c.lens_radius;
  }
}

void kat_any_camera(Scene& s) {
  const float lf3[3] = {0, 0, -1}, la3[3] = {0, 0, 0}, up[3] = {0, 1, 0};
  s.camera(lf3, la3, up, 40, 1, 0, 1, 0, 1);
  s.has_camera = true;
}

// the light list {flip(xz_rect(213,343,227,332,554)), sphere((278,700,280),50),
// triangle((150,500,150),(400,520,180),(260,540,420))} of oracle/ref/kat.inc, flattened like a scene's
int kat_light_list(KatHost& H) {
  Scene ls;
  const int rect = ls.wrap(H_FLIP, ls.rect(H_XZ, 213, 343, 227, 332, 554, -1), nullptr);
  const float c[3] = {278, 700, 280};
  const int sph = ls.sphere(c, 50, -1);
  const float p9[9] = {150, 500, 150, 400, 520, 180, 260, 540, 420};
  const int tri = ls.triangle(p9, -1, nullptr, nullptr);
  const int kids[3] = {rect, sph, tri};
  ls.world = ls.lights = ls.list(kids, 3);
  kat_any_camera(ls);
  std::string e;
  if (flatten(ls, H.light_list, e) < 0 || H.light_list.lights.size() != 3) return fail(SRR_EINVAL, "light KAT scene: " + e);
  return 0;
}

// Scene KATs: every object is built by the host scene calls and flattened, as a scene's are
// (rotation sines, a box's six faces and flips, a medium's boundary list and phase material,
// xf_count and its flip bit, the Perlin tables, texture rows).
int kat_flatten_object(Scene& s, int h, Flat& f) {  // world = hitable_list{h}, no lights, any camera
  s.world = s.list(&h, 1);
  s.lights = s.list(&h, 0);
  kat_any_camera(s);
  std::string e;
  return flatten(s, f, e) >= 0 ? 0 : fail(SRR_EINVAL, "KAT scene: " + e);
}

// KAT_SPHERE .. KAT_MEDIUM: one scene per record, the tables concatenated (`base`: each
// record's first rows, kernels.hip kat_scene)
int kat_record_scenes(const KatIn& in, KatHost& H) {
  auto prim = [](Scene& s, float kind_, const float* a, const float* b) {  // a sphere (a, b[0]) or a box (a, b)
    return kind_ == 0 ? s.sphere(a, b[0], -1) : s.box(a, b, -1);
  };
  Flat f, &all = H.scenes;
  for (int q = 0; q < in.n; ++q) {
    const float* r = in.rec(q);
    Scene s;
    int h = -1;
    if (in.kind == KAT_SPHERE) h = s.sphere(r, r[3], -1);
    else if (in.kind == KAT_MSPHERE) h = s.moving_sphere(r, r + 3, r[6], r[7], r[8], -1);
    else if (in.kind == KAT_RECT) {
      h = s.rect(r[0] == 0 ? H_XY : (r[0] == 1 ? H_XZ : H_YZ), r[2], r[3], r[4], r[5], r[6], -1);
      if (r[1] != 0) h = s.wrap(H_FLIP, h, nullptr);
    } else if (in.kind == KAT_BOX) h = s.box(r, r + 3, -1);
    else if (in.kind == KAT_XFORM) {
      h = prim(s, r[0], r + 1, r + 4);
      for (int l = 2; l >= 0; --l) {  // the wrappers are listed outermost first
        const float* w = r + 7 + 4 * l;
        if (w[0] == 1) h = s.wrap(H_TRANSLATE, h, w + 1);
        else if (w[0] == 2 || w[0] == 3) h = s.rotate(w[0] == 2 ? H_ROTY : H_ROTX, h, w[1]);
        else if (w[0] == 4) h = s.wrap(H_FLIP, h, nullptr);
      }
    } else {  // KAT_MEDIUM
      const float one[3] = {1, 1, 1};
      HTex t;
      t.kind = TEX_CONST;
      std::memcpy(t.c, one, 12);
      h = s.medium(prim(s, r[0], r + 1, r + 4), r[7], s.add_tex(t));
    }
    if (const int rc = kat_flatten_object(s, h, f)) return rc;
    const int32_t b8[8] = {(int32_t)all.objs.size(),  f.n_world,
                           (int32_t)all.xforms.size(), (int32_t)all.spheres.size(),
                           (int32_t)all.rects.size(),  (int32_t)all.media.size(),
                           (int32_t)all.mats.size(),   (int32_t)all.texs.size()};
    H.base.insert(H.base.end(), b8, b8 + 8);
    all.objs.insert(all.objs.end(), f.objs.begin(), f.objs.end());
    all.xforms.insert(all.xforms.end(), f.xforms.begin(), f.xforms.end());
    all.spheres.insert(all.spheres.end(), f.spheres.begin(), f.spheres.end());
    all.rects.insert(all.rects.end(), f.rects.begin(), f.rects.end());
    all.media.insert(all.media.end(), f.media.begin(), f.media.end());
    all.mats.insert(all.mats.end(), f.mats.begin(), f.mats.end());
    all.texs.insert(all.texs.end(), f.texs.begin(), f.texs.end());
  }
  H.perlin_ranvec = f.perlin_ranvec;
  H.perlin_perm = f.perlin_perm;
  return 0;
}

// KAT_ISOTROPIC .. KAT_TEX_IMAGE: one scene for all records; aux: the record's texture row
int kat_texture_scene(const KatIn& in, KatHost& H) {
  Scene s;
  const float org[3] = {0, 0, 0};
  auto constant = [&](float x, float y, float z) {
    HTex t;
    t.kind = TEX_CONST;
    t.c[0] = x, t.c[1] = y, t.c[2] = z;
    return s.add_tex(t);
  };
  auto checker = [&](int even, int odd) {
    HTex t;
    t.kind = TEX_CHECKER;
    t.even = even;
    t.odd = odd;
    return s.add_tex(t);
  };
  auto shown = [&](int tex) {  // a texture flattens only if a placed material reaches it
    const float prm[4] = {0, 0, 0, 0};
    return s.sphere(org, 1, s.material(MAT_LAMBERTIAN, tex, prm));
  };
  std::vector<int> hs;
  std::vector<float> scales;
  if (in.kind == KAT_ISOTROPIC) {  // the phase material of constant_medium(sphere, 1, checker(A, B))
    hs.push_back(s.medium(s.sphere(org, 1, -1), 1.0f, checker(constant(0.2f, 0.3f, 0.1f), constant(0.9f, 0.9f, 0.9f))));
  } else if (in.kind == KAT_TEX_CHECKER) {  // checker(A, B) and checker(checker(A, B), checker(C, D))
    const int A = constant(0.2f, 0.3f, 0.1f), B = constant(0.9f, 0.9f, 0.9f), C = constant(0.1f, 0.5f, 0.8f),
              D = constant(0.6f, 0.1f, 0.4f);
    hs.push_back(shown(checker(A, B)));
    hs.push_back(shown(checker(checker(A, B), checker(C, D))));
  } else if (in.kind == KAT_TEX_NOISE) {  // one noise_texture per scale the records name
    for (int q = 0; q < in.n; ++q) {
      const float sc = in.rec(q)[0];
      size_t k = 0;
      while (k < scales.size() && std::memcmp(&scales[k], &sc, 4) != 0) ++k;
      if (k == scales.size()) {
        if (scales.size() == 64) return fail(SRR_EINVAL, "noise KAT: more than 64 scales");
        scales.push_back(sc);
        HTex t;
        t.kind = TEX_NOISE;
        t.c[0] = sc;
        hs.push_back(shown(s.add_tex(t)));
      }
      H.aux[4 * (size_t)q] = (float)k;
    }
  } else {  // KAT_TEX_IMAGE: the 7 x 5 synthetic image of oracle/ref/kat.inc
    HTex t;
    t.kind = TEX_IMAGE;
    t.nx = 7;
    t.ny = 5;
    t.px = gen_image(7, 5, 7u, 0);
    hs.push_back(shown(s.add_tex(std::move(t))));
  }
  // (a rect between the spheres keeps them plain list objects, not a sphere group)
  std::vector<int> kids;
  for (int h : hs) {
    kids.push_back(h);
    kids.push_back(s.rect(H_XY, 0, 1, 0, 1, 0, -1));
  }
  Flat& f = H.scenes;
  if (const int rc = kat_flatten_object(s, s.list(kids.data(), (int)kids.size()), f)) return rc;
  if (in.kind != KAT_ISOTROPIC)  // aux: the record's texture row after flattening
    for (int q = 0; q < in.n; ++q) {
      const int k = in.kind == KAT_TEX_CHECKER ? (in.rec(q)[0] != 0 ? 1 : 0)
                                               : (in.kind == KAT_TEX_NOISE ? (int)H.aux[4 * (size_t)q] : 0);
      H.aux[4 * (size_t)q] = (float)f.mats[f.spheres[k].mat].tex;
    }
  if (in.kind == KAT_TEX_IMAGE) H.images = f.images;
  H.perlin_ranvec = f.perlin_ranvec;
  H.perlin_perm = f.perlin_perm;
  return 0;
}

// ------------------------------------------------- the world and the bounce KAT
// One launch per group of records: both kernels want a launch to hold the records of one group
// (one uploaded world, one light list) in file order.  key[q] is record q's group, checked by the
// caller.  For each group in ascending key, run(key, rec, count) gets a copy of the group's records
// in ascending record index; what it leaves there is written back to the records they came from.
int for_each_record_group(float* records, int n, int width, const std::vector<int>& key,
                          const std::function<int(int, float*, int)>& run) {
  std::map<int, std::vector<int>> groups;
  for (int q = 0; q < n; ++q) groups[key[q]].push_back(q);
  const size_t wb = width * sizeof(float);
  for (const auto& kv : groups) {
    const std::vector<int>& idx = kv.second;
    std::vector<float> rec(idx.size() * (size_t)width);
    for (size_t i = 0; i < idx.size(); ++i) std::memcpy(&rec[i * width], &records[(size_t)idx[i] * width], wb);
    if (const int rc = run(kv.first, rec.data(), (int)idx.size())) return rc;
    for (size_t i = 0; i < idx.size(); ++i) std::memcpy(&records[(size_t)idx[i] * width], &rec[i * width], wb);
  }
  return 0;
}

constexpr long long kWorldKatBaseId = 100000;  // text obj 100000 + w is world w of the `world` KAT's scene

// World w of a world-KAT scene flattened as a render of it would be (the scene's world
// set to the list, then the same flatten, group_sphere_runs included), and leaf_of: per
// DObj row that is a primitive, its position in the depth-first listing of the world's
// leaves in the FILE's order (a list's and a bvh command's children as written, a box's
// six rects, a wrapper's child) -- the order in which the reference harness numbers them.
int world_kat_flatten(Scene& sc, int w, Flat& f, std::vector<int32_t>& leaf_of, int& n_leaves, std::string& err) {
  int h = -1;
  for (auto& kv : sc.text_ids)
    if (kv.first == kWorldKatBaseId + w) h = kv.second;
  if (!sc.valid_obj(h) || sc.obj[h].kind != H_LIST) {
    err = "world KAT: no list object " + std::to_string(kWorldKatBaseId + w);
    return SRR_EINVAL;
  }
  sc.world = h;
  int rc = flatten(sc, f, err);
  if (rc < 0) return rc;
  // leaves under each handle, then flatten's emission order in file numbering: `top` for the
  // world list's own rows (-1 where an object BVH stands), `inner` for the BVHs' children
  std::function<int(int)> count = [&](int k) -> int {
    const HObj& o = sc.obj[k];
    switch (o.kind) {
      case H_LIST: case H_BOX: { int n = 0; for (int c : o.kids) n += count(c); return n; }
      case H_BVH: { int n = 0; for (int c : sc.bvhs[o.bvh].input) n += count(c); return n; }
      case H_FLIP: case H_TRANSLATE: case H_ROTY: case H_ROTX: return count(o.child);
      case H_MEDIUM: return -(1 << 20);  // (refused below)
      default: return 1;
    }
  };
  n_leaves = count(h);
  if (n_leaves <= 0) {
    err = "world KAT: a world holds a medium or nothing";
    return SRR_EINVAL;
  }
  std::vector<int32_t> top, inner;
  std::function<void(int, int, std::vector<int32_t>&)> emit = [&](int k, int base, std::vector<int32_t>& out) {
    const HObj& o = sc.obj[k];
    switch (o.kind) {
      case H_LIST: case H_BOX:
        for (int c : o.kids) { emit(c, base, out); base += count(c); }
        break;
      case H_BVH: {
        const HBvh& B = sc.bvhs[o.bvh];
        std::map<int, int> at;  // child handle -> first leaf number (children are distinct objects)
        for (int c : B.input) { at[c] = base; base += count(c); }
        if (&out == &top) top.push_back(-1);
        for (int l : B.leaves) emit(l, at.at(l), inner);
        break;
      }
      case H_FLIP: case H_TRANSLATE: case H_ROTY: case H_ROTX: emit(o.child, base, out); break;
      default: out.push_back(base);
    }
  };
  emit(h, 0, top);
  leaf_of.assign(f.objs.size(), -1);
  size_t tc = 0, ic = 0;
  bool ok = true;
  for (int k = 0; k < f.n_world && ok; ++k) {
    const DObj& d = f.objs[k];
    if (d.kind == OBJ_SGROUP) {
      const DSGroup& g = f.sgroups[d.idx];
      ok = tc + g.n_items <= top.size();
      for (int i = g.item_off; ok && i < g.item_off + g.n_items; ++i) {
        const DSGItem& it = f.sg_items[i];
        ok = it.pos >= 0 && it.pos < g.n_items && it.obj >= 0 && it.obj < (int)f.objs.size() && top[tc + it.pos] >= 0;
        if (ok) leaf_of[it.obj] = top[tc + it.pos];
      }
      tc += g.n_items;
    } else if (d.kind == OBJ_OBVH) {
      ok = tc < top.size() && top[tc] == -1;
      ++tc;
      const DObvh& o = f.obvhs[d.idx];
      for (int c = o.child_off; ok && c < o.child_off + o.n_children; ++c)
        for (int j = 0; ok && j < f.obvh_children[c].obj_count; ++j) {
          const int row = f.obvh_children[c].obj_begin + j;
          ok = ic < inner.size() && row >= 0 && row < (int)f.objs.size();
          if (ok) leaf_of[row] = inner[ic++];
        }
    } else {
      ok = (d.kind == OBJ_SPHERE || d.kind == OBJ_MSPHERE || d.kind == OBJ_RECT || d.kind == OBJ_TRI) && tc < top.size() &&
           top[tc] >= 0;
      if (ok) leaf_of[k] = top[tc++];
    }
  }
  if (!ok || tc != top.size() || ic != inner.size()) {
    err = "world KAT: the flattened world does not match the scene's leaves (a mesh, or an object used twice)";
    return SRR_EINVAL;
  }
  return 0;
}

size_t world_table_bytes(const Flat& f) {  // renderer.cpp's packed world tables, each padded to 16 bytes
  auto pad = [](size_t b) { return (b + 15) & ~(size_t)15; };
  return pad(f.objs.size() * sizeof(DObj)) + pad(f.xforms.size() * sizeof(DXform)) + pad(f.spheres.size() * sizeof(DSphere)) +
         pad(f.rects.size() * sizeof(DRect)) + pad(f.stris.size() * sizeof(DStandaloneTri)) +
         pad(f.meshes.size() * sizeof(DMesh)) + pad(f.media.size() * sizeof(DMedium)) + pad(f.mats.size() * sizeof(DMat)) +
         pad(f.texs.size() * sizeof(DTex)) + pad(f.lights.size() * sizeof(DLight));
}

constexpr long long kBounceKatBaseId = 200000;  // text obj 200000 + l is light list l of the `bounce` KAT's scene

// The scene flattened as a render of it with light list l would be.  Every material of the
// scene must survive flattening (each is placed in the world), so that material m of a record
// is row m of the device table.
int bounce_kat_flatten(Scene& sc, int l, Flat& f, std::string& err) {
  int h = -1;
  for (auto& kv : sc.text_ids)
    if (kv.first == kBounceKatBaseId + l) h = kv.second;
  if (!sc.valid_obj(h) || sc.obj[h].kind != H_LIST) {
    err = "bounce KAT: no list object " + std::to_string(kBounceKatBaseId + l);
    return SRR_EINVAL;
  }
  sc.lights = h;
  const int rc = flatten(sc, f, err);
  if (rc < 0) return rc;
  if (f.mats.size() != sc.mat.size()) {
    err = "bounce KAT: a material of the scene is not placed in its world";
    return SRR_EINVAL;
  }
  return 0;
}

// ------------------------------------------------- the fold and compaction KAT
constexpr int kFoldMaxRows = 1 << 24, kFoldMaxSpp = 1 << 16, kFoldMaxCount = 1 << 30;
constexpr int64_t kFoldMaxFloats = (int64_t)1 << 28;

int fold_bad(const std::string& what) { return fail(SRR_EINVAL, "fold KAT: " + what); }

// every entry of idx[0 .. n) lies in [0, range); with `injective`, none is repeated
bool fold_indices_ok(const int32_t* idx, int n, int range, bool injective) {
  std::vector<uint8_t> seen(injective ? (size_t)range : 0, 0);
  for (int j = 0; j < n; ++j) {
    if (idx[j] < 0 || idx[j] >= range) return false;
    if (injective && seen[idx[j]]++) return false;
  }
  return true;
}

// The samples on the device, `misalign` floats into a 16-byte-aligned allocation.
struct FoldSamples {
  DevBuf<float> buf;
  const float* ptr;
  FoldSamples(const float* host, size_t n, int misalign, int& rc) : buf(n ? n + 4 : 0, rc), ptr(nullptr) {
    if (rc || !n) return;
    ptr = buf.get() + misalign;
    if (hipMemcpy(buf.get() + misalign, host, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
      rc = fail(SRR_EIO, "copy to device failed");
  }
};

// An "io" array: a device copy of the caller's, written back by done(); NULL stays NULL.
template <class T>
struct FoldIo {
  T* host;
  size_t n;
  DevBuf<T> buf;
  FoldIo(T* h, size_t count, int& rc) : host(h), n(h ? count : 0), buf(h, h ? count : 0, rc) {}
  T* get() const { return buf.get(); }
  bool done() const { return !host || buf.download(host, n); }
};

// the checks of srr_device_fold_kat that need no device: 0, or the refusal
int fold_kat_check(int kind, const srr_fold_kat& a) {
  const int words = kFoldKats[kind].words;
  const bool rows_used = kind != kFoldLevelFinish;
  const bool slots_used = kind == kFoldWindow || kind == kFoldAdaptive || kind == kFoldSpec || kind == kFoldLevelFinish ||
                          (kind == kFoldCompact && (a.active_slot || a.pixels));
  const bool spp_used = words != 0 && kind != kFoldScatter;
  if (rows_used && (a.rows <= 0 || a.rows > kFoldMaxRows)) return fold_bad("rows out of range");
  if (slots_used && (a.n_slots <= 0 || a.n_slots > kFoldMaxRows)) return fold_bad("n_slots out of range");
  if (spp_used && (a.spp <= 0 || a.spp > kFoldMaxSpp)) return fold_bad("spp out of range");
  if (spp_used && (int64_t)a.rows * a.spp * words > kFoldMaxFloats) return fold_bad("too many samples");
  if (words && !a.sample) return fold_bad("no samples");
  const bool folds = kind == kFoldWindow || kind == kFoldAdaptive || kind == kFoldSpec;
  if (a.misalign < 0 || a.misalign > 3 || (a.misalign && !folds)) return fold_bad("misalign out of range");
  if (folds || kind == kFoldCompact) {
    if (kind == kFoldWindow && a.active_slot) return fold_bad("the window sums take no active_slot");
    if (a.active_slot) {
      if (!fold_indices_ok(a.active_slot, a.rows, a.n_slots, true))
        return fold_bad("an active_slot entry is out of range or repeated");
    } else if (slots_used && a.n_slots < a.rows) {
      return fold_bad("n_slots < rows without active_slot");
    }
  }
  switch (kind) {
    case kFoldWindow:
      if (!a.sums) return fold_bad("no acc");
      if (a.ns < 0) return fold_bad("ns out of range");
      break;
    case kFoldAdaptive:
    case kFoldSpec:
      if (!a.sums || !a.mom || !a.mean || !a.keep) return fold_bad("a state array is missing");
      if (a.budget < 1) return fold_bad("budget out of range");
      if (kind == kFoldAdaptive) {
        if (a.n_new < 1 || a.n_new > kFoldMaxCount) return fold_bad("n_new out of range");
        break;
      }
      if (!a.count || !a.ctr) return fold_bad("count or ctr is missing");
      if (a.batch_spp < 1) return fold_bad("batch_spp out of range");
      if (a.min_spp < 0 || a.n < 0 || a.s0 < 0 || a.w < 1 || a.n > kFoldMaxCount || a.w > kFoldMaxCount ||
          (int64_t)a.n + a.w > kFoldMaxCount)
        return fold_bad("n, w, s0 or min_spp out of range");
      if ((int64_t)a.s0 + a.spp > a.w) return fold_bad("s0 + spp_w > w");
      if (a.s0 > 0)
        for (int j = 0; j < a.rows; ++j) {
          const int32_t c = a.count[a.active_slot ? a.active_slot[j] : j];
          if (c < 0 || c > a.n + a.w) return fold_bad("a count outside [0, n + w]");
        }
      break;
    case kFoldLevelFinish:
      if (!a.count || !a.mom || !a.sums || !a.live || !a.keep || !a.lvl || !a.mean) return fold_bad("an array is missing");
      if (a.budget < 1 || a.min_spp < 0) return fold_bad("budget or min_spp out of range");
      for (int i = 0; i < a.n_slots; ++i)
        if (a.count[i] < 0 || a.count[i] > a.budget) return fold_bad("a count outside [0, budget]");
      break;
    case kFoldCompact:
      if (!a.keep || !a.slot_out || !a.pixel_out || !a.n_out) return fold_bad("an array is missing");
      if (a.pixels && (a.n_image <= 0 || !fold_indices_ok(a.pixels, a.n_slots, a.n_image, false)))
        return fold_bad("a pixels entry is outside the output");
      break;
    case kFoldAov:
    case kFoldAovEmission:
      if (!a.sums) return fold_bad("no acc");
      if (a.n_shard <= 0 || a.n_shard > kFoldMaxRows || a.p0 < 0 || (int64_t)a.p0 + a.rows > a.n_shard)
        return fold_bad("p0 + np beyond the shard's pixels");
      if (a.ns < 1) return fold_bad("ns out of range");
      if (kind == kFoldAovEmission && (!a.emission || a.s0 < 0 || a.s0 > kFoldMaxCount)) return fold_bad("no emission, or s0 out of range");
      break;
    case kFoldFinish:
      if (!a.sums || !a.mean) return fold_bad("an array is missing");
      if (a.ns < 1) return fold_bad("ns out of range");
      break;
    case kFoldScatter:
      if (!a.index || !a.image) return fold_bad("an array is missing");
      if (a.n_image <= 0 || a.n_image > kFoldMaxRows || !fold_indices_ok(a.index, a.rows, a.n_image, false))
        return fold_bad("an index entry is outside the image");
      break;
  }
  return 0;
}
}  // namespace

extern "C" {

int srr_device_fold_kat(const char* kind_name, const srr_fold_kat* ap) {
  // every argument is checked before the first HIP call, so a refusal needs no GPU
  if (!kind_name || !ap) return fold_bad("bad arguments");
  int kind = -1;
  for (const FoldKatDesc& d : kFoldKats)
    if (!strcmp(kind_name, d.name)) kind = d.kind;
  if (kind < 0) return fold_bad(std::string("no kind named ") + kind_name);
  const srr_fold_kat& a = *ap;
  if (const int bad = fold_kat_check(kind, a)) return bad;

  const int words = kFoldKats[kind].words;
  const size_t rows = kind == kFoldLevelFinish ? 0 : (size_t)a.rows;
  const size_t slots = kind == kFoldCompact && !a.active_slot && !a.pixels ? rows : (size_t)a.n_slots;
  const size_t n_samples = !words ? 0 : rows * (kind == kFoldScatter ? 1 : (size_t)a.spp) * words;
  int rc = 0;
  FoldSamples sample(a.sample, n_samples, a.misalign, rc);
  if (rc) return rc;
  const char* what = "fold KAT kernel failed";
  auto ran = [&]() { return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess; };
  switch (kind) {
    case kFoldWindow: {
      FoldIo<float> acc(a.sums, 3 * slots, rc), out(a.mean, 3 * slots, rc);
      if (rc) return rc;
      launch_accumulate_window(sample.ptr, a.rows, a.spp, acc.get(), 0, a.init != 0, out.get(), a.ns);
      if (!ran() || !acc.done() || !out.done()) return fail(SRR_EIO, what);
      return 0;
    }
    case kFoldAdaptive:
    case kFoldSpec: {
      DevBuf<int32_t> active(a.active_slot, a.active_slot ? rows : 0, rc);
      FoldIo<float> sums(a.sums, 3 * slots, rc), mom(a.mom, 2 * slots, rc), mean(a.mean, 3 * slots, rc);
      FoldIo<int32_t> count(a.count, slots, rc);
      FoldIo<uint8_t> keep(a.keep, rows, rc);
      FoldIo<unsigned long long> ctr((unsigned long long*)a.ctr, kind == kFoldSpec ? kSpecWords : 0, rc);
      if (rc) return rc;
      if (kind == kFoldAdaptive) {
        const AdaptiveFold A{sample.ptr, active.get(), a.rows, a.spp, sums.get(), (float2*)mom.get(), a.init, a.decide,
                             a.n_new, a.budget, a.rel_tol, a.abs_eps, keep.get(), mean.get(), count.get()};
        launch_adaptive_fold(A, 0);
      } else {
        const AdaptiveSpecFold A{sample.ptr, active.get(), a.rows, a.spp, sums.get(), (float2*)mom.get(), a.n, a.w, a.s0,
                                 a.batch_spp, a.min_spp, a.budget, a.rel_tol, a.abs_eps, keep.get(), mean.get(),
                                 count.get(), ctr.get()};
        launch_adaptive_fold_spec(A, 0);
      }
      if (!ran() || !sums.done() || !mom.done() || !mean.done() || !count.done() || !keep.done() || !ctr.done())
        return fail(SRR_EIO, what);
      return 0;
    }
    case kFoldLevelFinish: {
      DevBuf<int32_t> count(a.count, slots, rc);
      DevBuf<float> mom(a.mom, 2 * slots, rc), sums(a.sums, 3 * slots, rc);
      FoldIo<uint8_t> live(a.live, slots, rc), keep(a.keep, slots, rc);
      FoldIo<int32_t> lvl(a.lvl, kLvlWords, rc), count_out(a.count_out, slots, rc);
      FoldIo<float> mean(a.mean, 3 * slots, rc);
      if (rc) return rc;
      const AdaptiveRule R{a.budget, a.min_spp, a.rel_tol, a.abs_eps};
      launch_adaptive_level_select(a.n_slots, count.get(), (const float2*)mom.get(), R, live.get(), keep.get(), lvl.get(), 0);
      launch_adaptive_finish(a.n_slots, sums.get(), count.get(), a.budget, mean.get(), count_out.get(), lvl.get(), 0);
      if (!ran() || !live.done() || !keep.done() || !lvl.done() || !count_out.done() || !mean.done())
        return fail(SRR_EIO, what);
      return 0;
    }
    case kFoldCompact: {
      DevBuf<uint8_t> keep(a.keep, rows, rc);
      DevBuf<int32_t> active(a.active_slot, a.active_slot ? rows : 0, rc), pixels(a.pixels, a.pixels ? slots : 0, rc);
      DevBuf<int32_t> blk((rows + 255) / 256, rc);
      FoldIo<int32_t> slot_out(a.slot_out, rows, rc), pixel_out(a.pixel_out, rows, rc), n_out(a.n_out, 1, rc);
      if (rc) return rc;
      launch_adaptive_compact(keep.get(), active.get(), a.rows, pixels.get(), blk.get(), slot_out.get(), pixel_out.get(),
                              n_out.get(), 0);
      if (!ran() || !slot_out.done() || !pixel_out.done() || !n_out.done()) return fail(SRR_EIO, what);
      return 0;
    }
    case kFoldAov: {
      const size_t shard = (size_t)a.n_shard;
      FoldIo<float> acc(a.sums, 8 * rows, rc), albedo(a.albedo, 3 * shard, rc), normal(a.normal, 3 * shard, rc),
          depth(a.depth, shard, rc);
      if (rc) return rc;
      const AovFold A{sample.ptr, a.rows, a.spp, acc.get(), a.init, a.finish, a.ns, a.p0, albedo.get(), normal.get(),
                      depth.get()};
      launch_aov_fold(A, 0);
      if (!ran() || !acc.done() || !albedo.done() || !normal.done() || !depth.done()) return fail(SRR_EIO, what);
      return 0;
    }
    case kFoldAovEmission: {
      const size_t shard = (size_t)a.n_shard;
      FoldIo<float> acc(a.sums, 4 * rows, rc), emission(a.emission, 3 * shard, rc);
      DevBuf<int32_t> count(a.count, a.count ? shard : 0, rc);
      if (rc) return rc;
      const AovEmissionFold A{sample.ptr, a.rows, a.spp, a.s0, acc.get(), a.ns, a.p0, count.get(), emission.get()};
      launch_aov_fold_emission(A, 0);
      if (!ran() || !acc.done() || !emission.done()) return fail(SRR_EIO, what);
      return 0;
    }
    case kFoldFinish: {
      DevBuf<float> acc(a.sums, 3 * rows, rc);
      FoldIo<float> mean(a.mean, 3 * rows, rc);
      if (rc) return rc;
      launch_finish(acc.get(), mean.get(), a.rows, a.ns, 0);
      if (!ran() || !mean.done()) return fail(SRR_EIO, what);
      return 0;
    }
    default: {  // kFoldScatter
      DevBuf<int32_t> index(a.index, rows, rc);
      FoldIo<float> image(a.image, 3 * (size_t)a.n_image, rc);
      if (rc) return rc;
      launch_scatter_pixels(sample.ptr, index.get(), a.rows, image.get(), 0);
      if (!ran() || !image.done()) return fail(SRR_EIO, what);
      return 0;
    }
  }
}

int srr_device_kat(const char* name, int n, int width, float* records) {
  if (!name || !records || n <= 0 || width <= 0) return fail(SRR_EINVAL, "bad KAT arguments");
  int kind = -1;
  for (const KatDesc& d : kKats)
    if (!strcmp(name, d.name)) kind = d.kind;
  if (kind < 0) return fail(SRR_EINVAL, std::string("no device KAT named ") + name);
  if (width != kKats[kind].width) return fail(SRR_EINVAL, std::string("KAT ") + name + ": unexpected record width");
  const KatIn in{kind, n, width, records};
  KatHost H;
  H.aux.assign(4 * (size_t)n, 0.f);
  int rc = 0;
  if (kind == KAT_BECK_DIST || kind == KAT_BECK_PDF || kind == KAT_COSINE || kind == KAT_ORENNAYAR) kat_material_aux(in, H);
  else if (kind == KAT_TRIANGLE) kat_triangles(in, H);
  else if (kind == KAT_CAMERA) kat_cameras(in, H);
  else if (kind == KAT_LIGHTS || kind == KAT_LIGHT_LIST) rc = kat_light_list(H);
  else if (kat_has_scene_per_record(kind)) rc = kat_record_scenes(in, H);
  else if (kat_is_scene(kind)) rc = kat_texture_scene(in, H);
  if (rc) return rc;
  const Flat& t = kat_is_scene(kind) ? H.scenes : H.light_list;
  const size_t rn = (size_t)n * width;
  DevBuf<float> d_rec(records, rn, rc), d_aux(H.aux, rc), d_ranvec(H.perlin_ranvec, rc);
  DevBuf<DStandaloneTri> d_tris(H.tris, rc), d_stris(t.stris, rc);
  DevBuf<DCamera> d_cams(H.cams, rc);
  DevBuf<DRect> d_rects(t.rects, rc);
  DevBuf<DSphere> d_sph(t.spheres, rc);
  DevBuf<DLight> d_lights(t.lights, rc);
  DevBuf<DObj> d_objs(t.objs, rc);
  DevBuf<DXform> d_xforms(t.xforms, rc);
  DevBuf<DMedium> d_media(t.media, rc);
  DevBuf<DMat> d_mats(t.mats, rc);
  DevBuf<DTex> d_texs(t.texs, rc);
  DevBuf<uint8_t> d_images(H.images, rc);
  DevBuf<int32_t> d_perm(H.perlin_perm, rc), d_base(H.base, rc);
  if (rc) return rc;
  const KatTables kt{d_cams.get(), d_rects.get(), d_sph.get(), d_stris.get(), d_lights.get(), (int)t.lights.size(),
                     d_objs.get(), d_xforms.get(), d_media.get(), d_mats.get(), d_texs.get(), d_images.get(),
                     d_ranvec.get(), d_perm.get(), d_base.get()};
  if (launch_kat(kind, n, width, d_rec.get(), d_aux.get(), d_tris.get(), kt) < 0) return fail(SRR_EIO, "KAT kernel launch failed");
  if (hipDeviceSynchronize() != hipSuccess || !d_rec.download(records, rn)) return fail(SRR_EIO, "KAT kernel failed");
  return 0;
}

int srr_device_mesh_kat(const char* scene_text, int variant, int quad_max, int stack_cap, int use_gstack, int n,
                        int width, float* records) {
  // every argument is checked before the first HIP call
  if (!scene_text || !records || n <= 0 || n > 1 << 20 || width != kMeshKatWidth)
    return fail(SRR_EINVAL, "bad mesh KAT arguments");
  if (variant < kMeshKatBvh2 || variant > kMeshKatQuad) return fail(SRR_EINVAL, "no such mesh KAT variant");
  if (stack_cap < 1 || stack_cap > paths_kernel_stack()) return fail(SRR_EINVAL, "mesh KAT: stack_cap out of range");
  Scene sc;
  std::string err;
  int rc = scene_from_text(scene_text, sc, err);
  if (rc < 0) return fail(rc, err);
  Flat f;
  if ((rc = flatten(sc, f, err)) < 0) return fail(rc, err);
  // the world list's objects are the meshes, in order: mesh m of a record is world object m
  if (!sc.valid_obj(sc.world) || sc.obj[sc.world].kind != H_LIST || (int)sc.obj[sc.world].kids.size() != f.n_world)
    return fail(SRR_EINVAL, "mesh KAT: the world must be a list of bvh objects");
  std::vector<int32_t> mesh_obj(f.n_world), tri_file(f.tri_shade.size(), -1);
  for (int k = 0; k < f.n_world; ++k) {
    const int h = sc.obj[sc.world].kids[k];
    if (sc.obj[h].kind != H_BVH || f.objs[k].kind != OBJ_MESH || f.objs[k].xf_count != 0)
      return fail(SRR_EINVAL, "mesh KAT: a world object is not a bare triangle mesh");
    const HBvh& B = sc.bvhs[sc.obj[h].bvh];
    const DMesh& m = f.meshes[f.objs[k].idx];
    if (m.n_tris != (int)B.leaves.size() || m.tri_off < 0 || (size_t)m.tri_off + m.n_tris > tri_file.size())
      return fail(SRR_EINVAL, "mesh KAT: mesh tables do not match the bvh");
    std::map<int, int> pos;
    for (size_t q = 0; q < B.input.size(); ++q) pos[B.input[q]] = (int)q;
    for (size_t i = 0; i < B.leaves.size(); ++i) tri_file[m.tri_off + i] = pos.at(B.leaves[i]);
    mesh_obj[k] = k;
  }
  for (int q = 0; q < n; ++q) {
    const float mi = records[(size_t)q * width];
    if (!(mi >= 0 && mi < (float)f.n_world && mi == (float)(int)mi)) return fail(SRR_EINVAL, "mesh KAT: a record names no mesh");
  }
  // the quad walk serves whole waves: pad with copies of the last record
  const int n_run = variant == kMeshKatQuad ? (n + 63) / 64 * 64 : n;
  std::vector<float> rec((size_t)n_run * width);
  std::memcpy(rec.data(), records, (size_t)n * width * sizeof(float));
  for (int q = n; q < n_run; ++q) std::memcpy(&rec[(size_t)q * width], &rec[(size_t)(n - 1) * width], width * sizeof(float));
  srr_renderer* r = nullptr;  // uploads the tables exactly as a render does
  if ((rc = renderer_create_flat(f, 0, &r, err)) < 0) return fail(rc, err);
  std::unique_ptr<srr_renderer> keep(r);
  SceneView S = r->view;
  S.quad_max = quad_max;
  const int gst_cap = use_gstack ? kPathsGlobalStack : 0, lanes = (n_run + 255) / 256 * 256;
  rc = 0;
  DevBuf<float> d_rec(rec, rc);
  DevBuf<int32_t> d_mesh_obj(mesh_obj, rc), d_tri_file(tri_file, rc);
  DevBuf<int2> d_gst((size_t)gst_cap * lanes, rc);
  if (rc) return rc;
  const MeshKatArgs A{n_run, width, d_rec.get(), stack_cap, d_gst.get(), gst_cap, lanes, d_mesh_obj.get(), d_tri_file.get()};
  if (launch_mesh_kat(S, variant, A) < 0) return fail(SRR_EIO, "mesh KAT kernel launch failed");
  if (hipDeviceSynchronize() != hipSuccess || !d_rec.download(records, (size_t)n * width))
    return fail(SRR_EIO, "mesh KAT kernel failed");
  return 0;
}

int srr_world_kat_counts(const char* scene_text, int world, int32_t* counts) {
  if (!scene_text || !counts || world < 0) return fail(SRR_EINVAL, "bad world KAT arguments");
  Scene sc;
  std::string err;
  int rc = scene_from_text(scene_text, sc, err);
  if (rc < 0) return fail(rc, err);
  Flat f;
  std::vector<int32_t> leaf_of;
  int n_leaves = 0;
  if ((rc = world_kat_flatten(sc, world, f, leaf_of, n_leaves, err)) < 0) return fail(rc, err);
  int ng = 0, nb = 0;
  for (int k = 0; k < f.n_world; ++k) {
    ng += f.objs[k].kind == OBJ_SGROUP;
    nb += f.objs[k].kind == OBJ_OBVH;
  }
  counts[0] = f.n_world;
  counts[1] = ng;
  counts[2] = nb;
  counts[3] = n_leaves;
  counts[4] = (int32_t)world_table_bytes(f);
  return 0;
}

int srr_device_world_kat(const char* scene_text, int tables, int n, int width, float* records) {
  // every argument is checked before the first HIP call
  if (!scene_text || !records || n <= 0 || n > 1 << 20 || width != kWorldKatWidth || tables < 0 || tables > 1)
    return fail(SRR_EINVAL, "bad world KAT arguments");
  Scene sc;
  std::string err;
  int rc = scene_from_text(scene_text, sc, err);
  if (rc < 0) return fail(rc, err);
  struct Job { Flat f; std::vector<int32_t> leaf_of; };
  std::map<int, Job> jobs;  // a launch holds the records of one world: its objects are wave-uniform
  std::vector<int> world(n);
  for (int q = 0; q < n; ++q) {
    const float wf = records[(size_t)q * width];
    if (!(wf >= 0 && wf < 1024.f && wf == (float)(int)wf)) return fail(SRR_EINVAL, "world KAT: a record names no world");
    world[q] = (int)wf;
    jobs[world[q]];  // (filled below)
  }
  for (auto& kv : jobs) {  // every world is flattened and checked before anything is uploaded
    Job& j = kv.second;
    int n_leaves = 0;
    if ((rc = world_kat_flatten(sc, kv.first, j.f, j.leaf_of, n_leaves, err)) < 0) return fail(rc, err);
    if (tables == 1 && world_table_bytes(j.f) > (size_t)kPathsWorldLdsBytes)
      return fail(SRR_EINVAL, "world KAT: a world's tables do not fit the LDS copy");
    bool grouped = false;
    for (int k = 0; k < j.f.n_world; ++k) grouped = grouped || j.f.objs[k].kind == OBJ_SGROUP;
    for (int q = 0; q < n; ++q)  // list_hit is a medium's boundary walk, and a boundary's spheres are never grouped
      if (grouped && world[q] == kv.first && records[(size_t)q * width + 10] != 0)
        return fail(SRR_EINVAL, "world KAT: an is_medium record on a world with a sphere group");
  }
  return for_each_record_group(records, n, width, world, [&](int w, float* rec, int count) {
    const Job& j = jobs.at(w);
    srr_renderer* r = nullptr;  // uploads the tables exactly as a render does
    if ((rc = renderer_create_flat(j.f, 0, &r, err)) < 0) return fail(rc, err);
    std::unique_ptr<srr_renderer> keep(r);
    rc = 0;
    DevBuf<float> d_rec(rec, (size_t)count * width, rc);
    DevBuf<int32_t> d_leaf(j.leaf_of, rc);
    if (rc) return rc;
    const WorldKatArgs A{count, width, d_rec.get(), d_leaf.get()};
    if (launch_world_kat(r->view, tables, A) < 0) return fail(SRR_EIO, "world KAT kernel launch failed");
    if (hipDeviceSynchronize() != hipSuccess || !d_rec.download(rec, (size_t)count * width))
      return fail(SRR_EIO, "world KAT kernel failed");
    return 0;
  });
}

int srr_bounce_kat_counts(const char* scene_text, int list, int32_t* counts) {
  if (!scene_text || !counts || list < 0) return fail(SRR_EINVAL, "bad bounce KAT arguments");
  Scene sc;
  std::string err;
  int rc = scene_from_text(scene_text, sc, err);
  if (rc < 0) return fail(rc, err);
  Flat f;
  if ((rc = bounce_kat_flatten(sc, list, f, err)) < 0) return fail(rc, err);
  for (int k = 0; k < 6; ++k) counts[k] = 0;
  counts[0] = (int32_t)f.lights.size();
  for (const DLight& L : f.lights) {
    if (L.kind < LIGHT_NONE || L.kind > LIGHT_TRI) return fail(SRR_EINVAL, "bounce KAT: a light of an unknown kind");
    ++counts[1 + L.kind];
  }
  counts[5] = (int32_t)f.mats.size();
  return 0;
}

int srr_device_bounce_kat(const char* scene_text, int variant, int deep_tries, int n, int width, float* records) {
  // every argument is checked before the first HIP call
  if (!scene_text || !records || n <= 0 || n > 1 << 20 || width != kBounceKatWidth || variant < 0 || variant > 1 ||
      deep_tries < 0)
    return fail(SRR_EINVAL, "bad bounce KAT arguments");
  Scene sc;
  std::string err;
  int rc = scene_from_text(scene_text, sc, err);
  if (rc < 0) return fail(rc, err);
  std::map<int, Flat> flats;  // a launch holds the records of one light list (a wave keeps their order)
  std::vector<int> list(n);
  for (int q = 0; q < n; ++q) {
    const float* r = records + (size_t)q * width;
    if (!(r[0] >= 0 && r[0] < 1024.f && r[0] == (float)(int)r[0])) return fail(SRR_EINVAL, "bounce KAT: a record names no light list");
    if (!(r[1] >= 0 && r[1] < (float)sc.mat.size() && r[1] == (float)(int)r[1]))
      return fail(SRR_EINVAL, "bounce KAT: a record names no material");
    if (!(r[17] >= 0 && r[17] <= 1e6f && r[18] >= 0 && r[18] <= 1e6f)) return fail(SRR_EINVAL, "bounce KAT: a record's depth is out of range");
    list[q] = (int)r[0];
    flats[list[q]];  // (filled below)
  }
  for (auto& kv : flats)  // every list is flattened and checked before anything is uploaded
    if ((rc = bounce_kat_flatten(sc, kv.first, kv.second, err)) < 0) return fail(rc, err);
  return for_each_record_group(records, n, width, list, [&](int l, float* rec, int count) {
    srr_renderer* r = nullptr;  // uploads the tables exactly as a render does
    if ((rc = renderer_create_flat(flats.at(l), 0, &r, err)) < 0) return fail(rc, err);
    std::unique_ptr<srr_renderer> keep(r);
    rc = 0;
    DevBuf<float> d_rec(rec, (size_t)count * width, rc);
    if (rc) return rc;
    const BounceKatArgs A{count, width, d_rec.get(), variant, deep_tries};
    if (launch_bounce_kat(r->view, A) < 0) return fail(SRR_EIO, "bounce KAT kernel launch failed");
    if (hipDeviceSynchronize() != hipSuccess || !d_rec.download(rec, (size_t)count * width))
      return fail(SRR_EIO, "bounce KAT kernel failed");
    return 0;
  });
}

int srr_device_libm(const char* fn, int64_t n, const void* x, const void* y, void* out0, void* out1) {
  // every argument is checked before the first HIP call, so a refusal needs no GPU
  // (tests/test_device_libm.py test_unknown_names_are_refused runs without one)
  if (!fn || !x || !out0 || n <= 0 || n > (int64_t)1 << 30) return fail(SRR_EINVAL, "bad libm sweep arguments");
  int k = -1;
  for (int i = 0; i < kLibmFnCount; ++i)
    if (!strcmp(fn, kLibmFns[i].name)) k = i;
  if (k < 0) return fail(SRR_EINVAL, std::string("no device libm routine named ") + fn);
  const LibmFn& f = kLibmFns[k];
  if ((f.n_in == 2 && !y) || (f.n_out == 2 && !out1))
    return fail(SRR_EINVAL, std::string("libm routine ") + fn + ": missing second operand or output");
  const size_t b = (size_t)n * (f.f64 ? sizeof(double) : sizeof(float));  // bytes; the second operand and output only if used
  int rc = 0;
  DevBuf<char> d_x((const char*)x, b, rc), d_y((const char*)y, f.n_in == 2 ? b : 0, rc), d_out0(b, rc),
      d_out1(f.n_out == 2 ? b : 0, rc);
  if (rc) return rc;
  if (launch_libm(k, n, d_x.get(), d_y.get(), d_out0.get(), d_out1.get()) < 0) return fail(SRR_EIO, "libm kernel launch failed");
  if (hipDeviceSynchronize() != hipSuccess || !d_out0.download((char*)out0, b) || (f.n_out == 2 && !d_out1.download((char*)out1, b)))
    return fail(SRR_EIO, "libm kernel failed");
  return 0;
}

}  // extern "C"
