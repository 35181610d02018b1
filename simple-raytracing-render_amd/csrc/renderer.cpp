// Renderer: scene upload and the multi-lane wavefront driver (renderer.h).
#include "renderer.h"

#include "multi.h"
#include "adaptive_schedule.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <cstdio>

namespace srr {

constexpr int kVisitWords = 3 + 2 * 64;  // SRR_FLAG_COUNT_VISITS: sums + two histograms

// RCHK words a failure by the source expression; RMEM, for allocations and uploads, by the
// buffer's name ("bounce records: out of memory")
#define RMEM(x, what)                                                  \
  do {                                                                 \
    hipError_t e_ = (x);                                               \
    if (e_ != hipSuccess) {                                            \
      err = std::string(what) + ": " + hipGetErrorString(e_);          \
      return SRR_EIO;                                                  \
    }                                                                  \
  } while (0)
#define RCHK(x) RMEM(x, #x)

template <class T>
static hipError_t upload(T** dst, const std::vector<T>& v, DeviceBag& keep) {
  hipError_t e = keep.add(dst, v.size());
  if (e == hipSuccess && !v.empty()) e = hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return e;
}

int renderer_create(const Scene& sc, int device, srr_renderer** out, std::string& err) {
  Flat F;
  int rc = flatten(sc, F, err);
  if (rc < 0) return rc;
  return renderer_create_flat(F, device, out, err);
}

int renderer_create_flat(const Flat& F, int device, srr_renderer** out, std::string& err) {
  std::unique_ptr<srr_renderer> r(new srr_renderer());
  r->device = device;
  if (const char* e = getenv("SRR_LANES")) r->n_lanes = std::max(1, std::min(kMaxLanes, atoi(e)));
  RCHK(hipSetDevice(device));
  DeviceBag& K = r->scene_bufs;
#define UPLOAD(dst, v) RMEM(upload(&dst, v, K), "scene table " #v)
  DObj* objs; DXform* xf; DSphere* sph; DRect* rct; DStandaloneTri* st; DMesh* me; float* nodes; float* n4;
  float* tp; TriShade* ts; DMedium* md; DMat* mt; DTex* tx; uint8_t* im; float* pr; int32_t* pp; DLight* li;
  DCamera* cm;
  DObvh* ob;
  DObvhChild* oc;
  DSGroup* sg;
  DSGItem* sgi;
  std::vector<DCamera> cam{F.cam};
  UPLOAD(objs, F.objs);
  UPLOAD(xf, F.xforms);
  UPLOAD(sph, F.spheres);
  UPLOAD(rct, F.rects);
  UPLOAD(st, F.stris);
  UPLOAD(me, F.meshes);
  UPLOAD(nodes, F.nodes);
  UPLOAD(n4, F.node4);
  float* n4q;
  UPLOAD(n4q, F.node4q);
  UPLOAD(tp, F.tri_pos);
  // the walk's leaf-pair records (kernels.h SceneView::tri_edge): record i (128 B) holds
  // p0, e1 = p1 - p0, e2 = p2 - p0 of triangles i and i+1 (the last repeats itself), the
  // float differences tri_hit's front test forms -- computed here, they round the same
  float* tedge;
  {
    const size_t nt = F.tri_pos.size() / 16;
    std::vector<float> pr(32 * nt, 0.f);
    for (size_t i = 0; i < nt; ++i)
      for (int j = 0; j < 2; ++j) {
        const float* q = &F.tri_pos[16 * std::min(i + j, nt - 1)];
        float* o = &pr[32 * i + 9 * j];
        for (int c = 0; c < 3; ++c) {
          o[c] = q[c];
          o[3 + c] = q[4 + c] - q[c];
          o[6 + c] = q[8 + c] - q[c];
        }
      }
    RMEM(upload(&tedge, pr, K), "scene table tri_edge");
  }
  UPLOAD(ts, F.tri_shade);
  UPLOAD(md, F.media);
  UPLOAD(ob, F.obvhs);
  UPLOAD(oc, F.obvh_children);
  UPLOAD(sg, F.sgroups);
  UPLOAD(sgi, F.sg_items);
  UPLOAD(mt, F.mats);
  UPLOAD(tx, F.texs);
  UPLOAD(im, F.images);
  UPLOAD(pr, F.perlin_ranvec);
  UPLOAD(pp, F.perlin_perm);
  UPLOAD(li, F.lights);
  UPLOAD(cm, cam);
  // world-traversal tables packed for LDS staging (kernels.h SceneView::world_blob)
  std::vector<uint8_t> blob;
  int off[10];
  auto put = [&](int k, const void* data, size_t bytes) {
    off[k] = (int)blob.size();
    blob.insert(blob.end(), (const uint8_t*)data, (const uint8_t*)data + bytes);
    blob.resize((blob.size() + 15) & ~(size_t)15, 0);
  };
  put(0, F.objs.data(), F.objs.size() * sizeof(DObj));
  put(1, F.xforms.data(), F.xforms.size() * sizeof(DXform));
  put(2, F.spheres.data(), F.spheres.size() * sizeof(DSphere));
  put(3, F.rects.data(), F.rects.size() * sizeof(DRect));
  put(4, F.stris.data(), F.stris.size() * sizeof(DStandaloneTri));
  put(5, F.meshes.data(), F.meshes.size() * sizeof(DMesh));
  put(6, F.media.data(), F.media.size() * sizeof(DMedium));
  put(7, F.mats.data(), F.mats.size() * sizeof(DMat));
  put(8, F.texs.data(), F.texs.size() * sizeof(DTex));
  put(9, F.lights.data(), F.lights.size() * sizeof(DLight));
  uint8_t* wb;
  UPLOAD(wb, blob);
#undef UPLOAD
  SceneView& V = r->view;
  V.world_blob = (const uint4*)wb;
  V.world_words = (int)(blob.size() / 16);
  for (int k = 0; k < 10; ++k) V.world_off[k] = off[k];
  V.objs = objs;
  V.n_world = F.n_world;
  V.has_media = F.media.empty() ? 0 : 1;
  V.xforms = xf;
  V.spheres = sph;
  V.rects = rct;
  V.stris = st;
  V.meshes = me;
  V.nodes = (const float4*)nodes;
  V.node4 = (const float4*)n4;
  V.node4_lds = (int)std::min<size_t>(kPathsLdsNodes, F.node4.size() / 32);
  V.node4_total = (int)(F.node4.size() / 32);
  V.node4q = F.node4q_ok && !F.node4q.empty() ? (const float4*)n4q : nullptr;
  V.node4_lds_q = (int)std::min<size_t>(2 * kPathsLdsNodes, F.node4q.size() / kNode4qWords);
  {  // compressed 64-B nodes for the per-lane mesh walks (SRR_CBVH=0/1)
    const char* e = getenv("SRR_CBVH");
    V.use_q = V.node4q && e && atoi(e) != 0;
  }
  // Quad-cooperative mesh traversal (SRR_QUAD=1; off by default).  In round 2 it
  // paid on the 640,000-triangle teapot (1,054 -> 1,573 Msamples/s), but most of
  // that came from sharing the whole-tree walks of NaN-bound rays over a quad;
  // with those folded cooperatively (kernels.hip mesh_scan_nan) the per-lane walk
  // is faster there too: 5,384 vs 5,170 Msamples/s.
  {
    const char* e = getenv("SRR_QUAD");
    V.quad_trace = e ? (atoi(e) != 0) : false;
    const char* q = getenv("SRR_QUAD_MAX");
    V.quad_max = q ? atoi(q) : 32;  // 640k-tri teapot: 16 -> 1,569, 32 -> 1,598, 64 -> 1,552 Msamples/s
  }
  {  // one mesh at the top of the world list: k_paths compacts its traversals block-wide
    int n_mesh = 0;
    V.mesh_obj = -1;
    for (int k = 0; k < F.n_world; ++k)
      if (F.objs[k].kind == OBJ_MESH) {
        ++n_mesh;
        V.mesh_obj = k;
      }
    if (n_mesh != 1) V.mesh_obj = -1;
  }
  V.tri_pos = (const float4*)tp;
  V.tri_edge = (const float4*)tedge;
  V.tri_shade = ts;
  V.media = md;
  V.obvhs = ob;
  V.obvh_children = oc;
  V.sgroups = sg;
  V.sg_items = sgi;
  V.mats = mt;
  V.texs = tx;
  V.images = im;
  V.perlin_ranvec = pr;
  V.perlin_perm = pp;
  V.lights = li;
  V.n_lights = (int)F.lights.size();
  V.light_weight = V.n_lights > 0 ? (float)(1.0 / V.n_lights) : 0.f;
  V.cam = cm;
  r->has_meshes = !F.meshes.empty() || !F.obvhs.empty();
  r->diffuse_only = true;
  for (const DMat& m : F.mats)
    if (m.kind != MAT_LAMBERTIAN && m.kind != MAT_ORENNAYAR && m.kind != MAT_DIFFUSE_LIGHT) r->diffuse_only = false;
  // suspendable mesh walks by default (SRR_WALK_Q unset) where they were
  // measured to pay: specular / microfacet materials or media (walks from surfaces inside
  // the mesh's box run long: C3 +2 %, C4 +4 %, C4_real +3 %, C5 +6 %) or a large mesh (the
  // 640,000-triangle teapot +3 %); not for a diffuse-only scene with a small mesh, whose
  // walks are short (C2: the suspension check costs 0.5-1 % and gains nothing)
  {
    int max_tris = 0;
    for (const DMesh& m : F.meshes) max_tris = std::max(max_tris, (int)m.n_tris);
    r->walk_q_default = (!F.meshes.empty() && (!r->diffuse_only || V.has_media || max_tris >= 20000)) ? 8 : 0;
  }
  RCHK(hipStreamCreateWithFlags(&r->acc_st, hipStreamNonBlocking));
  RCHK(hipEventCreate(&r->ev_beg));
  RCHK(hipEventCreate(&r->ev_end));
  RCHK(hipEventCreateWithFlags(&r->ev_async_in, hipEventDisableTiming));
  for (int l = 0; l < kMaxLanes; ++l) {
    Lane& L = r->lanes[l];
    RCHK(hipStreamCreateWithFlags(&L.st, hipStreamNonBlocking));
    RCHK(hipEventCreate(&L.ev_t0));
    RCHK(hipEventCreate(&L.ev_t1));
    RCHK(hipEventCreate(&L.ev_s1));
    RCHK(hipEventCreateWithFlags(&L.ev_rb, hipEventDisableTiming));
    for (int k = 0; k < kRegionsPerLane; ++k) {
      RCHK(hipEventCreateWithFlags(&L.done_ev[k], hipEventDisableTiming));
      RCHK(hipEventCreateWithFlags(&L.acc_ev[k], hipEventDisableTiming));
    }
    RMEM(L.cnt.grow(16), "lane counters");
    RMEM(L.rb.grow(16), "lane counters' host mirror");
  }
  *out = r.release();
  return 0;
}

// PathState's depth-0 members for n paths (rays, RNG, depth, spec, hit record), the state a
// first hit needs: all the AOVs allocate, the start of a lane's pool.  P starts afresh.
static hipError_t alloc_depth0(DeviceBag& bag, PathState& P, size_t n) {
  P = PathState{};
  hipError_t e = bag.add(&P.ray_o, n);
  if (e == hipSuccess) e = bag.add(&P.ray_d, n);
  if (e == hipSuccess) e = bag.add(&P.lcg, n);
  if (e == hipSuccess) e = bag.add(&P.pcg, n);
  if (e == hipSuccess) e = bag.add(&P.depth, n);
  if (e == hipSuccess) e = bag.add(&P.spec, n);
  if (e == hipSuccess) e = bag.add(&P.hit_w, n);
  if (e == hipSuccess) e = bag.add(&P.hit_p, n);
  if (e == hipSuccess) e = bag.add(&P.hit_n, n);
  return e;
}

static int ensure_lane(Lane& L, size_t n, int depth, bool keep, std::string& err) {
  int d = std::max(depth, 1);
  if (n <= L.cap && d <= L.cap_depth && (!keep || L.has_raw)) return 0;
  L.bufs.clear();
  L.cap = 0;  // (until every buffer is there: a failure below leaves a pool that the next call replaces)
  L.act[0] = L.act[1] = L.lists = nullptr;
  PathState& P = L.P;
  RMEM(alloc_depth0(L.bufs, P, n), "lane path state");
  RMEM(L.bufs.add(&P.rec_a, n * d), "lane bounce records");
  RMEM(L.bufs.add(&P.sample, 3 * n), "lane samples");
  RMEM(L.bufs.add(&L.lists, 4 * n), "lane family lists");
  RMEM(L.bufs.add(&L.act[0], n), "lane active list");
  RMEM(L.bufs.add(&L.act[1], n), "lane active list");
  L.has_raw = keep;
  if (keep) {
    RMEM(L.bufs.add(&P.raw, 3 * n), "lane kept radiance");
    RMEM(L.bufs.add(&P.rays, n), "lane kept ray counts");
  }
  L.cap = n;
  L.cap_depth = d;
  return 0;
}

// Per-pixel running sums: zeroed by a render without SRR_FLAG_CONTINUE; a render
// with it adds its samples to them, so consecutive sample ranges accumulate in
// sample order -- bitwise the sums of one render of all of them.
static void accum_key(const srr_params* p, int key[5]) {
  const bool whole = p->shard_count <= 1;
  key[0] = p->nx;
  key[1] = p->ny;
  key[2] = whole ? 0 : p->shard_index;
  key[3] = whole ? 1 : p->shard_count;
  key[4] = whole ? 0 : p->tile;
}

// zero_pending (optional): the caller zeroes the sums itself (its first
// accumulation starts from 0) instead of a memset here
static int begin_accum(srr_renderer* r, const srr_params* p, int64_t npix, hipStream_t st, std::string& err,
                       bool* zero_pending = nullptr) {
  if (zero_pending) *zero_pending = false;
  int key[5];
  accum_key(p, key);
  if (p->flags & SRR_FLAG_CONTINUE) {
    if (r->acc_npix != npix) {
      err = "SRR_FLAG_CONTINUE: no running sums for this shard (render without the flag or srr_accum_set first)";
      return SRR_EINVAL;
    }
    if (p->sample_begin != r->acc_samples) {
      err = "SRR_FLAG_CONTINUE: sample_begin " + std::to_string(p->sample_begin) + " != the " +
            std::to_string(r->acc_samples) + " samples already in the running sums";
      return SRR_EINVAL;
    }
    if (r->acc_key[0] >= 0 && !std::equal(key, key + 5, r->acc_key)) {
      err = "SRR_FLAG_CONTINUE: the running sums belong to another frame or shard";
      return SRR_EINVAL;
    }
    std::copy(key, key + 5, r->acc_key);
    r->adaptive.sums_valid = false;  // the render adds to acc
    return 0;
  }
  r->adaptive.sums_valid = false;  // acc is zeroed: an adaptive state's sums go with it
  if (zero_pending) *zero_pending = true;
  else RCHK(hipMemsetAsync(r->acc.get(), 0, 3 * npix * sizeof(float), st));
  r->acc_npix = npix;
  r->acc_samples = 0;
  std::copy(key, key + 5, r->acc_key);
  return 0;
}

// Stages a shard's pixel list on the device (with the frame accumulator sized
// to it); an identity list is not uploaded (the path engine does not read it).
static hipError_t stage_pixels(srr_renderer* r, const int32_t* pix, int64_t npix, bool identity) {
  r->pix_key[0] = -1;  // srr_render_device sets the key once the render succeeds
  const hipError_t e = ensure_pixels(r, npix);
  if (e != hipSuccess) return e;
  r->pix_identity = identity;
  return identity ? hipSuccess : hipMemcpy(r->pixels.get(), pix, npix * sizeof(int32_t), hipMemcpyHostToDevice);
}

hipError_t ensure_pixels(srr_renderer* r, int64_t npix) {
  if ((size_t)npix <= r->pixels.capacity()) return hipSuccess;
  // the held list and the running sums go with the old buffers: nothing may continue them
  r->pix_key[0] = -1;
  r->acc_npix = 0;
  r->acc_samples = 0;
  std::fill(r->acc_key, r->acc_key + 5, -1);
  r->adaptive.sums_valid = false;
  return grow_pair(r->pixels, (size_t)npix, r->acc, 3 * (size_t)npix);
}

// A device Sobol set holds the first `have` points; the set is a
// prefix-stable sequence (tests/test_dist_gloo.py), so it is generated and
// uploaded only when a render needs more points than it holds.
static hipError_t ensure_sobol(DeviceMem<double>& set, int& have, int n_sobol) {
  if (n_sobol <= have) return hipSuccess;
  have = 0;
  hipError_t e = set.grow(2 * (size_t)n_sobol);
  if (e != hipSuccess) return e;
  std::vector<double> sp(2 * (size_t)n_sobol);
  sobol2((unsigned)n_sobol, sp.data());
  e = hipMemcpy(set.get(), sp.data(), sp.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) have = n_sobol;
  return e;
}

// SRR_FLAG_KEEP_PATHS: room for this frame's `need` paths, in both buffers or in neither
static int ensure_kept(srr_renderer* r, size_t need, std::string& err) {
  RMEM(grow_pair(r->raw_all, 3 * need, r->rays_all, need), "kept paths");
  r->kept_paths = (int64_t)need;
  return 0;
}

// Invalidates the running sums unless the render that began them committed:
// a failed render leaves partial sums that no SRR_FLAG_CONTINUE may build on.
struct AccCommit {
  srr_renderer* r;
  bool ok = false;
  ~AccCommit() {
    if (!ok) r->acc_npix = 0;
  }
};

// The stream, buffers and events of one path-engine frame (renderer.h FrameSlot):
// created on first use, grown as frames need.
static int slot_init(FrameSlot& F, hipStream_t shared_st, std::string& err) {
  if (F.ev_beg) return 0;
  if (shared_st) {
    F.st = shared_st;
  } else {
    RCHK(hipStreamCreateWithFlags(&F.st, hipStreamNonBlocking));
    F.own_stream = true;
  }
  RCHK(hipEventCreate(&F.ev_beg));
  RCHK(hipEventCreate(&F.ev_end));
  RMEM(F.ctr.grow(kPathsCtrWords), "frame counters");
  RMEM(F.ctr_host.grow(kPathsCtrWords), "frame counters' host mirror");
  return 0;
}

// the slot's events and its own stream; the buffers go with the slot itself
static void slot_destroy(FrameSlot& F) {
  for (hipEvent_t e : F.win_ev) (void)hipEventDestroy(e);
  if (F.ev_beg) (void)hipEventDestroy(F.ev_beg);
  if (F.ev_end) (void)hipEventDestroy(F.ev_end);
  if (F.own_stream && F.st) (void)hipStreamDestroy(F.st);
  F = FrameSlot{};
}

// Path-resident engine (kernels.hip k_paths): one persistent kernel per window
// of samples; samples land in a [pixel][sample] buffer that k_accumulate_window
// sums per pixel in sample order, so the image is bitwise the wavefront engine's.
// paths_enqueue puts a whole frame on slot F's stream (sums in `acc`, zeroed by
// the first window when `zero_pending`); paths_finish waits for it and reads its
// counters.  The caller has staged the pixel list and the Sobol set.
// What the k_paths launches of one frame share: paths_prepare sizes the slot's bounce
// records and traversal-stack extension and reads the per-frame environment knobs.
struct PathsSetup {
  int gst_cap = 0;     // global stack extension entries per lane (0: none)
  int walk_q = 0;      // suspendable mesh walks (PathWork::walk_q before the gstack condition)
  int deep_tries = 32; // coop_mixture threshold
  int stack_cap = kPathsLdsStack;
  size_t budget = 0;   // sample-window bytes (SRR_WINDOW_MB over the renderers sharing the device)
  int tail_min = kPathsTailMin;  // chunk-synchronous variants: survivors that trigger a tail pass (SRR_TAIL_MIN)
  int pool_cap = 64;             // ... and usable survivor slots (SRR_POOL_CAP)
};

static int paths_prepare(srr_renderer* r, FrameSlot& F, int max_depth, PathsSetup& ps, std::string& err) {
  // persistent lanes and their bounce records
  if (!r->pw_lanes) r->pw_lanes = paths_lanes_per_device(r->view, r->device);
  // (a second column set, a head-pass lane's, where a chunk-synchronous variant may be
  // launched: diffuse only, no media; 16 B x lanes x max_depth more, 210 MB per slot at depth 50)
  const bool head_cols = r->diffuse_only && !r->view.has_media;
  const size_t rec_need = (head_cols ? 2 : 1) * (size_t)r->pw_lanes * std::max(1, max_depth);
  RMEM(F.rec.grow(rec_need), "bounce records");
  // global extension of the BVH4 traversal stack, for meshes deep enough to need it
  // (SRR_GSTACK=0 disables it: every deeper traversal then re-walks the BVH2)
  const char* gs_env = getenv("SRR_GSTACK");
  ps.gst_cap = (r->has_meshes && !(gs_env && !atoi(gs_env))) ? kPathsGlobalStack : 0;
  // ... followed by the save area of suspended mesh walks (3 float4, 6 int2's bytes, per lane)
  static_assert(sizeof(float4) == 2 * sizeof(int2), "the save area is counted in stack entries");
  if (ps.gst_cap) RMEM(F.gstack.grow(((size_t)ps.gst_cap + 6) * r->pw_lanes), "traversal-stack extension");
  // suspendable mesh walks: a walk still running when at most SRR_WALK_Q / 64
  // of its wave's lanes walk continues in the next wave-iteration (default: the scene's
  // walk_q_default, 8 or 0); SRR_WALK_Q=0 never suspends and launches the kernel variant
  // without the feature (read per frame: tests switch it between renders)
  const char* wq_env = getenv("SRR_WALK_Q");
  ps.walk_q = wq_env ? std::max(0, std::min(64, atoi(wq_env))) : r->walk_q_default;
  // sample window: all pixels x W samples, buffer within SRR_WINDOW_MB (default 16384: a
  // 1080p frame of 1,024 spp in 2 windows, not 3 -- one drain and one serial accumulation
  // fewer)
  ps.budget = (size_t)16384 << 20;
  if (const char* e = getenv("SRR_WINDOW_MB")) ps.budget = (size_t)std::max(1, atoi(e)) << 20;
  ps.budget /= (size_t)std::max(1, r->window_share);
  // attempts after which a pending resampling loop takes every free lane of its
  // wave (kernels.hip coop_mixture); SRR_DEEP_TRIES=0 forces that branch (tests)
  const char* dt_env = getenv("SRR_DEEP_TRIES");
  ps.deep_tries = dt_env ? std::max(0, atoi(dt_env)) : 32;
  // the survivor pool of the chunk-synchronous variants (tests force the rare flows; read per frame)
  if (const char* e = getenv("SRR_TAIL_MIN")) ps.tail_min = std::max(1, std::min(64, atoi(e)));
  if (const char* e = getenv("SRR_POOL_CAP")) ps.pool_cap = std::max(1, std::min(64, atoi(e)));
  ps.stack_cap = kPathsLdsStack;  // kernels.hip kStack
  if (const char* e = getenv("SRR_STACK_CAP")) ps.stack_cap = std::max(1, std::min(kPathsLdsStack, atoi(e)));
  return 0;
}

// Samples per window for `npix` pixels that still need `spp` samples: within the
// window budget and k_paths' 32-bit path numbering (npix * W < 2^31).
static int window_samples(const PathsSetup& ps, int64_t npix, int spp) {
  const int64_t w_max = std::max<int64_t>(1, (((int64_t)1 << 31) - 1) / std::max<int64_t>(1, npix));
  int W = (int)std::max<int64_t>(
      1, std::min<int64_t>(std::min<int64_t>(spp, w_max), (int64_t)(ps.budget / (12 * (size_t)npix))));
  // a window of a multiple of 4 samples is summed with 16-byte loads (k_accumulate_window16;
  // 1080p: 345 -> 344 samples, still 3 windows of 1,024); the sums do not depend on W
  if (W < spp && W >= 16) W &= ~3;
  return W;
}

// The slot's sample window holds at least win_paths paths.
static int ensure_window(srr_renderer* r, FrameSlot& F, size_t win_paths, std::string& err) {
  hipError_t e = F.sample.grow(3 * win_paths);
  if (e == hipErrorOutOfMemory) {
    // the synchronous slot and the two async slots each keep their window across
    // mode switches (at most 3 x SRR_WINDOW_MB of the 288 GB); only when the device
    // runs out are the other mode's windows given back (the next frame there allocates again)
    (void)hipGetLastError();
    if (&F == &r->sync_slot) {
      drain_async(r);
      for (FrameSlot& A : r->async_slots) A.sample.reset();
    } else {
      r->sync_slot.sample.reset();
    }
    e = F.sample.grow(3 * win_paths);
  }
  RMEM(e, "sample window");
  return 0;
}

// One k_paths launch over `npix` pixels (list `pixels`, nullptr = identity) x the Wn
// samples whose first global index is s_first; no kept paths, no diagnostics.
static PathWork paths_work(srr_renderer* r, FrameSlot& F, const srr_params* p, const PathsSetup& ps,
                           const int32_t* pixels, int64_t npix, int s_first, int Wn) {
  PathWork w{};
  w.pixels = pixels;
  w.sobol = r->sobol.get() + 2 * (size_t)s_first;
  w.npix = (int)npix;
  w.spp_w = Wn;
  w.s_base = s_first;
  w.nx = p->nx;
  w.ny = p->ny;
  w.div_spp = make_udiv31((uint32_t)Wn);
  w.div_nx = make_udiv31((uint32_t)p->nx);
  w.base_seed = p->base_seed;
  w.n_paths = (int64_t)npix * Wn;
  w.max_depth = p->max_depth;
  w.cursor = F.ctr.get() + kCtrCursor;
  w.counters = F.ctr.get();
  w.sample = F.sample.get();
  w.rec = F.rec.get();
  w.err = (int*)(F.ctr.get() + kCtrError);
  const int64_t bl = paths_block_lanes(r->view);  // whole blocks of the launch's size
  w.lanes = (int)std::min<int64_t>(r->pw_lanes, ((w.n_paths + bl - 1) / bl) * bl);
  w.stack_cap = ps.stack_cap;
  w.gstack = ps.gst_cap ? F.gstack.get() : nullptr;
  w.gstack_cap = ps.gst_cap;
  w.deep_tries = ps.deep_tries;
  w.walk_q = ps.gst_cap ? ps.walk_q : 0;  // (the save area follows the global stack extension)
  w.tail_min = ps.tail_min;
  w.pool_cap = ps.pool_cap;
  return w;
}

static int paths_enqueue(srr_renderer* r, FrameSlot& F, const srr_params* p, bool identity, int64_t npix,
                         float* acc, bool zero_pending, int64_t acc_total, float* d_mean, bool diagnostics,
                         std::string& err) {
  const bool keep = (p->flags & SRR_FLAG_KEEP_PATHS) != 0;
  hipStream_t st = F.st;
  PathsSetup ps;
  {
    const int rc = paths_prepare(r, F, p->max_depth, ps, err);
    if (rc < 0) return rc;
  }
  const int W = window_samples(ps, npix, p->spp);
  if ((int64_t)npix * W >= ((int64_t)1 << 31)) {
    err = "frame too large for one sample window (npix >= 2^31)";
    return SRR_EINVAL;
  }
  {
    const int rc = ensure_window(r, F, (size_t)npix * W, err);
    if (rc < 0) return rc;
  }
  RCHK(hipMemsetAsync(F.ctr.get(), 0, kPathsCtrWords * sizeof(unsigned long long), st));
  const bool want_sums = (p->flags & SRR_FLAG_SUMS) != 0;
  // per-window HIP events around k_paths, read once the frame is done (no host
  // round trip between windows)
  const int n_windows = (p->spp + W - 1) / W;
  while ((int)F.win_ev.size() < 2 * n_windows) {
    hipEvent_t e;
    RCHK(hipEventCreate(&e));
    F.win_ev.push_back(e);
  }
  F.n_windows = n_windows;
  const bool all_fam = !r->diffuse_only;
  // diagnostics (SRR_WAVE_TIMES=1): per-wave start / exit times of each k_paths launch
  static const bool want_wave_times = getenv("SRR_WAVE_TIMES") != nullptr;
  unsigned long long* wave_times = nullptr;
  const int n_waves = (r->pw_lanes + 63) / 64;
  if (want_wave_times && diagnostics) {
    RMEM(r->pw_wave_times.grow(4 * (size_t)n_waves), "wave times");
    wave_times = r->pw_wave_times.get();
    RCHK(hipMemsetAsync(wave_times, 0, 4 * (size_t)n_waves * sizeof(unsigned long long), st));
  }
#ifdef SRR_SLOW_RAYS
  RMEM(r->pw_slow.grow(16 * 65536 + 16), "slow-ray records");
  RCHK(hipMemsetAsync(r->pw_slow.get() + 16 * 65536, 0, 16 * sizeof(float), st));
#endif
  RCHK(hipEventRecord(F.ev_beg, st));
  for (int s0 = 0; s0 < p->spp; s0 += W) {
    const int Wn = std::min(W, p->spp - s0);
    PathWork w = paths_work(r, F, p, ps, identity ? nullptr : r->pixels.get(), npix, p->sample_begin + s0, Wn);
    w.raw = keep ? r->raw_all.get() : nullptr;
    w.rays = keep ? r->rays_all.get() : nullptr;
    w.keep_spp = p->spp;
    w.keep_s0 = s0;
    w.wave_times = wave_times;
    w.slow_rays = diagnostics ? r->pw_slow.get() : nullptr;
    w.slow_count = w.slow_rays ? (unsigned*)(r->pw_slow.get() + 16 * 65536) : nullptr;
    const int wi = s0 / W;
    if (wi > 0) RCHK(hipMemsetAsync(w.cursor, 0, sizeof(unsigned long long), st));  // window 0: zeroed with ctr
    RCHK(hipEventRecord(F.win_ev[2 * wi], st));
    if (launch_paths(r->view, w, all_fam ? 1 : 0, st) != 0) {
      err = "k_paths refused: stack_cap " + std::to_string(w.stack_cap) +
            " exceeds the kernel build's LDS stack (a host and kernels built with different SRR_KSTACK)";
      return SRR_EINVAL;
    }
    RCHK(hipEventRecord(F.win_ev[2 * wi + 1], st));
    // the last window also writes the output (k_finish fused): means, or raw sums (SRR_FLAG_SUMS)
    const bool last = s0 + Wn >= p->spp;
    launch_accumulate_window(F.sample.get(), (int)npix, Wn, acc, st, wi == 0 && zero_pending, last ? d_mean : nullptr,
                             want_sums ? 0 : (int)acc_total);
    if (wave_times) {  // realtime clock: 100 MHz (10 ns ticks)
      RCHK(hipEventSynchronize(F.win_ev[2 * wi + 1]));
      float ms = 0;
      RCHK(hipEventElapsedTime(&ms, F.win_ev[2 * wi], F.win_ev[2 * wi + 1]));
      std::vector<unsigned long long> wt(4 * (size_t)n_waves);
      RCHK(hipMemcpy(wt.data(), wave_times, wt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      std::vector<std::pair<double, int>> ex;
      unsigned long long t0 = ~0ull;
      for (int i = 0; i < n_waves; ++i)
        if (wt[4 * i + 1]) t0 = std::min(t0, wt[4 * i]);
      for (int i = 0; i < n_waves; ++i)
        if (wt[4 * i + 1]) ex.push_back({(wt[4 * i + 1] - t0) * 1e-5, i});  // ms
      std::sort(ex.begin(), ex.end());
      if (!ex.empty()) {
        auto q = [&](double f) { return ex[std::min(ex.size() - 1, (size_t)(f * ex.size()))].first; };
        fprintf(stderr, "k_paths wave exits (ms after the first wave start, %zu waves, kernel %.3f ms): "
                "min %.3f p10 %.3f p50 %.3f p90 %.3f p99 %.3f max %.3f\n", ex.size(), ms, ex.front().first, q(0.1),
                q(0.5), q(0.9), q(0.99), ex.back().first);
        // per wave: start, exit, world rays, wave-iterations, most mixture rounds in one iteration
        auto show = [&](const char* what, int i) {
          fprintf(stderr, "  %s wave %d: start %.3f exit %.3f rays %llu iterations %llu max mixture rounds %llu\n", what,
                  i, (wt[4 * i] - t0) * 1e-5, (wt[4 * i + 1] - t0) * 1e-5, wt[4 * i + 2], wt[4 * i + 3] & 0xffffffffull,
                  wt[4 * i + 3] >> 32);
        };
        show("median", ex[ex.size() / 2].second);
        for (size_t k = ex.size() - std::min<size_t>(4, ex.size()); k < ex.size(); ++k) show("late", ex[k].second);
      }
      RCHK(hipMemsetAsync(wave_times, 0, wt.size() * sizeof(unsigned long long), st));
    }
  }
  if (n_windows == 0) {  // spp 0: nothing rendered, the output is the sums as they stand
    if (want_sums)
      RCHK(hipMemcpyAsync(d_mean, acc, 3 * (size_t)npix * sizeof(float), hipMemcpyDeviceToDevice, st));
    else
      launch_finish(acc, d_mean, npix, (int)acc_total, st);
  }
  RCHK(hipMemcpyAsync(F.ctr_host.get(), F.ctr.get(), kPathsCtrWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  RCHK(hipEventRecord(F.ev_end, st));
  F.npix = npix;
  F.paths = npix * p->spp;
  return 0;
}

static int paths_finish(srr_renderer* r, FrameSlot& F, const srr_params* p, srr_stats* stats, std::string& err) {
  RCHK(hipStreamSynchronize(F.st));
  RCHK(hipGetLastError());
  srr_stats s{};
  double kernel_ms = 0;
  for (int wi = 0; wi < F.n_windows; ++wi) {
    float ms = 0;
    RCHK(hipEventElapsedTime(&ms, F.win_ev[2 * wi], F.win_ev[2 * wi + 1]));
    kernel_ms += ms;
  }
  unsigned long long ctr[kPathsCtrWords];
  std::memcpy(ctr, F.ctr_host.get(), sizeof(ctr));
  if (getenv("SRR_PATHS_TIMING") && ctr[kCtrWaveIters]) {
    const double it = (double)ctr[kCtrWaveIters];
    fprintf(stderr, "k_paths per wave-iteration (ticks): refill %.0f  world %.0f  mesh %.0f  record %.0f  scatter %.0f  fold %.0f  (%llu wave-iterations)\n",
            ctr[kCtrTicksRefill] / it, ctr[kCtrTicksWorld] / it, ctr[kCtrTicksMesh] / it, ctr[kCtrTicksRecord] / it,
            (ctr[kCtrTicksShade] - ctr[kCtrTicksRecord]) / it, ctr[kCtrTicksFold] / it, ctr[kCtrWaveIters]);
    fprintf(stderr, "  scatter: mixture loop %.0f ticks, %.2f rounds per wave-iteration\n", ctr[kCtrTicksMixture] / it,
            ctr[kCtrMixtureRounds] / it);
    auto per = [](unsigned long long a, unsigned long long b) { return b ? (double)a / (double)b : 0.0; };
    fprintf(stderr, "  families: beck %.0f ticks/it (runs in %.1f %% of its, %.1f lanes/run), spec %.0f (%.1f %%, %.1f), "
                    "diff set-up %.0f (%.1f %%, %.1f); lanes in a path %.1f of 64\n",
            ctr[kCtrTicksBeck] / it, 100 * ctr[kCtrItsBeck] / it, per(ctr[kCtrLanesBeck], ctr[kCtrItsBeck]),
            ctr[kCtrTicksSpec] / it, 100 * ctr[kCtrItsSpec] / it, per(ctr[kCtrLanesSpec], ctr[kCtrItsSpec]),
            ctr[kCtrTicksDiffSetup] / it, 100 * ctr[kCtrItsDiff] / it, per(ctr[kCtrLanesDiff], ctr[kCtrItsDiff]),
            ctr[kCtrLanesInPath] / it);
    fprintf(stderr, "  mesh: longest walk %.1f node steps/it, %.1f lane steps/it over %.1f walking lanes, "
                    "%.0f ticks per step of the longest walk\n",
            ctr[kCtrMeshSteps] / it, ctr[kCtrMeshLaneSteps] / it, ctr[kCtrMeshWalkers] / it,
            per(ctr[kCtrTicksMesh], ctr[kCtrMeshSteps]));
    fprintf(stderr, "  mesh leaf queue: %.0f ticks/it, %.1f passes/it (%.0f ticks per pass)\n", ctr[kCtrLeafTicks] / it,
            ctr[kCtrLeafPasses] / it, per(ctr[kCtrLeafTicks], ctr[kCtrLeafPasses]));
    fprintf(stderr, "  mesh step parts (ticks/it): node fetch %.0f  slab + queue %.0f  order + push + pop %.0f\n",
            ctr[kCtrStepFetch] / it, ctr[kCtrStepSlab] / it, ctr[kCtrStepOrder] / it);
    fprintf(stderr, "  beckmann mixture: %.2f attempts per Beckmann scatter, %.2f for the wave's slowest lane per run\n",
            per(ctr[kCtrBeckAttempts], ctr[kCtrLanesBeck]), per(ctr[kCtrBeckAttemptsMax], ctr[kCtrItsBeck]));
    fprintf(stderr, "  suspended walks: %.2f lanes per wave-iteration\n", ctr[kCtrSuspended] / it);
    fprintf(stderr, "  camera-ray-only iterations (every tracing lane at depth 0): %llu of %llu, world + mesh %.0f ticks "
                    "per wave-iteration of them; the others %.0f\n",
            ctr[kCtrItsCamOnly], ctr[kCtrWaveIters], per(ctr[kCtrTicksCamOnly], ctr[kCtrItsCamOnly]),
            per(ctr[kCtrTicksWorld] + ctr[kCtrTicksMesh] - ctr[kCtrTicksCamOnly], ctr[kCtrWaveIters] - ctr[kCtrItsCamOnly]));
    // (the wave-iterations above count every trace pass; the pre-trace passes are among them,
    // their ticks in no other phase)
    fprintf(stderr, "  pre-trace: %llu passes of the %llu wave-iterations, %.0f ticks each (%.0f per wave-iteration); "
                    "shade rounds %.2f per wave-iteration\n",
            ctr[kCtrPretracePasses], ctr[kCtrWaveIters], per(ctr[kCtrTicksPretrace], ctr[kCtrPretracePasses]),
            ctr[kCtrTicksPretrace] / it, ctr[kCtrShadeRounds] / it);
    // the chunk-synchronous flow's passes (each one wave-iteration: trace, shade, fold and its bookkeeping)
    fprintf(stderr, "  head passes: %llu, %.0f ticks each, %.1f lanes in a path; tail passes: %llu, %.0f ticks each, %.1f lanes\n",
            ctr[kCtrHeadPasses], per(ctr[kCtrTicksHead], ctr[kCtrHeadPasses]), per(ctr[kCtrHeadLanes], ctr[kCtrHeadPasses]),
            ctr[kCtrTailPasses], per(ctr[kCtrTicksTail], ctr[kCtrTailPasses]), per(ctr[kCtrTailLanes], ctr[kCtrTailPasses]));
  }
#ifdef SRR_SLOW_RAYS
  if (r->pw_slow.get()) {  // diagnostics build: dump the slow world hits' records (one line per lane, JSON)
    unsigned n = 0;
    RCHK(hipMemcpy(&n, r->pw_slow.get() + 16 * 65536, sizeof(unsigned), hipMemcpyDeviceToHost));
    n = std::min(n, 65536u);
    std::vector<float> v(16 * (size_t)n);
    if (n) RCHK(hipMemcpy(v.data(), r->pw_slow.get(), v.size() * sizeof(float), hipMemcpyDeviceToHost));
    auto I = [&](size_t k) { int x; memcpy(&x, &v[k], 4); return x; };
    for (unsigned i = 0; i < n; ++i) {
      const size_t b = 16 * (size_t)i;
      fprintf(stderr, "SLOWRAY {\"g\": %d, \"depth\": %d, \"o\": [%.9g, %.9g, %.9g], \"d\": [%.9g, %.9g, %.9g], "
              "\"tm\": %.9g, \"ticks\": %d, \"steps\": %d, \"obj\": %d, \"prim\": %d, \"t\": %.9g, \"slot\": %d, "
              "\"t0\": %d, \"spp_w\": %d}\n", I(b), I(b + 1), v[b + 2], v[b + 3], v[b + 4], v[b + 5], v[b + 6], v[b + 7], v[b + 8],
              I(b + 9), I(b + 10), I(b + 11), I(b + 12), v[b + 13], I(b + 14), I(b + 15), p->spp);
    }
  }
#else
  (void)r;
  (void)p;
#endif
  if (ctr[kCtrError]) {
    err = "k_paths index guard tripped (bits " + std::to_string(ctr[kCtrError]) + ")";
    return SRR_EIO;
  }
  float total = 0;
  RCHK(hipEventElapsedTime(&total, F.ev_beg, F.ev_end));
  s.world_rays = (int64_t)ctr[kCtrWorldRays];
  s.stack_overflows = (int64_t)ctr[kCtrStackOverflows];
  s.deep_traversals = (int64_t)ctr[kCtrDeepTraversals];
  s.mixture_capped = (int64_t)ctr[kCtrMixtureCapped];
  s.walks_suspended = (int64_t)ctr[kCtrSuspended];
  s.paths = F.paths;
  s.trace_ms = kernel_ms;
  s.total_ms = total;
  s.trace_launches = F.n_windows;
  if (stats) *stats = s;
  return 0;
}

static void finish_slot(srr_renderer* r, FrameSlot& F) {
  F.busy = false;
  srr_params none{};
  F.rc = paths_finish(r, F, &none, &F.stats, F.err);
  r->done_tickets.push_back({F.ticket, F.rc, F.stats, F.err});
}

// Frames in flight read the shard's pixel list and the Sobol set: anything that
// reallocates them waits for those frames first (their stats stay for srr_render_wait).
void drain_async(srr_renderer* r) {
  for (FrameSlot& F : r->async_slots)
    if (F.busy) finish_slot(r, F);
}

static int paths_stage(srr_renderer* r, const srr_params* p, const int32_t* pix, int64_t npix, bool& identity,
                       std::string& err) {
  identity = r->pix_identity;
  if (pix != nullptr || p->sample_begin + p->spp > r->sobol_n) drain_async(r);
  if (pix) {  // a new pixel list (else the renderer holds this shard's already)
    identity = p->shard_count <= 1;
    for (int64_t i = 0; identity && i < npix; i += std::max<int64_t>(1, npix / 64)) identity = pix[i] == i;
    RMEM(stage_pixels(r, pix, npix, identity), "pixel list and running sums");
  }
  RMEM(ensure_sobol(r->sobol, r->sobol_n, p->sample_begin + p->spp), "Sobol points");
  return 0;
}

static int render_paths(srr_renderer* r, const srr_params* p, const int32_t* pix, int64_t npix, float* d_mean,
                        srr_stats* stats, std::string& err) {
  const bool keep = (p->flags & SRR_FLAG_KEEP_PATHS) != 0;
  bool identity = false;
  {
    const int rc = paths_stage(r, p, pix, npix, identity, err);
    if (rc < 0) return rc;
  }
  if (keep) {
    const int rc = ensure_kept(r, (size_t)npix * p->spp, err);
    if (rc < 0) return rc;
  }
  FrameSlot& F = r->sync_slot;
  {
    const int rc = slot_init(F, r->acc_st, err);
    if (rc < 0) return rc;
  }
  // the sums of a fresh frame are zeroed by the first window's accumulation (init)
  bool zero_pending = false;
  {
    const int rc = begin_accum(r, p, npix, F.st, err, p->spp > 0 ? &zero_pending : nullptr);
    if (rc < 0) return rc;
  }
  AccCommit commit{r};
  const int64_t acc_total = r->acc_samples + p->spp;
  {
    const int rc = paths_enqueue(r, F, p, identity, npix, r->acc.get(), zero_pending, acc_total, d_mean, true, err);
    if (rc < 0) {
      (void)hipStreamSynchronize(F.st);  // windows already enqueued must not outlive the error
      return rc;
    }
  }
  {
    const int rc = paths_finish(r, F, p, stats, err);
    if (rc < 0) return rc;
  }
  r->acc_samples = acc_total;
  commit.ok = true;
  return 0;
}

// ---- adaptive sampling (include/srr_capi.h srr_render_adaptive)
static int ensure_adaptive(AdaptiveState& A, size_t npix, std::string& err) {
  if (npix <= A.cap) return 0;
  const int pass_spp_max = A.pass_spp_max;
  const int64_t fill_paths = A.fill_paths;
  A = AdaptiveState{};  // every old buffer goes before the first new one comes
  A.pass_spp_max = pass_spp_max;  // (the setting of srr_adaptive_speculate stays)
  A.fill_paths = fill_paths;
  RMEM(A.mom.grow(npix), "adaptive moments");
  RMEM(A.count.grow(npix), "adaptive counts");
  RMEM(A.live.grow(npix), "adaptive live flags");
  RMEM(A.lvl.grow(kLvlWords), "adaptive resume words");
  RMEM(A.lvl_host.grow(kLvlWords), "adaptive resume words' host mirror");
  for (int k = 0; k < 2; ++k) {
    RMEM(A.slot[k].grow(npix), "adaptive slot list");
    RMEM(A.pixel[k].grow(npix), "adaptive pixel list");
  }
  RMEM(A.keep.grow(npix), "adaptive keep flags");
  RMEM(A.blk.grow((npix + 255) / 256 + 1), "adaptive compaction scratch");
  RMEM(A.n_host.grow(1), "adaptive count's host mirror");
  RMEM(A.spec_ctr.grow(kSpecWords), "speculative fold counters");
  RMEM(A.spec_ctr_host.grow(kSpecWords), "speculative fold counters' host mirror");
  A.cap = npix;  // (set last: after a failure above the next call starts afresh)
  return 0;
}

// The end of a fresh or resumed frame: counters back, one sync, the stats out.
static int adaptive_frame_end(FrameSlot& F, srr_adaptive_stats& s, srr_adaptive_stats* stats, std::string& err) {
  hipStream_t st = F.st;
  RCHK(hipMemcpyAsync(F.ctr_host.get(), F.ctr.get(), kPathsCtrWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  RCHK(hipEventRecord(F.ev_end, st));
  RCHK(hipStreamSynchronize(st));
  RCHK(hipGetLastError());
  if (F.ctr_host.get()[kCtrError]) {
    err = "k_paths index guard tripped (bits " + std::to_string(F.ctr_host.get()[kCtrError]) + ")";
    return SRR_EIO;
  }
  float total = 0;
  RCHK(hipEventElapsedTime(&total, F.ev_beg, F.ev_end));
  s.world_rays = (int64_t)F.ctr_host.get()[kCtrWorldRays];
  s.total_ms = total;
  if (stats) {
    s.struct_size = stats->struct_size;
    *stats = s;
  }
  return 0;
}

// Speculative passes (include/srr_capi.h srr_adaptive_speculate) of one call: whether the
// setting gives this call's batch_spp two batches or more, the width of each pass, and
// what srr_adaptive_last_spec_stats reports afterwards.
struct SpecCall {
  bool on = false;
  int pass_spp_max = 0;
  int64_t fill_paths = 0;
  int32_t windows = 0;
  int64_t traced = 0;
};

static SpecCall spec_call(const AdaptiveState& A, const srr_adaptive_params* a) {
  SpecCall sc;
  sc.pass_spp_max = A.pass_spp_max;
  sc.fill_paths = A.fill_paths;
  sc.on = A.pass_spp_max / a->batch_spp >= 2;
  return sc;
}

// samples the pass at level n gives each of its n_act slots
static int spec_width(const SpecCall& sc, const srr_adaptive_params* a, int64_t n_act, int n, int budget) {
  if (!sc.on) return std::min(a->batch_spp, budget - n);
  return adaptive_pass_width(n_act, n, budget, a->batch_spp, sc.pass_spp_max, sc.fill_paths);
}

// One window (s0, Wn) of the speculative pass (n, w) over the n_act rows of `slots`.
static void spec_fold(srr_renderer* r, FrameSlot& F, const srr_adaptive_params* a, const int32_t* slots, int64_t n_act,
                      int n, int w, int s0, int Wn, int budget, float* d_mean) {
  AdaptiveState& A = r->adaptive;
  AdaptiveSpecFold f{};
  f.sample = F.sample.get();
  f.active_slot = slots;
  f.n_active = (int)n_act;
  f.spp_w = Wn;
  f.sums = r->acc.get();
  f.mom = A.mom.get();
  f.n = n;
  f.w = w;
  f.s0 = s0;
  f.batch_spp = a->batch_spp;
  f.min_spp = a->min_spp;
  f.budget = budget;
  f.rel_tol = a->rel_tol;
  f.abs_eps = a->abs_eps;
  f.keep = A.keep.get();
  f.mean = d_mean;
  f.count = A.count.get();
  f.ctr = A.spec_ctr.get();
  launch_adaptive_fold_spec(f, F.st);
}

// After the frame's sync: the call's stats without the samples traced past a stop, and
// the record for srr_adaptive_last_spec_stats.  stopped (may be nullptr) += the slots that
// stopped below the budget inside speculative passes.
static void spec_frame_end(AdaptiveState& A, const SpecCall& sc, srr_adaptive_stats& s, int64_t* stopped) {
  const int64_t discarded = sc.on ? (int64_t)A.spec_ctr_host.get()[kSpecDiscarded] : 0;
  if (sc.on && stopped) *stopped += (int64_t)A.spec_ctr_host.get()[kSpecStopped];
  s.paths = sc.traced - discarded;
  A.spec_windows = sc.windows;
  A.spec_traced = sc.traced;
  A.spec_discarded = discarded;
}

// The pass loop: everything that can refuse the frame has been checked and every
// buffer sized (render_adaptive), so from here on only HIP itself can fail.
// win_cap: paths the slot's sample window holds.
static int adaptive_passes(srr_renderer* r, FrameSlot& F, const srr_params* p, const srr_adaptive_params* a,
                           const PathsSetup& ps, bool identity, int64_t npix, size_t win_cap, float* d_mean,
                           int32_t* d_count, srr_adaptive_stats* stats, std::string& err) {
  AdaptiveState& A = r->adaptive;
  hipStream_t st = F.st;
  const int budget = p->spp;
  const int32_t* shard_pixels = identity ? nullptr : r->pixels.get();
  int32_t* n_dev = A.blk.get() + (A.cap + 255) / 256;
  srr_adaptive_stats s{};
  SpecCall sc = spec_call(A, a);
  RCHK(hipMemsetAsync(F.ctr.get(), 0, kPathsCtrWords * sizeof(unsigned long long), st));
  if (sc.on) RCHK(hipMemsetAsync(A.spec_ctr.get(), 0, kSpecWords * sizeof(unsigned long long), st));
  RCHK(hipEventRecord(F.ev_beg, st));
  int n = 0;     // samples every active pixel holds
  int cur = -1;  // the active lists are A.slot / A.pixel[cur]; -1: every slot, in order
  int64_t n_act = npix;
  bool first_launch = true;
  while (n_act > 0 && n < budget) {
    const int w = spec_width(sc, a, n_act, n, budget), n_new = n + w;
    // can a pixel retire after this pass?  (if none can, no flags, no compaction, no read-back:
    // n_new is the last boundary of a speculative pass, so none of its boundaries asks the rule)
    const bool decide = n_new >= budget || (n_new >= a->min_spp && a->rel_tol > 0.f);
    // several batches in one pass: the fold asks the rule at every batch boundary
    const bool spec = w > a->batch_spp && decide;
    const int32_t* slots = cur < 0 ? nullptr : A.slot[cur].get();
    const int32_t* pixels = cur < 0 ? shard_pixels : A.pixel[cur].get();
    // the pass in sample windows that fit the slot's buffer (one, unless the frame is huge)
    int W = (int)std::min<int64_t>(window_samples(ps, n_act, w), (int64_t)(win_cap / (size_t)n_act));
    if (W < w && W >= 16) W &= ~3;
    for (int s0 = 0; s0 < w; s0 += W) {
      const int Wn = std::min(W, w - s0);
      const PathWork pw = paths_work(r, F, p, ps, pixels, n_act, n + s0, Wn);
      if (!first_launch) RCHK(hipMemsetAsync(pw.cursor, 0, sizeof(unsigned long long), st));  // first: zeroed with ctr
      first_launch = false;
      if (launch_paths(r->view, pw, r->diffuse_only ? 0 : 1, st) != 0) {
        err = "k_paths refused the launch";  // (stack_cap was checked before the first pass)
        return SRR_EINVAL;
      }
      sc.windows += 1;
      if (spec) {
        spec_fold(r, F, a, slots, n_act, n, w, s0, Wn, budget, d_mean);
        continue;
      }
      AdaptiveFold f{};
      f.sample = F.sample.get();
      f.active_slot = slots;
      f.n_active = (int)n_act;
      f.spp_w = Wn;
      f.sums = r->acc.get();
      f.mom = A.mom.get();
      f.init = n + s0 == 0;
      f.decide = decide && s0 + Wn >= w;
      f.n_new = n_new;
      f.budget = budget;
      f.rel_tol = a->rel_tol;
      f.abs_eps = a->abs_eps;
      f.keep = A.keep.get();
      f.mean = d_mean;
      f.count = A.count.get();
      launch_adaptive_fold(f, st);
    }
    n = n_new;
    s.passes += 1;
    sc.traced += n_act * w;
    if (n >= budget) break;  // the fold retired every active pixel at the budget
    if (!decide) continue;
    const int nxt = cur < 0 ? 0 : cur ^ 1;
    launch_adaptive_compact(A.keep.get(), slots, (int)n_act, shard_pixels, A.blk.get(), A.slot[nxt].get(), A.pixel[nxt].get(),
                            n_dev, st);
    // the one host round trip of a pass: the next launch is sized by the survivors
    RCHK(hipMemcpyAsync(A.n_host.get(), n_dev, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    RCHK(hipStreamSynchronize(st));
    const int64_t n_next = *A.n_host.get();
    if (n_next < 0 || n_next > n_act) {
      err = "adaptive compaction returned " + std::to_string(n_next) + " of " + std::to_string(n_act) + " pixels";
      return SRR_EIO;
    }
    // (the slots that stop inside a speculative pass are counted by its folds: the pass that
    // reaches the budget is followed by no compaction)
    if (!spec) s.pixels_retired += n_act - n_next;
    n_act = n_next;
    cur = nxt;
  }
  // every slot retired in some pass's fold, which left its count in the state
  if (d_count)
    RCHK(hipMemcpyAsync(d_count, A.count.get(), (size_t)npix * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  if (sc.on)
    RCHK(hipMemcpyAsync(A.spec_ctr_host.get(), A.spec_ctr.get(), kSpecWords * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost, st));
  const int rc = adaptive_frame_end(F, s, nullptr, err);
  if (rc < 0) return rc;
  spec_frame_end(A, sc, s, &s.pixels_retired);
  if (stats) {
    s.struct_size = stats->struct_size;
    *stats = s;
  }
  return 0;
}

// The pass loop of a resumed frame (include/srr_capi.h): the slots of the state hold
// different counts, so each pass takes the live slots of the least count -- one common
// s_base per k_paths launch, as in a fresh frame -- and retirement is evaluated afresh
// from the state (k_adaptive_level) before every pass.  Checked and sized like
// adaptive_passes: only HIP itself can fail here.
static int adaptive_resume_passes(srr_renderer* r, FrameSlot& F, const srr_params* p, const srr_adaptive_params* a,
                                  const PathsSetup& ps, bool identity, int64_t npix, size_t win_cap, float* d_mean,
                                  int32_t* d_count, srr_adaptive_stats* stats, std::string& err) {
  AdaptiveState& A = r->adaptive;
  hipStream_t st = F.st;
  const int budget = p->spp;
  const int32_t* shard_pixels = identity ? nullptr : r->pixels.get();
  const AdaptiveRule rule{budget, a->min_spp, a->rel_tol, a->abs_eps};
  int32_t* lvl = A.lvl.get();
  srr_adaptive_stats s{};
  SpecCall sc = spec_call(A, a);
  RCHK(hipMemsetAsync(F.ctr.get(), 0, kPathsCtrWords * sizeof(unsigned long long), st));
  if (sc.on) RCHK(hipMemsetAsync(A.spec_ctr.get(), 0, kSpecWords * sizeof(unsigned long long), st));
  RCHK(hipEventRecord(F.ev_beg, st));
  bool first_launch = true;
  int prev_level = -1;
  for (;;) {
    launch_adaptive_level_select((int)npix, A.count.get(), A.mom.get(), rule, A.live.get(), A.keep.get(), lvl, st);
    launch_adaptive_compact(A.keep.get(), nullptr, (int)npix, shard_pixels, A.blk.get(), A.slot[0].get(),
                            A.pixel[0].get(), lvl + kLvlActive, st);
    // the one host round trip of a pass: the active count sizes the launch, the level is its s_base
    RCHK(hipMemcpyAsync(A.lvl_host.get(), lvl, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    RCHK(hipStreamSynchronize(st));
    const int64_t n_act = A.lvl_host.get()[kLvlActive];
    const int n = A.lvl_host.get()[kLvlLevel];
    if (n_act == 0 && n == INT_MAX) break;  // every slot is retired
    // a live slot holds fewer samples than the budget, and a pass raises the least live count
    if (n_act < 1 || n_act > npix || n < 0 || n >= budget || n <= prev_level) {
      err = "adaptive level selection returned " + std::to_string(n_act) + " of " + std::to_string(npix) +
            " slots at " + std::to_string(n) + " samples (budget " + std::to_string(budget) + ")";
      return SRR_EIO;
    }
    prev_level = n;
    const int w = spec_width(sc, a, n_act, n, budget), n_new = n + w;
    // several batches in one pass: the fold asks the rule at every batch boundary, and the
    // next k_adaptive_level finds the slots that stopped retired, from the same moments
    const bool spec = w > a->batch_spp;
    int W = (int)std::min<int64_t>(window_samples(ps, n_act, w), (int64_t)(win_cap / (size_t)n_act));
    if (W < w && W >= 16) W &= ~3;
    for (int s0 = 0; s0 < w; s0 += W) {
      const int Wn = std::min(W, w - s0);
      const PathWork pw = paths_work(r, F, p, ps, A.pixel[0].get(), n_act, n + s0, Wn);
      if (!first_launch) RCHK(hipMemsetAsync(pw.cursor, 0, sizeof(unsigned long long), st));  // first: zeroed with ctr
      first_launch = false;
      if (launch_paths(r->view, pw, r->diffuse_only ? 0 : 1, st) != 0) {
        err = "k_paths refused the launch";  // (stack_cap was checked before the first pass)
        return SRR_EINVAL;
      }
      sc.windows += 1;
      if (spec) {
        spec_fold(r, F, a, A.slot[0].get(), n_act, n, w, s0, Wn, budget, d_mean);
        continue;
      }
      AdaptiveFold f{};
      f.sample = F.sample.get();
      f.active_slot = A.slot[0].get();
      f.n_active = (int)n_act;
      f.spp_w = Wn;
      f.sums = r->acc.get();
      f.mom = A.mom.get();
      f.init = n + s0 == 0;
      // the fold's own verdict is not used: with the budget at n_new its last window writes
      // every active slot's count (and a mean that k_adaptive_finish writes again)
      f.decide = s0 + Wn >= w;
      f.n_new = n_new;
      f.budget = n_new;
      f.rel_tol = a->rel_tol;
      f.abs_eps = a->abs_eps;
      f.keep = A.keep.get();
      f.mean = d_mean;
      f.count = A.count.get();
      launch_adaptive_fold(f, st);
    }
    s.passes += 1;
    sc.traced += n_act * w;
  }
  launch_adaptive_finish((int)npix, r->acc.get(), A.count.get(), budget, d_mean, d_count, lvl, st);
  RCHK(hipMemcpyAsync(A.lvl_host.get(), lvl, kLvlWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (sc.on)
    RCHK(hipMemcpyAsync(A.spec_ctr_host.get(), A.spec_ctr.get(), kSpecWords * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost, st));
  const int rc = adaptive_frame_end(F, s, nullptr, err);
  if (rc < 0) return rc;
  spec_frame_end(A, sc, s, nullptr);
  s.pixels_retired = A.lvl_host.get()[kLvlBelow];
  if (stats) {
    s.struct_size = stats->struct_size;
    *stats = s;
  }
  return 0;
}

// resume: continue the renderer's adaptive state (capi.cpp has checked that it is valid and
// belongs to this frame) instead of starting from sample 0
int render_adaptive(srr_renderer* r, const srr_params* p, const srr_adaptive_params* a, const int32_t* pix,
                    int64_t npix, float* d_mean, int32_t* d_count, srr_adaptive_stats* stats, bool resume,
                    std::string& err) {
  if (const char* e = getenv("SRR_ENGINE"); e && !strcmp(e, "wave")) {
    err = "srr_render_adaptive: path engine only (SRR_ENGINE=wave is set)";
    return SRR_EINVAL;
  }
  // the state is this frame's from here on, and valid once it succeeds
  r->adaptive.valid_npix = 0;
  r->adaptive.sums_valid = false;
  r->adaptive.spec_windows = -1;  // (srr_adaptive_last_spec_stats: none until this call succeeds)
  RCHK(hipSetDevice(r->device));
  // the rgb sums of the pass loop live in the progressive accumulator: whatever it
  // held is gone, and what this frame leaves (pixels of different sample counts) is
  // nothing a SRR_FLAG_CONTINUE render may build on
  r->acc_npix = 0;
  bool identity = false;
  {
    const int rc = paths_stage(r, p, pix, npix, identity, err);
    if (rc < 0) return rc;
  }
  FrameSlot& F = r->sync_slot;
  {
    const int rc = slot_init(F, r->acc_st, err);
    if (rc < 0) return rc;
  }
  PathsSetup ps;
  {
    const int rc = paths_prepare(r, F, p->max_depth, ps, err);
    if (rc < 0) return rc;
  }
  if (ps.stack_cap > paths_kernel_stack()) {
    err = "k_paths refused: stack_cap " + std::to_string(ps.stack_cap) +
          " exceeds the kernel build's LDS stack (a host and kernels built with different SRR_KSTACK)";
    return SRR_EINVAL;
  }
  // the first pass has the most paths: its window serves every later one
  size_t win_cap = (size_t)npix * window_samples(ps, npix, std::min(a->batch_spp, p->spp));
  if (const SpecCall sc = spec_call(r->adaptive, a); sc.on) {
    // the widest pass the schedule can produce: n_act slots get at most w_max samples each and,
    // beyond one batch, at most fill_paths paths together (a pass that still does not fit
    // is cut into sample windows, like any other)
    const int w_max = (int)std::min<int64_t>((int64_t)(sc.pass_spp_max / a->batch_spp) * a->batch_spp, p->spp);
    const size_t fill = (size_t)(sc.fill_paths ? sc.fill_paths : kAdaptiveFillDefault);
    win_cap = std::max(win_cap, std::min((size_t)npix * window_samples(ps, npix, w_max), fill));
  }
  if (win_cap >= ((size_t)1 << 31)) {
    err = "frame too large for one sample window (npix >= 2^31)";
    return SRR_EINVAL;
  }
  {
    const int rc = ensure_window(r, F, win_cap, err);
    if (rc < 0) return rc;
  }
  {
    const int rc = ensure_adaptive(r->adaptive, (size_t)npix, err);
    if (rc < 0) return rc;
  }
  const int rc = (resume ? adaptive_resume_passes : adaptive_passes)(r, F, p, a, ps, identity, npix, win_cap, d_mean,
                                                                    d_count, stats, err);
  if (rc < 0) (void)hipStreamSynchronize(F.st);  // passes already enqueued must not outlive the error
  if (rc == 0) {
    AdaptiveState& A = r->adaptive;
    A.valid_npix = npix;
    A.sums_valid = true;
    const int key[5] = {p->nx, p->ny, p->shard_index, p->shard_count, p->tile};
    std::copy(key, key + 5, A.key);
  }
  return rc;
}

int adaptive_state_get(srr_renderer* r, float* sums, float* mom, int32_t* count, std::string& err) {
  const AdaptiveState& A = r->adaptive;
  const size_t n = (size_t)A.valid_npix;
  RCHK(hipSetDevice(r->device));
  // (every frame and every set has synchronised its stream before it returned)
  if (sums) RCHK(hipMemcpy(sums, r->acc.get(), 3 * n * sizeof(float), hipMemcpyDeviceToHost));
  if (mom) RCHK(hipMemcpy(mom, A.mom.get(), n * sizeof(float2), hipMemcpyDeviceToHost));
  if (count) RCHK(hipMemcpy(count, A.count.get(), n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return 0;
}

int adaptive_state_set(srr_renderer* r, const srr_params* p, const float* sums, const float* mom,
                       const int32_t* count, int64_t npix, std::string& err) {
  AdaptiveState& A = r->adaptive;
  A.valid_npix = 0;  // valid again once every copy below has succeeded
  A.sums_valid = false;
  RCHK(hipSetDevice(r->device));
  drain_async(r);  // frames in flight read the pixel list this may reallocate
  r->acc_npix = 0;  // the sums are an adaptive frame's: nothing a SRR_FLAG_CONTINUE render may build on
  RMEM(ensure_pixels(r, npix), "pixel list and running sums");
  {
    const int rc = ensure_adaptive(A, (size_t)npix, err);
    if (rc < 0) return rc;
  }
  RCHK(hipMemcpy(r->acc.get(), sums, 3 * (size_t)npix * sizeof(float), hipMemcpyHostToDevice));
  RCHK(hipMemcpy(A.mom.get(), mom, (size_t)npix * sizeof(float2), hipMemcpyHostToDevice));
  RCHK(hipMemcpy(A.count.get(), count, (size_t)npix * sizeof(int32_t), hipMemcpyHostToDevice));
  A.valid_npix = npix;
  A.sums_valid = true;
  const int key[5] = {p->nx, p->ny, p->shard_index, p->shard_count, p->tile};
  std::copy(key, key + 5, A.key);
  return 0;
}

int adaptive_variance(srr_renderer* r, const int32_t* d_count, float* d_var, std::string& err) {
  const AdaptiveState& A = r->adaptive;
  RCHK(hipSetDevice(r->device));
  hipStream_t st = r->sync_slot.st;  // the stream the frame's folds ran on
  launch_adaptive_variance((int)A.valid_npix, A.mom.get(), d_count, d_var, st);
  RCHK(hipGetLastError());
  RCHK(hipStreamSynchronize(st));
  return 0;
}

// srr_render_device_async: a fresh frame (no CONTINUE, KEEP_PATHS, COUNT_VISITS or
// wavefront engine) on one of the renderer's two frame slots, each with its own
// stream, sums and buffers, so the next frame's persistent blocks take the CUs
// the previous frame's drain frees.  Returns at once; srr_render_wait reads it.
int render_device_async(srr_renderer* r, const srr_params* p, const int32_t* pix, int64_t npix, float* d_mean,
                        int64_t* ticket, std::string& err) {
  if (p->flags & (SRR_FLAG_CONTINUE | SRR_FLAG_KEEP_PATHS | SRR_FLAG_COUNT_VISITS | SRR_FLAG_WAVEFRONT)) {
    err = "srr_render_device_async: fresh path-engine frames only (no CONTINUE, KEEP_PATHS, COUNT_VISITS, WAVEFRONT)";
    return SRR_EINVAL;
  }
  if (const char* e = getenv("SRR_ENGINE"); e && !strcmp(e, "wave")) {
    err = "srr_render_device_async: SRR_ENGINE=wave is synchronous only";
    return SRR_EINVAL;
  }
  RCHK(hipSetDevice(r->device));
  FrameSlot& F = r->async_slots[r->next_ticket % 2];
  if (F.busy) finish_slot(r, F);  // the slot's previous frame has not been waited for: finish it now
  bool identity = false;
  {
    const int rc = paths_stage(r, p, pix, npix, identity, err);
    if (rc < 0) return rc;
  }
  {
    const int rc = slot_init(F, nullptr, err);
    if (rc < 0) return rc;
  }
  RMEM(F.acc.grow(3 * (size_t)npix), "async frame sums");
  // the caller's stream order: the frame starts after what the legacy stream holds
  RCHK(hipEventRecord(r->ev_async_in, nullptr));
  RCHK(hipStreamWaitEvent(F.st, r->ev_async_in, 0));
  {
    const int rc = paths_enqueue(r, F, p, identity, npix, F.acc.get(), true, p->spp, d_mean, false, err);
    if (rc < 0) {
      // windows already on F.st read the slot's buffers: drain them before the slot is reused
      (void)hipStreamSynchronize(F.st);
      return rc;
    }
  }
  F.ticket = r->next_ticket++;
  F.busy = true;
  *ticket = F.ticket;
  return 0;
}

hipEvent_t render_ticket_event(srr_renderer* r, int64_t ticket) {
  for (FrameSlot& F : r->async_slots)
    if (F.busy && F.ticket == ticket) return F.ev_end;
  return nullptr;
}

int render_wait(srr_renderer* r, int64_t ticket, srr_stats* stats, std::string& err) {
  RCHK(hipSetDevice(r->device));
  for (size_t k = 0; k < r->done_tickets.size(); ++k)
    if (r->done_tickets[k].ticket == ticket) {
      const DoneTicket d = r->done_tickets[k];
      r->done_tickets.erase(r->done_tickets.begin() + k);
      if (stats) *stats = d.stats;
      err = d.err;
      return d.rc;
    }
  for (FrameSlot& F : r->async_slots)
    if (F.busy && F.ticket == ticket) {
      F.busy = false;
      srr_params none{};
      return paths_finish(r, F, &none, stats, err);
    }
  err = "srr_render_wait: unknown or already waited ticket " + std::to_string(ticket);
  return SRR_EINVAL;
}

int render_device(srr_renderer* r, const srr_params* p, const int32_t* pix, int64_t npix, float* d_mean,
                  srr_stats* stats, std::string& err) {
  static const bool wave_env = [] {
    const char* e = getenv("SRR_ENGINE");
    return e && !strcmp(e, "wave");
  }();
  const bool wave_engine = wave_env || (p->flags & SRR_FLAG_WAVEFRONT);
  // every buffer either engine allocates belongs to the renderer's device,
  // whatever device the caller has current
  RCHK(hipSetDevice(r->device));
  // the path engine stages the world tables in LDS when they fit
  // (kernels.hip kWorldLdsBytes) and reads them from global memory otherwise
  if (!wave_engine && !(p->flags & SRR_FLAG_COUNT_VISITS))
    return render_paths(r, p, pix, npix, d_mean, stats, err);
  drain_async(r);  // the wavefront engine restages the pixel list
  const bool keep = (p->flags & SRR_FLAG_KEEP_PATHS) != 0;
  const int R = kRegionsPerLane;
  hipStream_t ast = r->acc_st;
  unsigned long long* visits = nullptr;
  if (p->flags & SRR_FLAG_COUNT_VISITS) {
    RMEM(r->visits.grow(kVisitWords), "visit counters");
    visits = r->visits.get();
    RCHK(hipMemset(visits, 0, kVisitWords * sizeof(unsigned long long)));
  }
  // frame buffers
  if (pix) RMEM(stage_pixels(r, pix, npix, false), "pixel list and running sums");
  else if (r->pix_identity) {  // the path engine skipped the upload of an identity list
    std::vector<int32_t> id((size_t)npix);
    for (int64_t i = 0; i < npix; ++i) id[i] = (int32_t)i;
    RMEM(stage_pixels(r, id.data(), npix, false), "pixel list and running sums");
  }
  // Sobol points of the global sample range [sample_begin, sample_begin + spp):
  // the set is a prefix-stable sequence, so a sample shard reads its own slice.
  RMEM(ensure_sobol(r->sobol, r->sobol_n, p->sample_begin + p->spp), "Sobol points");
  if (keep) {
    const int rc = ensure_kept(r, (size_t)npix * p->spp, err);
    if (rc < 0) return rc;
  }
  // Batches: (pixel chunk, sample chunk) in the order every pixel must see its
  // samples accumulated.
  int64_t N = p->batch_paths > 0 ? p->batch_paths : (int64_t)1 << 20;
  int64_t pix_chunk = std::min<int64_t>(npix, N);
  int S = (int)std::max<int64_t>(1, std::min<int64_t>(p->spp, N / pix_chunk));
  const int64_t region = pix_chunk * S;
  std::vector<BatchInfo> batches;
  for (int64_t p0 = 0; p0 < npix; p0 += pix_chunk) {
    int np = (int)std::min<int64_t>(pix_chunk, npix - p0);
    for (int s0 = 0; s0 < p->spp; s0 += S) {
      BatchInfo B{};
      B.pixels = r->pixels.get();
      B.sobol = r->sobol.get() + 2 * (size_t)p->sample_begin;
      B.s_base = p->sample_begin;
      B.p0 = (int)p0;
      B.spp_batch = std::min(S, p->spp - s0);
      B.n_paths = np * B.spp_batch;
      B.s0 = s0;
      B.nx = p->nx;
      B.ny = p->ny;
      B.base_seed = p->base_seed;
      batches.push_back(B);
    }
  }
  const size_t nb = batches.size();
  // lanes: enough paths in flight to fill the GPU, without idle lanes on small frames
  int lanes = (int)std::min<size_t>(nb, (size_t)r->n_lanes);
  lanes = std::max(1, lanes);
  size_t cap = (size_t)region * R;
  if (cap > (size_t)INT32_MAX / 4) {
    err = "batch_paths too large";
    return SRR_EINVAL;
  }
  for (int l = 0; l < lanes; ++l) {
    int rc = ensure_lane(r->lanes[l], cap, p->max_depth, keep, err);
    if (rc < 0) return rc;
  }
  RCHK(hipDeviceSynchronize());
  {
    const int rc = begin_accum(r, p, npix, ast, err);
    if (rc < 0) return rc;
  }
  AccCommit commit{r};
  RCHK(hipEventRecord(r->ev_beg, ast));
  for (int l = 0; l < lanes; ++l) {
    Lane& L = r->lanes[l];
    L.n = 0;
    L.cur = 0;
    L.pending = false;
    L.trace_ms = L.shade_ms = 0;
    for (int k = 0; k < R; ++k) {
      L.reg_batch[k] = -1;
      L.acc_pending[k] = false;
    }
    if (!keep) {
      L.P.raw = nullptr;
      L.P.rays = nullptr;
    }
    RCHK(hipStreamWaitEvent(L.st, r->ev_beg, 0));
  }
  std::vector<int> b_lane(nb, -1), b_reg(nb, -1);
  std::vector<char> b_done(nb, 0);
  srr_stats s{};
  size_t next_batch = 0, acc_head = 0;
  const int64_t target = std::max<int64_t>(region, (int64_t)3 << 20) / 2;  // paths in flight per lane

  while (acc_head < nb) {
    bool progress = false;
    for (int l = 0; l < lanes; ++l) {
      Lane& L = r->lanes[l];
      if (L.pending) {
        hipError_t q = hipEventQuery(L.ev_rb);
        if (q == hipErrorNotReady) continue;
        RCHK(q);
        L.pending = false;
        progress = true;
        float ms = 0;
        RCHK(hipEventElapsedTime(&ms, L.ev_t0, L.ev_t1));
        L.trace_ms += ms;
        RCHK(hipEventElapsedTime(&ms, L.ev_t1, L.ev_s1));
        L.shade_ms += ms;
        L.n = L.rb.get()[R];
        for (int k = 0; k < R; ++k)
          if (L.reg_batch[k] >= 0 && !b_done[L.reg_batch[k]] && L.rb.get()[k] == 0) {
            b_done[L.reg_batch[k]] = 1;
            RCHK(hipEventRecord(L.done_ev[k], L.st));
          }
      }
      // refill free regions with new batches
      while (next_batch < nb && L.n < target) {
        int fr = -1;
        for (int k = 0; k < R; ++k)
          if (L.reg_batch[k] < 0) {
            fr = k;
            break;
          }
        if (fr < 0) break;
        if (L.acc_pending[fr]) {  // the region's previous batch is still being accumulated
          RCHK(hipStreamWaitEvent(L.st, L.acc_ev[fr], 0));
          L.acc_pending[fr] = false;
        }
        BatchInfo& B = batches[next_batch];
        B.active = L.act[L.cur];
        B.act0 = L.n;
        B.slot0 = (int)(fr * region);
        B.count = L.cnt.get() + L.cur;
        launch_raygen(r->view, L.P, B, L.st);
        L.n += B.n_paths;
        L.reg_batch[fr] = (int)next_batch;
        b_lane[next_batch] = l;
        b_reg[next_batch] = fr;
        s.paths += B.n_paths;
        ++next_batch;
        progress = true;
      }
      if (L.n > 0) {
        int n = L.n, cur = L.cur;
        int* alive = L.cnt.get() + 2;
        int* fam = alive + R;
        RCHK(hipMemsetAsync(L.cnt.get() + (cur ^ 1), 0, sizeof(int), L.st));
        int* fetch = alive + R + 4;  // persistent trace's ray cursor
        RCHK(hipMemsetAsync(alive, 0, (R + 5) * sizeof(int), L.st));
        RCHK(hipEventRecord(L.ev_t0, L.st));
        launch_trace(r->view, L.P, L.act[cur], L.cnt.get() + cur, n, L.lists, (int)L.cap, fam, fetch, p->max_depth, visits,
                     L.st);
        RCHK(hipEventRecord(L.ev_t1, L.st));
        launch_shade(r->view, L.P, L.lists, (int)L.cap, fam, L.act[cur ^ 1], L.cnt.get() + (cur ^ 1), alive, (int)region,
                     n, p->max_depth, L.st);
        RCHK(hipEventRecord(L.ev_s1, L.st));
        RCHK(hipMemcpyAsync(L.rb.get(), alive, R * sizeof(int), hipMemcpyDeviceToHost, L.st));
        RCHK(hipMemcpyAsync(L.rb.get() + R, L.cnt.get() + (cur ^ 1), sizeof(int), hipMemcpyDeviceToHost, L.st));
        RCHK(hipEventRecord(L.ev_rb, L.st));
        L.pending = true;
        L.cur ^= 1;
        s.world_rays += n;
        s.trace_launches += 1;
        s.bounces += 1;
        progress = true;
      }
    }
    // accumulate finished batches strictly in batch order, on the acc stream
    while (acc_head < next_batch && b_done[acc_head]) {
      Lane& L = r->lanes[b_lane[acc_head]];
      int rg = b_reg[acc_head];
      BatchInfo& B = batches[acc_head];
      RCHK(hipStreamWaitEvent(ast, L.done_ev[rg], 0));
      launch_accumulate(L.P, B, r->acc.get(), ast);
      if (keep) {  // region paths are [pixel][sample-in-batch]; the frame keeps [pixel][spp]
        int np = B.n_paths / B.spp_batch, Sb = B.spp_batch;
        RCHK(hipMemcpy2DAsync(r->raw_all.get() + 3 * ((size_t)B.p0 * p->spp + B.s0), 3 * sizeof(float) * p->spp,
                              L.P.raw + 3 * (size_t)B.slot0, 3 * sizeof(float) * Sb, 3 * sizeof(float) * Sb, np,
                              hipMemcpyDeviceToDevice, ast));
        RCHK(hipMemcpy2DAsync(r->rays_all.get() + ((size_t)B.p0 * p->spp + B.s0), p->spp, L.P.rays + B.slot0, Sb, Sb, np,
                              hipMemcpyDeviceToDevice, ast));
      }
      RCHK(hipEventRecord(L.acc_ev[rg], ast));
      L.acc_pending[rg] = true;
      L.reg_batch[rg] = -1;
      ++acc_head;
      progress = true;
    }
    if (!progress) std::this_thread::yield();
  }
  const int64_t acc_total = r->acc_samples + p->spp;
  if (p->flags & SRR_FLAG_SUMS)
    RCHK(hipMemcpyAsync(d_mean, r->acc.get(), 3 * (size_t)npix * sizeof(float), hipMemcpyDeviceToDevice, ast));
  else
    launch_finish(r->acc.get(), d_mean, npix, (int)acc_total, ast);
  RCHK(hipEventRecord(r->ev_end, ast));
  RCHK(hipStreamSynchronize(ast));
  RCHK(hipGetLastError());
  r->acc_samples = acc_total;
  commit.ok = true;
  float total = 0;
  RCHK(hipEventElapsedTime(&total, r->ev_beg, r->ev_end));
  s.total_ms = total;
  for (int l = 0; l < lanes; ++l) {
    s.trace_ms += r->lanes[l].trace_ms;
    s.shade_ms += r->lanes[l].shade_ms;
  }
  if (getenv("SRR_TIMING")) dump_trace_timing();
  if (visits) {
    unsigned long long v[kVisitWords];
    RCHK(hipDeviceSynchronize());
    RCHK(hipMemcpy(v, visits, sizeof(v), hipMemcpyDeviceToHost));
    if (getenv("SRR_HIST")) {  // diagnostics: node steps per ray / per wave
      for (int h = 0; h < 2; ++h) {
        fprintf(stderr, h ? "steps per wave (max):" : "steps per ray:");
        for (int b = 0; b < 64; ++b)
          if (v[3 + 64 * h + b]) fprintf(stderr, " %d:%llu", b, v[3 + 64 * h + b]);
        fprintf(stderr, "\n");
      }
    }
    s.box_tests = (int64_t)v[0];
    s.tri_tests = (int64_t)v[1];
    s.stack_overflows = (int64_t)v[2];
  }
  if (stats) *stats = s;
  return 0;
}

// ---- first-hit AOVs
// Per path in flight: PathState's depth-0 members (rays 32 B, RNG 16 B, depth 4 B, spec
// 8 B, hit record 48 B), the active list (4 B), the family lists (16 B) and the values
// (32 B): 160 B, 160 MiB at the default batch of 2^20 paths.  srr_render_aov_through adds
// 12 B + 12 B x max_depth per path of its own, smaller default batch (ensure_aov_through).
static int ensure_aov(AovState& A, size_t n, size_t npix, int n_sobol, std::string& err) {
  if (!A.st) RCHK(hipStreamCreateWithFlags(&A.st, hipStreamNonBlocking));
  if (n > A.cap) {
    A.bufs.clear();
    A.cap = 0;
    RMEM(alloc_depth0(A.bufs, A.P, n), "AOV path state");
    RMEM(A.bufs.add(&A.active, n), "AOV active list");
    RMEM(A.bufs.add(&A.lists, 4 * n), "AOV family lists");
    RMEM(A.bufs.add(&A.cnt, 8), "AOV counters");
    RMEM(A.bufs.add(&A.val, 2 * n), "AOV values");
    A.cap = n;
  }
  RMEM(grow_pair(A.pixels, npix, A.acc, 8 * npix), "AOV pixel list and sums");
  RMEM(ensure_sobol(A.sobol, A.sobol_n, n_sobol), "AOV Sobol points");
  return 0;
}

// one batch of the AOV calls: pixels [p0, p0 + np) x samples [s0, s0 + min(S, spp - s0)),
// laid out from slot 0 in A.active
static BatchInfo aov_batch(const AovState& A, const srr_params* p, int p0, int np, int s0, int S) {
  BatchInfo B{};
  B.active = A.active;
  B.count = A.cnt;
  B.act0 = 0;
  B.slot0 = 0;
  B.pixels = A.pixels.get();
  B.sobol = A.sobol.get() + 2 * (size_t)p->sample_begin;
  B.s_base = p->sample_begin;
  B.p0 = p0;
  B.spp_batch = std::min(S, p->spp - s0);
  B.n_paths = np * B.spp_batch;
  B.s0 = s0;
  B.nx = p->nx;
  B.ny = p->ny;
  B.base_seed = p->base_seed;
  return B;
}
// ... and the fold of its values
static AovFold aov_fold(const AovState& A, const srr_params* p, const BatchInfo& B, int np, float* d_albedo,
                        float* d_normal, float* d_depth) {
  AovFold F{};
  F.val = (const float*)A.val;
  F.np = np;
  F.spp_b = B.spp_batch;
  F.acc = A.acc.get();
  F.init = B.s0 == 0;
  F.finish = B.s0 + B.spp_batch == p->spp;
  F.ns = p->spp;
  F.p0 = B.p0;
  F.albedo = d_albedo;
  F.normal = d_normal;
  F.depth = d_depth;
  return F;
}

// srr_render_aov_emission's own buffers: 16 B per path of the call's batch for the emission
// values (the 8-word `val` layout and the other calls' state stay as they are) and 16 B per
// pixel of sums.  Allocated the first time SRR_AOV_EMISSION is asked for.
static int ensure_aov_emission(AovState& A, size_t n, size_t npix, std::string& err) {
  RMEM(A.emit.grow(at_least_16_bytes<float4>(n)), "AOV emission values");
  RMEM(A.acc_e.grow(at_least_16_bytes<float>(4 * npix)), "AOV emission sums");
  return 0;
}
static AovEmissionFold aov_fold_emission(const AovState& A, const srr_params* p, const BatchInfo& B, int np,
                                         const int32_t* d_count, float* d_emission) {
  AovEmissionFold F{};
  F.emit = (const float*)A.emit.get();
  F.np = np;
  F.spp_b = B.spp_batch;
  F.s0 = B.s0;
  F.acc = A.acc_e.get() + 4 * (size_t)B.p0;
  F.ns = p->spp;
  F.p0 = B.p0;
  F.count = d_count;
  F.emission = d_emission;
  return F;
}

// srr_render_aov (d_emission == nullptr) and the first-hit form of srr_render_aov_emission
static int aov_first_hit(srr_renderer* r, const srr_params* p, const int32_t* pix, int64_t npix, float* d_albedo,
                         float* d_normal, float* d_depth, float* d_emission, const int32_t* d_count,
                         std::string& err) {
  RCHK(hipSetDevice(r->device));
  // batches as in render_device: a pixel chunk x a sample chunk of at most N paths;
  // a pixel chunk sees all its sample chunks, in order, before the next one starts
  const int64_t N = p->batch_paths > 0 ? p->batch_paths : (int64_t)1 << 20;
  const int64_t pix_chunk = std::min<int64_t>(npix, N);
  const int S = (int)std::max<int64_t>(1, std::min<int64_t>(p->spp, N / pix_chunk));
  const int64_t region = pix_chunk * S;
  if (region > INT32_MAX / 8) {
    err = "batch_paths too large";
    return SRR_EINVAL;
  }
  AovState& A = r->aov;
  {  // every allocation comes before the first launch
    int rc = ensure_aov(A, (size_t)region, (size_t)npix, p->sample_begin + p->spp, err);
    if (rc == 0 && d_emission) rc = ensure_aov_emission(A, (size_t)region, (size_t)npix, err);
    if (rc < 0) return rc;
  }
  const bool old_three = d_albedo || d_normal || d_depth;
  RCHK(hipMemcpyAsync(A.pixels.get(), pix, npix * sizeof(int32_t), hipMemcpyHostToDevice, A.st));
  for (int64_t p0 = 0; p0 < npix; p0 += pix_chunk) {
    const int np = (int)std::min<int64_t>(pix_chunk, npix - p0);
    for (int s0 = 0; s0 < p->spp; s0 += S) {
      const BatchInfo B = aov_batch(A, p, (int)p0, np, s0, S);
      RCHK(hipMemsetAsync(A.cnt, 0, 8 * sizeof(int32_t), A.st));
      launch_raygen(r->view, A.P, B, A.st);
      launch_trace(r->view, A.P, A.active, A.cnt, B.n_paths, A.lists, (int)A.cap, A.cnt + 1, A.cnt + 5, p->max_depth,
                   nullptr, A.st);
      launch_aov_eval(r->view, A.P, B.n_paths, A.val, d_emission ? A.emit.get() : nullptr, A.st);
      if (old_three) launch_aov_fold(aov_fold(A, p, B, np, d_albedo, d_normal, d_depth), A.st);
      if (d_emission) launch_aov_fold_emission(aov_fold_emission(A, p, B, np, d_count, d_emission), A.st);
    }
  }
  RCHK(hipGetLastError());
  RCHK(hipStreamSynchronize(A.st));
  return 0;
}

int render_aov(srr_renderer* r, const srr_params* p, const int32_t* pix, int64_t npix, float* d_albedo,
               float* d_normal, float* d_depth, std::string& err) {
  return aov_first_hit(r, p, pix, npix, d_albedo, d_normal, d_depth, nullptr, nullptr, err);
}

// ---- through-specular AOVs
// Per path of the call's batch, besides ensure_aov's 160 B: the second active list (4 B), the
// running depth and record count (8 B) and max_depth metal records of 12 B: 172 B + 12 B x
// max_depth, 940 B at the largest max_depth of 64.  The default batch keeps that within
// kAovThroughBytes: 2^20 paths up to max_depth 7, 285,569 at 64.  These buffers are sized and
// strided by the call's own batch and replaced, not grown, when it needs more; only ensure_aov's
// buffers, shared with srr_render_aov, keep the largest batch either call has used.
// With the emission (srr_render_aov_emission) a path holds 16 B more, 188 B + 12 B x max_depth,
// and that call's default batch keeps it within the same bound.
constexpr int64_t kAovThroughBytes = (int64_t)256 << 20;
static int64_t aov_through_path_bytes(int max_depth, bool emission) {
  return (emission ? 188 : 172) + 12 * (int64_t)max_depth;
}

static int ensure_aov_through(AovState& A, size_t n, int depth, std::string& err) {
  const size_t words = 3 * n * (size_t)std::max(depth, 1);
  if (n > A.t_cap || words > A.t_rec) {
    A.t_bufs.clear();
    A.t_cap = A.t_rec = 0;
    RMEM(A.t_bufs.add(&A.next, n), "AOV second active list");
    RMEM(A.t_bufs.add(&A.chain, n), "AOV chain state");
    RMEM(A.t_bufs.add(&A.rec, words), "AOV metal records");
    A.t_cap = n;
    A.t_rec = words;
  }
  RMEM(A.n_host.grow(4), "AOV active count's host mirror");
  return 0;
}

// srr_render_aov_through (d_emission == nullptr) and the through-specular form of
// srr_render_aov_emission
static int aov_through(srr_renderer* r, const srr_params* p, const int32_t* pix, int64_t npix, float* d_albedo,
                       float* d_normal, float* d_depth, float* d_emission, const int32_t* d_count,
                       srr_aov_stats* stats, std::string& err) {
  RCHK(hipSetDevice(r->device));
  const int64_t N =
      p->batch_paths > 0
          ? p->batch_paths
          : std::min<int64_t>((int64_t)1 << 20,
                              kAovThroughBytes / aov_through_path_bytes(p->max_depth, d_emission != nullptr));
  const int64_t pix_chunk = std::min<int64_t>(npix, N);
  const int S = (int)std::max<int64_t>(1, std::min<int64_t>(p->spp, N / pix_chunk));
  const int64_t region = pix_chunk * S;
  if (region > INT32_MAX / 8) {
    err = "batch_paths too large";
    return SRR_EINVAL;
  }
  AovState& A = r->aov;
  {  // every allocation comes before the first launch
    int rc = ensure_aov(A, (size_t)region, (size_t)npix, p->sample_begin + p->spp, err);
    if (rc == 0) rc = ensure_aov_through(A, (size_t)region, p->max_depth, err);
    if (rc == 0 && d_emission) rc = ensure_aov_emission(A, (size_t)region, (size_t)npix, err);
    if (rc < 0) return rc;
  }
  const bool old_three = d_albedo || d_normal || d_depth;
  srr_aov_stats s{};
  RCHK(hipMemcpyAsync(A.pixels.get(), pix, npix * sizeof(int32_t), hipMemcpyHostToDevice, A.st));
  for (int64_t p0 = 0; p0 < npix; p0 += pix_chunk) {
    const int np = (int)std::min<int64_t>(pix_chunk, npix - p0);
    for (int s0 = 0; s0 < p->spp; s0 += S) {
      const BatchInfo B = aov_batch(A, p, (int)p0, np, s0, S);
      RCHK(hipMemsetAsync(A.cnt, 0, 8 * sizeof(int32_t), A.st));
      launch_raygen(r->view, A.P, B, A.st);
      s.paths += B.n_paths;
      // the bounce loop: the lists alternate, their counts are cnt[0] and cnt[6]; the host
      // reads each bounce's survivor count, which sizes the next launch and ends the loop
      int32_t* list[2] = {A.active, A.next};
      int32_t* count[2] = {A.cnt, A.cnt + 6};
      int n = B.n_paths;
      for (int bounce = 0, cur = 0; n > 0; ++bounce, cur ^= 1) {
        if (bounce > p->max_depth) {
          err = "through-specular AOVs: a path outlived max_depth";
          (void)hipStreamSynchronize(A.st);
          return SRR_EIO;
        }
        RCHK(hipMemsetAsync(A.cnt + 1, 0, 5 * sizeof(int32_t), A.st));  // family counts, fetch
        RCHK(hipMemsetAsync(count[cur ^ 1], 0, sizeof(int32_t), A.st));
        launch_trace(r->view, A.P, list[cur], count[cur], n, A.lists, (int)A.cap, A.cnt + 1, A.cnt + 5, p->max_depth,
                     nullptr, A.st);
        AovChain C{};
        C.active = list[cur];
        C.count = count[cur];
        C.next = list[cur ^ 1];
        C.next_count = count[cur ^ 1];
        C.max_depth = p->max_depth;
        C.cap = (int)region;
        C.chain = A.chain;
        C.rec = A.rec;
        C.val = A.val;
        C.emit = d_emission ? A.emit.get() : nullptr;
        launch_aov_chain(r->view, A.P, C, n, A.st);
        RCHK(hipMemcpyAsync(A.n_host.get(), count[cur ^ 1], sizeof(int32_t), hipMemcpyDeviceToHost, A.st));
        RCHK(hipStreamSynchronize(A.st));
        s.world_rays += n;
        s.longest_chain = std::max(s.longest_chain, bounce);
        n = *A.n_host.get();
        if (n < 0 || n > B.n_paths) {
          err = "through-specular AOVs: active count out of range";
          (void)hipStreamSynchronize(A.st);
          return SRR_EIO;
        }
        if (bounce == 0) s.chained_paths += n;
      }
      if (old_three) launch_aov_fold(aov_fold(A, p, B, np, d_albedo, d_normal, d_depth), A.st);
      if (d_emission) launch_aov_fold_emission(aov_fold_emission(A, p, B, np, d_count, d_emission), A.st);
    }
  }
  RCHK(hipGetLastError());
  RCHK(hipStreamSynchronize(A.st));
  if (stats) {
    s.struct_size = stats->struct_size;
    *stats = s;
  }
  return 0;
}

int render_aov_through(srr_renderer* r, const srr_params* p, const int32_t* pix, int64_t npix, float* d_albedo,
                       float* d_normal, float* d_depth, srr_aov_stats* stats, std::string& err) {
  return aov_through(r, p, pix, npix, d_albedo, d_normal, d_depth, nullptr, nullptr, stats, err);
}

int render_aov_emission(srr_renderer* r, const srr_params* p, const int32_t* pix, int64_t npix, int through,
                        float* d_albedo, float* d_normal, float* d_depth, float* d_emission, const int32_t* d_count,
                        srr_aov_stats* stats, std::string& err) {
  if (through) return aov_through(r, p, pix, npix, d_albedo, d_normal, d_depth, d_emission, d_count, stats, err);
  const int rc = aov_first_hit(r, p, pix, npix, d_albedo, d_normal, d_depth, d_emission, d_count, err);
  if (rc == 0 && stats) {  // every path is its primary ray
    const int64_t paths = npix * (int64_t)p->spp;
    *stats = srr_aov_stats{stats->struct_size, 0, paths, paths, 0};
  }
  return rc;
}

}  // namespace srr

srr_renderer::~srr_renderer() {
  if (multi) {
    srr::multi_destroy(multi);
    multi = nullptr;
  }
  (void)hipSetDevice(device);
  (void)hipDeviceSynchronize();
  // events and streams; every buffer belongs to a member, and members go after this body,
  // with the device still synchronised
  srr::slot_destroy(sync_slot);
  for (auto& F : async_slots) srr::slot_destroy(F);
  if (ev_async_in) (void)hipEventDestroy(ev_async_in);
  if (aov.st) (void)hipStreamDestroy(aov.st);
  for (auto& L : lanes) {
    for (hipEvent_t e : {L.ev_t0, L.ev_t1, L.ev_s1, L.ev_rb})
      if (e) (void)hipEventDestroy(e);
    for (int k = 0; k < srr::kRegionsPerLane; ++k) {
      if (L.done_ev[k]) (void)hipEventDestroy(L.done_ev[k]);
      if (L.acc_ev[k]) (void)hipEventDestroy(L.acc_ev[k]);
    }
    if (L.st) (void)hipStreamDestroy(L.st);
  }
  if (ev_beg) (void)hipEventDestroy(ev_beg);
  if (ev_end) (void)hipEventDestroy(ev_end);
  if (acc_st) (void)hipStreamDestroy(acc_st);
}
