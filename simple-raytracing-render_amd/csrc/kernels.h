// Device-side views of the uploaded scene and of the per-path wavefront state,
// plus the kernel launch shims (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_scene.h"

namespace srr {

struct SceneView {  // device pointers into the flattened tables (device_scene.h)
  const DObj* objs;
  int n_world;
  int has_media;
  const DXform* xforms;
  const DSphere* spheres;
  const DRect* rects;
  const DStandaloneTri* stris;
  const DMesh* meshes;
  const float4* nodes;  // 2 float4 per BVH2 node: lo (min.xyz, skip), hi (max.xyz, leaf)
  const float4* node4;  // 8 float4 per 4-wide node (device_scene.h), breadth-first per mesh
  int node4_lds;        // leading nodes the path kernel keeps in LDS (<= kPathsLdsNodes)
  int node4_total;      // BVH4 nodes of all meshes (the LDS caches take a prefix)
  const float4* node4q; // the same nodes compressed to 64 B (device_scene.h kNode4qWords), or nullptr
  int node4_lds_q;      // ...and how many of those the path kernel keeps in LDS (<= 2 kPathsLdsNodes)
  int use_q;            // k_paths traces meshes over node4q (SRR_CBVH)
  int quad_trace;       // k_paths traces meshes quad-cooperatively (BVH4 larger than an XCD's L2)
  int quad_max;         // ...when at most this many lanes of the wave enter the mesh (else per lane)
  int mesh_obj;         // the world list's one top-level mesh object, else -1 (kernels.hip world_hit: walk suspension's list mode)
  const float4* tri_pos;  // 4 float4 per triangle: p0, p1, p2, pad
  const float4* tri_edge;  // 8 float4 per triangle i: p0, e1, e2 of i and i+1 packed (renderer.cpp)
  const TriShade* tri_shade;
  const DMedium* media;
  const DObvh* obvhs;                 // object BVHs (global memory)
  const DObvhChild* obvh_children;
  const DSGroup* sgroups;             // sphere runs behind a BVH (global memory)
  const DSGItem* sg_items;
  const DMat* mats;
  const DTex* texs;
  const uint8_t* images;
  const float* perlin_ranvec;
  const int32_t* perlin_perm;
  const DLight* lights;
  int n_lights;
  float light_weight;  // hitable_list::pdf_value's weight, (float)(1.0 / n_lights) (hitable_list.h:55)
  const DCamera* cam;
  // the world traversal's and shading's small tables packed in one blob (16-B
  // aligned pieces) that the kernels copy to LDS: byte offsets of objs, xforms,
  // spheres, rects, stris, meshes, media, mats, texs, lights
  const uint4* world_blob;
  int world_words;  // 16-B words
  int world_off[10];
};

// Struct-of-arrays state of the paths of one batch (capacity N).
struct PathState {
  float4* ray_o;    // origin.xyz, time
  float4* ray_d;    // direction.xyz
  uint64_t* lcg;    // 48-bit LCG state (mathf.h:12), per path
  uint64_t* pcg;    // PCG32 state (pdf.h:20), per path
  int32_t* depth;   // the reference's *depth
  uint64_t* spec;   // bit k: bounce k was specular
  int4* hit_w;      // closest hit: object (-1 miss), primitive, t (float bits), material (-1 null)
  float4* hit_p;    // its record (k_record): p.xyz, u
  float4* hit_n;    //   normal.xyz, v
  float4* rec_a;    // [path][max_depth]: attenuation*scattering_pdf (or attenuation), pdf
  float* sample;    // [path][3] de_nan'd radiance
  float* raw;       // [path][3] radiance before de_nan (optional)
  uint8_t* rays;    // [path] world rays traced (optional)
};

struct BatchInfo {
  int32_t* active;        // active list the batch's paths are appended to
  int32_t* count;         // device count of that list, set to act0 + n_paths
  int act0;               // ... at this offset
  int slot0;              // first path-state slot of the batch's region
  const int32_t* pixels;  // shard pixel list (PPM-order indices)
  const double* sobol;    // [spp][2], already offset to global sample s_base
  int p0;                 // first shard pixel of the batch
  int n_paths;            // pixels_in_batch * spp_batch
  int s0, spp_batch;      // sample range [s0, s0 + spp_batch) of this render
  int s_base;             // global index of this render's sample 0 (sample sharding)
  int nx, ny;
  uint64_t base_seed;
};

// floor(n / d) for 0 <= n < 2^31 as (n * m) >> p with m = ceil(2^p / d),
// p = 31 + ceil(log2 d) (Granlund-Montgomery: exact for every 31-bit n; m < 2^32)
struct UDiv31 {
  uint32_t m, p;
};
inline UDiv31 make_udiv31(uint32_t d) {
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  const uint32_t p = 31 + l;
  return UDiv31{(uint32_t)(((1ull << p) + d - 1) / d), p};
}

// One window of a frame for the path-resident persistent kernel (k_paths):
// every (pixel, sample) of pixels x [0, spp_w) is a path, numbered pixel-major
// g = lp * spp_w + s (a wave's lanes take samples of one pixel: coherent first
// bounces); lanes fetch g from `cursor` as their paths finish.
struct PathWork {
  const int32_t* pixels;  // shard pixel list (PPM-order indices), nullptr = identity
  const double* sobol;    // [spp_w][2], window sample 0 first
  int npix, spp_w;
  int s_base;             // global sample index of window sample 0 (per-path seeds)
  int nx, ny;
  UDiv31 div_spp, div_nx;  // invariant divisors spp_w and nx (path index -> pixel, pixel -> i, j)
  uint64_t base_seed;
  int64_t n_paths;        // npix * spp_w
  int max_depth;
  unsigned long long* cursor;  // next path to start (device, zeroed per window)
  unsigned long long* counters;  // kPathsCtrWords words, named by PathsCtr (below)
  float* sample;          // [n_paths][3] de_nan'd radiance, index g
  float* raw;             // optional kept paths [npix][keep_spp][3] before de_nan
  uint8_t* rays;          // optional kept [npix][keep_spp] world rays per path
  int keep_spp, keep_s0;  // frame spp and this window's first sample in them
  float4* rec;            // bounce records [2][max_depth][lanes]: a survivor slot's column, then a head-pass lane's
  int lanes;              // persistent lanes (grid * block)
  int* err;               // guard bits set on an out-of-range index (never expected)
  int stack_cap;          // BVH4 traversal stack entries (kStack = 8; fewer forces the exact re-walk)
  int2* gstack;           // the stack's global extension [gstack_cap][lanes] (deep meshes), or nullptr
  int gstack_cap;
  unsigned long long* wave_times;  // diagnostics (SRR_WAVE_TIMES): per wave [start, exit] s_memrealtime, or nullptr
  int deep_tries;         // coop_mixture: failed attempts after which a path takes every free lane (32)
  float* slow_rays;       // diagnostics build (-DSRR_SLOW_RAYS=ticks): [65536][16] records of slow world hits
  unsigned* slow_count;
  // suspendable mesh walks (kernels.hip TraceCtx::walk_thr): a lane's walk, after a node
  // step, stops for this wave-iteration once at most walk_q / 64 of the wave's lanes in a
  // path are still walking (0: never); its state goes to the [3][lanes] float4 save area
  // that follows gstack's gstack_cap x lanes entries (so walks suspend only with gstack)
  int walk_q;
  // chunk-synchronous variants (kernels.hip k_paths' PT; SRR_TAIL_MIN, SRR_POOL_CAP): survivors
  // in the wave's pool that trigger a tail pass, and the usable survivor slots (1..64)
  int tail_min, pool_cap;
};
constexpr int kPathsTailMin = 48;  // PathWork::tail_min by default: 16 of the 64 slots stay free for arrivals

// The words of PathWork::counters (renderer.cpp FrameSlot::ctr), zeroed per frame.  k_paths
// adds to them, paths_finish reads the first group into srr_stats and prints the rest as
// the SRR_PATHS_TIMING report.  Words from kCtrTicksRefill on, the four event counts among
// them aside, are written only by the diagnostics (TIMED) variants, per wave, in ticks of
// s_memtime; "its" are wave-iterations.
enum PathsCtr : int {
  kCtrWorldRays = 0,        // world rays traced (srr_stats::world_rays)
  kCtrCursor = 1,           // PathWork::cursor: next path to start (zeroed per window)
  kCtrError = 2,            // PathWork::err: guard bits of an out-of-range index
  // per-wave ticks in the phases of the path loop
  kCtrTicksRefill = 4,
  kCtrTicksWorld,           // world hit without its mesh part
  kCtrTicksMesh,            // ... and the mesh part (TraceCtx::mesh_cycles)
  kCtrTicksShade,           // record + scatter (the report subtracts the record's)
  kCtrTicksFold,
  kCtrWaveIters = 9,        // wave-iterations (every trace pass, the pre-trace's among them)
  kCtrTicksRecord = 10,     // world_record
  kCtrStackOverflows = 11,  // traversals that overflowed into the exact re-walk (TraceCtx::ovf)
  kCtrDeepTraversals = 12,  // traversals that used the stack's global extension
  kCtrTicksMixture = 13,    // the wave-cooperative mixture loop
  kCtrMixtureRounds = 14,
  kCtrMixtureCapped = 15,   // resampling loops stopped by kMixtureGuard
  // the per-lane scatter's BECK / SPEC / DIFF-set-up branches: wave ticks in each,
  // iterations each ran in, lanes it ran for
  kCtrTicksBeck = 16, kCtrTicksSpec, kCtrTicksDiffSetup,
  kCtrItsBeck, kCtrItsSpec, kCtrItsDiff,
  kCtrLanesBeck, kCtrLanesSpec, kCtrLanesDiff,
  kCtrLanesInPath,          // lanes in a path, summed over the wave-iterations
  // mesh walks (wave time in the mesh is kCtrTicksMesh): the longest walk's node steps,
  // all lanes' steps, walking lanes; the leaf-triangle queue's ticks and passes; the
  // parts of a node step: node fetch, slab + queue set-up, order + push + pop
  kCtrMeshSteps, kCtrMeshLaneSteps, kCtrMeshWalkers,
  kCtrLeafTicks, kCtrLeafPasses,
  kCtrStepFetch, kCtrStepSlab, kCtrStepOrder,
  kCtrBeckAttempts,         // mixture attempts of the Beckmann scatters: the wave's sum
  kCtrBeckAttemptsMax,      // ... and its slowest lane's
  kCtrSuspended = 36,       // suspended mesh walks (srr_stats::walks_suspended)
  // world + mesh ticks of, and the count of, the wave-iterations whose tracing lanes all
  // hold a camera ray (depth 0); the other iterations are the rest
  kCtrTicksCamOnly = 37, kCtrItsCamOnly,
  // the pre-trace: ticks and passes of the chunk's trace, shade rounds
  // (the chunk-synchronous flow: the head pass's first trace is the pre-trace)
  kCtrTicksPretrace = 39, kCtrPretracePasses, kCtrShadeRounds,
  // the chunk-synchronous flow's two kinds of pass: ticks of the whole pass (refill or
  // adoption, trace, shade, fold, promotion), passes, lanes in a path at the trace
  kCtrTicksHead = 42, kCtrHeadPasses, kCtrHeadLanes,
  kCtrTicksTail, kCtrTailPasses, kCtrTailLanes,
  kPathsCtrCount
};
constexpr int kPathsCtrWords = 48;  // words allocated (FrameSlot::ctr)
static_assert(kPathsCtrCount == 48 && kPathsCtrCount <= kPathsCtrWords, "PathsCtr fits FrameSlot::ctr");
static_assert(kCtrTailLanes == kCtrTicksHead + 5, "head and tail words");
// the groups that code walks by offset: the phases, the three family branches in BECK, SPEC,
// DIFF order (ticks, its, lanes), the step parts (TraceCtx::step_parts), the deep word behind
// the overflow word (TraceCtx::ovf)
static_assert(kCtrTicksFold == kCtrTicksRefill + 4 && kCtrTicksFold < kCtrWaveIters, "phase ticks");
static_assert(kCtrTicksDiffSetup == kCtrTicksBeck + 2 && kCtrItsBeck == kCtrTicksBeck + 3 && kCtrItsDiff == kCtrItsBeck + 2 &&
                  kCtrLanesBeck == kCtrItsBeck + 3 && kCtrLanesDiff == kCtrLanesBeck + 2 && kCtrLanesInPath == 25,
              "family words");
static_assert(kCtrMeshSteps == 26 && kCtrStepOrder == kCtrStepFetch + 2 && kCtrBeckAttemptsMax == 35 &&
                  kCtrBeckAttemptsMax < kCtrSuspended, "mesh words");
static_assert(kCtrDeepTraversals == kCtrStackOverflows + 1, "TraceCtx::ovf counts overflows, ovf[1] deep traversals");
static_assert(kCtrItsCamOnly == 38 && kCtrShadeRounds == 41, "camera-only and pre-trace words");
#ifndef SRR_KSTACK
#define SRR_KSTACK 8
#endif
constexpr int kPathsLdsStack = SRR_KSTACK;  // LDS traversal stack entries per lane (kernels.hip kStack)
constexpr int kPathsGlobalStack = 56;  // global stack entries per lane beyond the LDS ones

constexpr int kPathsWorldLdsBytes = 8192;  // == kernels.hip kWorldLdsBytes
#ifndef SRR_LDS_NODES
#define SRR_LDS_NODES 96
#endif
constexpr int kPathsLdsNodes = SRR_LDS_NODES;  // BVH4 nodes cached in LDS by k_paths (128 B each)

// k_paths' camera-ray ring (kernels.hip ring_put / ring_get): one entry per lane, the
// path's camera ray and RNG streams.  In the chunk-synchronous variants (no media, not
// quad-cooperative, diffuse only) the same entries are the wave's survivor pool
// (kernels.hip pool_put / pool_get): ray, LCG, then path index and depth in the PCG's
// words 9 and 10; words 11..13 (once the pre-traced hit) are unused
constexpr int kRingRayWords = 11;            // o.xyz, d.xyz, time, lcg (2 words), pcg (2 words)
constexpr int kRingHitWord = kRingRayWords;  // words 11, 12, 13
constexpr int kRingWordsHit = kRingHitWord + 3;
constexpr int ring_words(bool pretrace) { return pretrace ? kRingWordsHit : kRingRayWords; }
static_assert(ring_words(false) == 11 && ring_words(true) == 14 && kRingHitWord + 2 < kRingWordsHit, "ring entry layout");

// k_paths' LDS by block shape.  1,024 lanes (one block per CU, the same 4 waves per
// SIMD as four 256-lane blocks): one allocation of the CU's 160 KB, which beside the
// 8 KB world, 8 B x kPathsLdsStack per lane of stacks and the ring (44 B per lane, 56 B
// with the hit) caches the top BVH4 nodes: at kPathsLdsStack 8, 344 beside an 11-word
// ring and 248 beside a 14-word one.  256 lanes: four blocks share the CU, 40 KB each.
constexpr int kLdsPerCu = 160 * 1024;
constexpr int paths_lds_fixed(int bs, bool wl) {  // world tables, both stack arrays, alignment slack
  return (wl ? kPathsWorldLdsBytes : 16) + 8 * kPathsLdsStack * bs + bs;
}
constexpr int paths_lds_nodes_big(bool pretrace) {
  return (kLdsPerCu - paths_lds_fixed(1024, true) - 4 * ring_words(pretrace) * 1024) / 128;
}
// 256-lane blocks with the world tables in global memory keep kPathsLdsNodes nodes
// beside the 11-word ring; the 14-word ring leaves room for fewer
constexpr int paths_lds_nodes_global(bool pretrace) {
  const int room = (kLdsPerCu / 4 - paths_lds_fixed(256, false) - 4 * ring_words(pretrace) * 256) / 128;
  return room < kPathsLdsNodes ? room : kPathsLdsNodes;
}
constexpr int kPathsLdsNodesSmall = 8;  // 256-lane blocks, world in LDS, with a ring
// nodes cached by the variant: bs lanes per block, wl world tables in LDS, ring (not the
// quad-cooperative flow), pretrace (ring entries carry the hit)
constexpr int paths_lds_nodes(int bs, bool wl, bool ring, bool pretrace) {
  return bs == 1024 ? paths_lds_nodes_big(pretrace)
                    : (wl && ring) ? kPathsLdsNodesSmall : ring ? paths_lds_nodes_global(pretrace) : kPathsLdsNodes;
}
constexpr int paths_lds_bytes(int bs, bool wl, bool ring, bool pretrace) {
  return (wl ? kPathsWorldLdsBytes : 16) + 8 * kPathsLdsStack * bs + 128 * paths_lds_nodes(bs, wl, ring, pretrace) +
         (ring ? 4 * ring_words(pretrace) * bs : 4);
}
constexpr bool paths_lds_fits(int bs, bool wl, bool ring, bool pretrace) {
  return paths_lds_nodes(bs, wl, ring, pretrace) >= 1 && paths_lds_bytes(bs, wl, ring, pretrace) <= (bs == 1024 ? kLdsPerCu : kLdsPerCu / 4);
}
#if SRR_KSTACK == 8 && SRR_LDS_NODES == 96
static_assert(paths_lds_nodes_big(false) == 344 && paths_lds_nodes_big(true) == 248, "1,024-lane node sets");
#endif
// every dispatched shape: 1,024 lanes (world in LDS, ring) with and without the hit; 256 lanes with
// the world in LDS or global memory, ring (with and without the hit) or quad-cooperative
static_assert(paths_lds_fits(1024, true, true, false) && paths_lds_fits(1024, true, true, true), "1,024-lane blocks: 160 KB");
static_assert(paths_lds_fits(256, true, true, false) && paths_lds_fits(256, true, true, true) &&
              paths_lds_fits(256, true, false, false), "256-lane blocks, world in LDS: 40 KB");
static_assert(paths_lds_fits(256, false, true, false) && paths_lds_fits(256, false, true, true) &&
              paths_lds_fits(256, false, false, false), "256-lane blocks, world in global memory: 40 KB");
void dump_trace_timing();
int paths_lanes_per_device(const SceneView& S, int device);  // persistent grid capacity
int paths_block_lanes(const SceneView& S);  // k_paths lanes per block for this scene (256 or 1,024)
// 0, or -1 (nothing launched) when W.stack_cap exceeds the kernels' LDS stack (kStack)
int launch_paths(const SceneView& S, const PathWork& W, int all_families, hipStream_t st);
// device known-answer tests (srr_device_kat, kernels.hip k_kat).  kKats, the one table of the kinds: the name a
// test asks for and the floats per record (layouts in oracle/ref/kat.inc); row i is kind i (checked below)
enum KatKind : int { KAT_ERF, KAT_BECK11, KAT_BECK_DIST, KAT_BECK_PDF, KAT_COSINE, KAT_ORENNAYAR, KAT_DIELECTRIC,
                     KAT_METAL, KAT_TRIANGLE, KAT_AABB, KAT_SQRT, KAT_CAMERA, KAT_LIGHTS, KAT_LIGHT_LIST,
                     // scene KATs (one flattened host scene per record, kat_scene)
                     KAT_SPHERE, KAT_MSPHERE, KAT_RECT, KAT_BOX, KAT_XFORM, KAT_MEDIUM, KAT_ISOTROPIC, KAT_TEX_CHECKER,
                     KAT_TEX_NOISE, KAT_TEX_IMAGE };
struct KatDesc {
  KatKind kind;
  const char* name;
  int width;
};
constexpr KatDesc kKats[] = {
    {KAT_ERF, "erf", 3},                {KAT_BECK11, "beckmann11", 5},           {KAT_BECK_DIST, "beckmann_dist", 16},
    {KAT_BECK_PDF, "beckmann_pdf", 21}, {KAT_COSINE, "cosine_pdf", 21},          {KAT_ORENNAYAR, "orennayar_pdf", 21},
    {KAT_DIELECTRIC, "dielectric", 14}, {KAT_METAL, "metal", 14},                {KAT_TRIANGLE, "triangle", 26},
    {KAT_AABB, "aabb", 15},             {KAT_SQRT, "sqrt", 2},                   {KAT_CAMERA, "camera", 23},
    {KAT_LIGHTS, "lights", 15},         {KAT_LIGHT_LIST, "light_list", 15},      {KAT_SPHERE, "sphere", 22},
    {KAT_MSPHERE, "moving_sphere", 26}, {KAT_RECT, "rect", 25},                  {KAT_BOX, "box", 24},
    {KAT_XFORM, "xform", 35},           {KAT_MEDIUM, "medium", 22},              {KAT_ISOTROPIC, "isotropic", 13},
    {KAT_TEX_CHECKER, "texture_checker", 7}, {KAT_TEX_NOISE, "texture_noise", 7}, {KAT_TEX_IMAGE, "texture_image", 5}};
constexpr int kKatCount = (int)(sizeof(kKats) / sizeof(kKats[0]));
constexpr bool kat_table_in_kind_order() {
  for (int i = 0; i < kKatCount; ++i)
    if ((int)kKats[i].kind != i) return false;
  return true;
}
static_assert(kKatCount == KAT_TEX_IMAGE + 1 && kat_table_in_kind_order(), "kKats[i] must be KatKind i");
// device tables of the camera / light KATs (srr_device_kat builds them with the
// host scene code: one camera per record, one light list for all records), and of
// the scene KATs (sphere ... texture_image): the flattened tables of one host scene
// per record, concatenated, with each record's first rows in `base` (kernels.hip
// kat_scene; nullptr: one scene for all records)
struct KatTables {
  const DCamera* cams;
  const DRect* rects;
  const DSphere* spheres;
  const DStandaloneTri* stris;
  const DLight* lights;
  int n_lights;
  const DObj* objs;
  const DXform* xforms;
  const DMedium* media;
  const DMat* mats;
  const DTex* texs;
  const uint8_t* images;
  const float* perlin_ranvec;
  const int32_t* perlin_perm;
  const int32_t* base;  // [n][8]: objs, world count, xforms, spheres, rects, media, mats, texs
};
int launch_kat(int kind, int n, int w, float* d_rec, const float* d_aux, const DStandaloneTri* d_tris,
               const KatTables& kt);
// the mesh-walk KAT (srr_device_mesh_kat, kernels.hip k_mesh_kat): every walker the release
// build's basic_hit / list_hit reach -- mesh_hit<false> (SRR_TRAVERSAL=bvh2, and a medium's
// boundary), mesh_hit4<false> (SRR_TRAVERSAL=bvh4), mesh_hit4<true> (the default) and
// mesh_hit4_quad<true> (SRR_QUAD=1; the path kernel always prunes) -- with the
// kTraceBlock stack stride (the 1,024-lane stride would need a second block shape)
enum MeshKatVariant : int { kMeshKatBvh2 = 0, kMeshKatBvh4 = 1, kMeshKatBvh4Prune = 2, kMeshKatQuad = 3 };
constexpr int kMeshKatWidth = 21;  // mesh o(3) d(3) tmin tmax is_medium | hit t tri p(3) n(3) u v
struct MeshKatArgs {
  int n, width;             // records (a multiple of 64 for the quad variant)
  float* rec;               // device records, outputs written in place
  int stack_cap;            // TraceCtx::st_cap, 1 .. kStack
  int2* gst;                // TraceCtx::gst: [gst_cap][lanes], or nullptr with gst_cap 0
  int gst_cap;
  int lanes;                // TraceCtx::gst_stride: at least the launched lanes
  const int32_t* mesh_obj;  // [mesh of the record] -> its object row (an OBJ_MESH)
  const int32_t* tri_file;  // [DFS triangle index, over all meshes] -> index in its bvh command
};
// 0, -1 (bad arguments, nothing launched) or -5 (launch failed); SceneView::quad_max decides the quad variant's route
int launch_mesh_kat(const SceneView& S, int variant, const MeshKatArgs& A);
// the world-walk KAT (srr_device_world_kat, kernels.hip k_world_kat): world_hit<false, TR> and
// world_record<TR> (is_medium records: list_hit<TR> over the world's objects) on the records of
// one uploaded world, with TR = TR_BVH4_PRUNE, and | TR_WL with the tables staged in LDS
constexpr int kWorldKatWidth = 24;  // world o(3) d(3) time tmin tmax is_medium | hit t obj p(3) n(3) u v, 2 spare
struct WorldKatArgs {
  int n, width;            // records, all of the uploaded world
  float* rec;              // device records, outputs written in place
  const int32_t* leaf_of;  // [DObj row] -> the primitive's position in the world's depth-first leaf listing
};
// 0, -1 (bad arguments, nothing launched) or -5 (launch failed); tables: 0 global, 1 staged in LDS
// (S.world_words * 16 <= kPathsWorldLdsBytes)
int launch_world_kat(const SceneView& S, int tables, const WorldKatArgs& A);
// the bounce KAT (srr_device_bounce_kat, kernels.hip k_bounce_kat): one shading bounce per record over
// the one uploaded light list; variant 0 the wavefront engine's family_of / hit_emitted / scatter<family>,
// variant 1 k_paths' split diffuse bounce (skip_mixture, then coop_mixture with deep_tries) for diffuse
// records with lights
// l m p(3) n(3) u v o(3) d(3) time depth maxDepth lcg(2) pcg(4) | scattered origin(3) dir(3) time colour(3)
// attempts lcg(2) pcg(4)
constexpr int kBounceKatWidth = 43;
struct BounceKatArgs {
  int n, width;  // records, all of the uploaded light list; material m of a record is row m of SceneView::mats
  float* rec;    // device records, outputs written in place (the attempts column is left alone)
  int variant;
  int deep_tries;
};
// 0, -1 (bad arguments, nothing launched) or -5 (launch failed)
int launch_bounce_kat(const SceneView& S, const BounceKatArgs& A);
// device libm sweeps (srr_device_libm): routine kLibmFns[fn] over n elements, one per
// thread; device pointers (d_y / d_out1 unused unless n_in / n_out is 2).  The switches
// of kernels.hip k_libm_f32 / k_libm_f64 go by LibmId, and row i of the table is id i
// (checked below); an id without a case writes NaN.
enum LibmId : int {
  kLibmRsin, kLibmRcos, kLibmRexp, kLibmRlog, kLibmRpow, kLibmRacos, kLibmRasin, kLibmRatan2, kLibmRdiv,
  kLibmSincosf, kLibmAtanf, kLibmSin64, kLibmCos64, kLibmSincos64, kLibmAcos64, kLibmAtan2_64, kLibmLog64,
  kLibmOcmlLog, kLibmOcmlSin, kLibmOcmlCos, kLibmOcmlPow5
};
struct LibmFn {
  LibmId id;
  const char* name;
  int f64, n_in, n_out;
};
constexpr LibmFn kLibmFns[] = {
    {kLibmRsin, "rsin", 0, 1, 1},          {kLibmRcos, "rcos", 0, 1, 1},         {kLibmRexp, "rexp", 0, 1, 1},
    {kLibmRlog, "rlog", 0, 1, 1},          {kLibmRpow, "rpow", 0, 2, 1},         {kLibmRacos, "racos", 0, 1, 1},
    {kLibmRasin, "rasin", 0, 1, 1},        {kLibmRatan2, "ratan2", 0, 2, 1},     {kLibmRdiv, "rdiv", 0, 2, 1},
    {kLibmSincosf, "sincosf", 0, 1, 2},    {kLibmAtanf, "atanf", 0, 1, 1},       {kLibmSin64, "sin64", 1, 1, 1},
    {kLibmCos64, "cos64", 1, 1, 1},        {kLibmSincos64, "sincos64", 1, 1, 2}, {kLibmAcos64, "acos64", 1, 1, 1},
    {kLibmAtan2_64, "atan2_64", 1, 2, 1},  {kLibmLog64, "log64", 1, 1, 1},       {kLibmOcmlLog, "ocml_log", 1, 1, 1},
    {kLibmOcmlSin, "ocml_sin", 1, 1, 1},   {kLibmOcmlCos, "ocml_cos", 1, 1, 1},  {kLibmOcmlPow5, "ocml_pow5", 1, 1, 1}};
constexpr int kLibmFnCount = (int)(sizeof(kLibmFns) / sizeof(kLibmFns[0]));
constexpr bool libm_table_in_id_order() {
  for (int i = 0; i < kLibmFnCount; ++i)
    if ((int)kLibmFns[i].id != i) return false;
  return true;
}
static_assert(kLibmFnCount == kLibmOcmlPow5 + 1 && libm_table_in_id_order(), "kLibmFns[i] must be LibmId i");
int launch_libm(int fn, int64_t n, const void* d_x, const void* d_y, void* d_out0, void* d_out1);
// the fold and compaction KAT (srr_device_fold_kat): no kernel of its own -- each kind runs the
// launch wrapper below that a frame runs, on the caller's buffers.  Row i is kind i; words: the
// floats per sample of the kind's sample array (0: the kind has none)
enum FoldKatKind : int { kFoldWindow, kFoldAdaptive, kFoldSpec, kFoldLevelFinish, kFoldCompact, kFoldAov,
                         kFoldAovEmission, kFoldFinish, kFoldScatter };
struct FoldKatDesc {
  FoldKatKind kind;
  const char* name;
  int words;
};
constexpr FoldKatDesc kFoldKats[] = {
    {kFoldWindow, "window", 3},    {kFoldAdaptive, "adaptive_fold", 3},        {kFoldSpec, "adaptive_fold_spec", 3},
    {kFoldLevelFinish, "level_finish", 0}, {kFoldCompact, "compact", 0},       {kFoldAov, "aov_fold", 8},
    {kFoldAovEmission, "aov_fold_emission", 4}, {kFoldFinish, "finish", 0},    {kFoldScatter, "scatter", 3}};
constexpr int kFoldKatCount = (int)(sizeof(kFoldKats) / sizeof(kFoldKats[0]));
constexpr bool fold_table_in_kind_order() {
  for (int i = 0; i < kFoldKatCount; ++i)
    if ((int)kFoldKats[i].kind != i) return false;
  return true;
}
static_assert(kFoldKatCount == kFoldScatter + 1 && fold_table_in_kind_order(), "kFoldKats[i] must be FoldKatKind i");
// MERL table lookup (merl.h) for n queries; device pointers
int launch_merl_lookup(const double* table, int64_t n, const double* angles, double* rgb, int32_t* cell);
// acc[pixel] (+)= the window's samples in order; init: acc starts at 0 (no
// memset); out != nullptr (the last window): also out = acc * (float)(1.0 / scale_ns)
// (k_finish), or the raw sums when scale_ns == 0
void launch_accumulate_window(const float* sample, int npix, int spp_w, float* acc, hipStream_t st, bool init = false,
                              float* out = nullptr, int scale_ns = 0);
// ---- adaptive sampling (srr_render_adaptive, renderer.cpp render_adaptive)
int paths_kernel_stack();  // the kernels' LDS traversal stack entries (kStack): launch_paths refuses a larger stack_cap
// the convergence rule of include/srr_capi.h, evaluated by the code the kernel runs
int adaptive_converged_host(int32_t n, float s1, float s2, float rel_tol, float abs_eps);
// the variance of the mean luminance of include/srr_capi.h, by the code the kernel runs
float variance_of_mean_host(int32_t n, float s1, float s2);
// var[slot] = that of (count[slot], mom[slot]) for the n slots of an adaptive frame
void launch_adaptive_variance(int n, const float2* mom, const int32_t* count, float* var, hipStream_t st);
// One sample window of a pass: row j of `sample` ([n_active][spp_w][3]) holds the
// window's samples of slot active_slot[j] (nullptr: slot j), a slot being a position
// in the shard's pixel list.  The fold adds them, in sample order, to the slot's rgb
// sums and luminance moments (init: the state starts from 0).  decide (the pass's
// last window, when a pixel may retire): the slot, now holding n_new samples,
// retires if n_new >= budget or (rel_tol > 0 and the rule holds): keep[j] = 0 and
// mean / count (may be nullptr) of the slot are written; else keep[j] = 1.
struct AdaptiveFold {
  const float* sample;
  const int32_t* active_slot;
  int n_active, spp_w;
  float* sums;   // [slot][3]
  float2* mom;   // [slot] (s1, s2)
  int init, decide;
  int n_new, budget;
  float rel_tol, abs_eps;
  uint8_t* keep;   // [n_active]
  float* mean;     // [slot][3]
  int32_t* count;  // [slot]
};
void launch_adaptive_fold(const AdaptiveFold& A, hipStream_t st);
// One sample window of a SPECULATIVE pass (include/srr_capi.h srr_adaptive_speculate): the
// pass gives every active slot, which holds n samples, the w samples [n, n + w); this
// window holds the spp_w of them from n + s0 on, rows as in AdaptiveFold.  The fold adds a
// row's samples in order and asks the rule at every boundary c of the pass ((c - n) %
// batch_spp == 0, or c == n + w): the slot stops at the first c with c >= budget, or
// c >= min_spp, rel_tol > 0 and the rule holding -- nothing past c is folded, count[slot]
// = c, mean[slot] = sums * (float)(1.0 / (float)c) and keep[j] = 0.  A slot that does not
// stop leaves count[slot] = n + s0 + spp_w and keep[j] = 1.  In a window with s0 > 0 a
// slot whose count is not n + s0, or that is retired at n + s0 when that is a boundary,
// stopped in an earlier window of the pass: it is left as it is.  ctr[0] += the samples
// of the window that lie past their slot's stop, ctr[1] += the slots that stopped in it
// below the budget.
struct AdaptiveSpecFold {
  const float* sample;
  const int32_t* active_slot;
  int n_active, spp_w;
  float* sums;   // [slot][3]
  float2* mom;   // [slot] (s1, s2)
  int n, w, s0;
  int batch_spp, min_spp, budget;
  float rel_tol, abs_eps;
  uint8_t* keep;   // [n_active]
  float* mean;     // [slot][3]
  int32_t* count;  // [slot]
  unsigned long long* ctr;  // [kSpecDiscarded], [kSpecStopped]
};
enum { kSpecDiscarded = 0, kSpecStopped = 1, kSpecWords = 2 };
void launch_adaptive_fold_spec(const AdaptiveSpecFold& A, hipStream_t st);
// Stable compaction of the rows with keep[j] != 0, in ascending j: slot_out[k] =
// their slots, pixel_out[k] = pixels[slot] (nullptr: the slot itself), *n_out = how
// many.  blk: scratch of (n_active + 255) / 256 ints.  The lists must not alias.
void launch_adaptive_compact(const uint8_t* keep, const int32_t* active_slot, int n_active, const int32_t* pixels,
                             int32_t* blk, int32_t* slot_out, int32_t* pixel_out, int32_t* n_out, hipStream_t st);
// ---- resuming an adaptive frame (srr_render_adaptive_resume, renderer.cpp adaptive_resume_passes)
// A slot that holds n samples is retired iff n >= budget, or n >= min_spp, rel_tol > 0
// and the convergence rule holds for its moments.
struct AdaptiveRule {
  int budget, min_spp;
  float rel_tol, abs_eps;
};
// the words of a resume's device scratch `lvl`; a pass reads the first two back in one copy
enum { kLvlActive = 0, kLvlLevel = 1, kLvlLive = 2, kLvlBelow = 3, kLvlWords = 4 };
// The next pass's active set from the state of all n_slots slots: live[i] = slot i is
// not retired, lvl[kLvlLevel] = the least count among the live slots (INT_MAX: none),
// lvl[kLvlLive] = how many are live, keep[i] = live and count[i] == that level; then
// launch_adaptive_compact over every slot leaves their lists in slot_out / pixel_out
// and their number in lvl[kLvlActive].
void launch_adaptive_level_select(int n_slots, const int32_t* count, const float2* mom, const AdaptiveRule& R,
                                  uint8_t* live, uint8_t* keep, int32_t* lvl, hipStream_t st);
// mean[slot] = sums[slot] * (float)(1.0 / (float)count[slot]) and count_out[slot] (may be
// nullptr) = count[slot] for every slot; lvl[kLvlBelow] (zeroed here) = the slots with count < budget
void launch_adaptive_finish(int n_slots, const float* sums, const int32_t* count, int budget, float* mean,
                            int32_t* count_out, int32_t* lvl, hipStream_t st);
void launch_raygen(const SceneView& S, const PathState& P, const BatchInfo& B, hipStream_t st);
void launch_trace(const SceneView& S, const PathState& P, const int* active, const int* count, int max_n,
                  int* lists, int list_cap, int* fam_count, int* fetch, int max_depth, unsigned long long* ctr,
                  hipStream_t st);
void launch_shade(const SceneView& S, const PathState& P, const int* lists, int list_cap, const int* fam_count,
                  int* next, int* next_count, int* region_alive, int region_size, int max_n, int max_depth,
                  hipStream_t st);
void launch_accumulate(const PathState& P, const BatchInfo& B, float* acc, hipStream_t st);
void launch_finish(const float* acc, float* mean, int64_t n, int ns, hipStream_t st);
// ---- first-hit AOVs (srr_render_aov, renderer.cpp render_aov)
// After launch_raygen (slot0 = act0 = 0) and launch_trace of a batch of n primary rays:
// val[2p] = (albedo.rgb, depth), val[2p + 1] = (normal.xyz, 0) of path p, de_nan'd.
// emit != nullptr (srr_render_aov_emission): also emit[p] = (emitted().rgb, 0), by the
// kernel's other instantiation; nullptr launches the kernel that does no emission work.
void launch_aov_eval(const SceneView& S, const PathState& P, int n, float4* val, float4* emit, hipStream_t st);
// acc[8 lp + c] (+)= the batch's spp_b samples of pixel lp in sample order (init: the
// sums start from 0); finish: also the means sum * (float)(1.0 / (float)ns) to the
// caller's buffers (nullptr: not asked for) at shard pixel p0 + lp.
struct AovFold {
  const float* val;  // [np][spp_b][8]
  int np, spp_b;
  float* acc;        // [np][8]
  int init, finish, ns, p0;
  float* albedo;
  float* normal;
  float* depth;
};
void launch_aov_fold(const AovFold& A, hipStream_t st);
// The emission's fold (srr_render_aov_emission): acc[4 lp + c] (+)= those of the batch's
// samples [s0, s0 + spp_b) of pixel lp that lie below the pixel's count n_i = count[p0 + lp]
// clamped into 1..ns (count == nullptr: ns), in sample order, from 0 when s0 == 0; the
// batch that holds sample n_i - 1 writes sum * (float)(1.0 / (float)n_i) to emission.
struct AovEmissionFold {
  const float* emit;  // [np][spp_b][4]
  int np, spp_b, s0;
  float* acc;         // [np][4]
  int ns, p0;
  const int32_t* count;  // [shard pixels] or nullptr
  float* emission;       // [shard pixels][3]
};
void launch_aov_fold_emission(const AovEmissionFold& A, hipStream_t st);
// ---- through-specular AOVs (srr_render_aov_through, renderer.cpp render_aov_through)
// One bounce after launch_trace over the *count paths of `active`: a path whose hit is
// metal or dielectric below max_depth takes that specular step (record, running depth,
// scatter<FAM_SPEC>, next ray, depth + 1) and is appended to next / *next_count; every
// other path ends and leaves val[2p], val[2p + 1] as launch_aov_eval does, the albedo
// folded back to front through the path's metal records.  max_n >= *count sizes the grid.
struct AovChain {
  const int32_t* active;
  const int32_t* count;
  int32_t* next;
  int32_t* next_count;  // zeroed by the caller
  int max_depth;
  int cap;              // paths of the call's batch: chain's size, rec's stride
  int2* chain;          // [cap] (running depth as float bits, metal records written)
  float* rec;           // [max_depth][cap][3] metal colours, in bounce order per path
  float4* val;          // [>= cap][2]
  float4* emit;         // [>= cap] (emission.rgb, 0), or nullptr: the instantiation without emission
};
void launch_aov_chain(const SceneView& S, const PathState& P, const AovChain& C, int max_n, hipStream_t st);
// image[index[i]] = packed[i] (float3 per pixel) for i < n: multi-device frame assembly
void launch_scatter_pixels(const float* packed, const int32_t* index, int64_t n, float* image, hipStream_t st);

}  // namespace srr
