// The device-resident renderer behind srr_renderer_* (include/srr_capi.h):
// uploaded scene tables plus the wavefront path pools.
//
// Work is organised in LANES: each lane owns a HIP stream and a pool of path
// slots split into regions; a region holds one batch (a pixel chunk x sample
// chunk).  A lane runs trace -> shade (material-sorted) bounces over all its live
// paths, refilling freed regions with new batches, so a batch's tail of long
// paths overlaps the next batches' first bounces; several lanes run
// concurrently so one lane's straggler waves overlap other lanes' kernels.
// Finished batches are accumulated on a separate stream strictly in batch order
// (per-pixel sums stay in sample order, hence bitwise reproducible).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/srr_capi.h"
#include "devmem.h"
#include "kernels.h"
#include "scene.h"

namespace srr {

constexpr int kRegionsPerLane = 3;  // <= kernels.hip kMaxRegions
constexpr int kMaxLanes = 4;

struct Lane {
  hipStream_t st = nullptr;
  hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr, ev_s1 = nullptr, ev_rb = nullptr;
  hipEvent_t done_ev[kRegionsPerLane] = {};  // batch in region finished (lane stream)
  hipEvent_t acc_ev[kRegionsPerLane] = {};   // batch in region accumulated (acc stream)
  bool acc_pending[kRegionsPerLane] = {};    // region reuse must wait for acc_ev
  // the path pool (renderer.cpp ensure_lane): P, act and lists point into `bufs`
  PathState P{};
  int32_t* act[2] = {nullptr, nullptr};
  int32_t* lists = nullptr;  // 4 material-family lists
  DeviceBag bufs;
  size_t cap = 0;            // paths the pool holds (0: none)
  int cap_depth = 0;
  bool has_raw = false;
  DeviceMem<int32_t> cnt;  // [0..1] active counts, [2..2+R) region survivors, [2+R..6+R) families
  PinnedMem<int32_t> rb;   // host mirror of region survivors + next count
  // per-frame state
  int n = 0, cur = 0;
  bool pending = false;
  int reg_batch[kRegionsPerLane];
  double trace_ms = 0, shade_ms = 0;
};

// One frame of the path engine: its stream, bounce records, traversal-stack
// extension, sample window, counters and events (renderer.cpp paths_enqueue);
// the synchronous path owns one, srr_render_device_async alternates two.
struct FrameSlot {
  hipStream_t st = nullptr;
  bool own_stream = false;
  hipEvent_t ev_beg = nullptr, ev_end = nullptr;
  std::vector<hipEvent_t> win_ev;  // per sample window: k_paths start / end
  DeviceMem<float4> rec;
  // [kPathsGlobalStack][pw_lanes] int2 (kernels.h), then [3][pw_lanes] float4 of suspended
  // mesh walks (kernels.h PathWork::walk_q)
  DeviceMem<int2> gstack;                   // allocated once and kept
  DeviceMem<float> sample;                  // the sample window: [paths][3]
  DeviceMem<unsigned long long> ctr;        // [0] world rays, [1] path cursor, ...
  PinnedMem<unsigned long long> ctr_host;   // mirror, read after the frame's stream sync
  DeviceMem<float> acc;                     // async slots: the frame's own per-pixel sums [pixels][3]
  // a frame in flight (async slots)
  bool busy = false;
  int64_t ticket = -1, npix = 0, paths = 0;
  int n_windows = 0;
  int rc = 0;
  srr_stats stats{};
  std::string err;
};

struct DoneTicket {  // an async frame finished before its srr_render_wait
  int64_t ticket;
  int rc;
  srr_stats stats;
  std::string err;
};

// Per-slot state and active lists of srr_render_adaptive (renderer.cpp render_adaptive);
// a slot is a position in the shard's pixel list.  The rgb sums are srr_renderer::acc.
struct AdaptiveState {
  size_t cap = 0;               // slots the buffers hold (0: none)
  // slots whose moments the most recent successful frame left in `mom` (0: none);
  // srr_adaptive_variance reads them
  int64_t valid_npix = 0;
  // srr_renderer::acc still holds that state's rgb sums: every other writer of acc clears
  // this (begin_accum, ensure_pixels, srr_accum_set), and srr_render_adaptive_resume needs it
  bool sums_valid = false;
  // the frame and shard the state belongs to: {nx, ny, shard_index, shard_count, tile}
  int key[5] = {-1, -1, -1, -1, -1};
  DeviceMem<float2> mom;       // [slot] luminance moments (s1, s2)
  DeviceMem<int32_t> count;    // [slot] samples held (n_i): the folds' count target
  DeviceMem<uint8_t> live;     // [slot] not retired (a resume's k_adaptive_level)
  DeviceMem<int32_t> lvl;      // a resume's words (kernels.h kLvl*)
  PinnedMem<int32_t> lvl_host; // their mirror
  DeviceMem<int32_t> slot[2];   // active slots, ping-pong over the compactions
  DeviceMem<int32_t> pixel[2];  // their image pixels (PathWork::pixels)
  DeviceMem<uint8_t> keep;      // [active row] survives the pass
  DeviceMem<int32_t> blk;       // compaction scratch: per-block counts / offsets, then [nb] the new active count
  PinnedMem<int32_t> n_host;    // mirror of the new active count
  // speculative passes (srr_adaptive_speculate): the setting, which outlives the buffers,
  // and what srr_adaptive_last_spec_stats reports of the most recent frame (windows < 0: none yet)
  int pass_spp_max = 0;
  int64_t fill_paths = 0;
  int32_t spec_windows = -1;
  int64_t spec_traced = 0, spec_discarded = 0;
  DeviceMem<unsigned long long> spec_ctr;       // kernels.h kSpec* words of the frame's speculative folds
  PinnedMem<unsigned long long> spec_ctr_host;  // their mirror
};

// Buffers of srr_render_aov (renderer.cpp render_aov): a stream, a pixel list, Sobol
// points and depth-0 path state of its own, so the call leaves the frame state alone.
struct AovState {
  hipStream_t st = nullptr;
  size_t cap = 0;       // paths the batch buffers hold (0: none)
  PathState P{};        // depth-0 state only: rays, RNG, depth, spec, hit record
  int32_t* active = nullptr;
  int32_t* lists = nullptr;  // launch_trace's 4 material-family lists [4][cap]
  int32_t* cnt = nullptr;    // [0] active count, [1..4] family counts, [5] fetch
  float4* val = nullptr;     // [cap][2] per-path values
  DeviceBag bufs;            // the batch buffers: what P, active, lists, cnt and val point to
  DeviceMem<int32_t> pixels;
  DeviceMem<float> acc;      // [pixels][8], sized with the list
  DeviceMem<double> sobol;
  int sobol_n = 0;
  // srr_render_aov_through only (renderer.cpp ensure_aov_through), sized by that call's own
  // batch: t_cap paths, t_rec floats of metal records
  size_t t_cap = 0, t_rec = 0;
  int32_t* next = nullptr;   // the other active list of the bounce loop
  int2* chain = nullptr;     // kernels.h AovChain::chain
  float* rec = nullptr;      // kernels.h AovChain::rec
  DeviceBag t_bufs;          // what next, chain and rec point to
  PinnedMem<int32_t> n_host;  // mirror of the next bounce's active count
  // srr_render_aov_emission only (renderer.cpp ensure_aov_emission), allocated the first time
  // SRR_AOV_EMISSION is asked for
  DeviceMem<float4> emit;    // [>= the call's batch] per-path (emission.rgb, 0)
  DeviceMem<float> acc_e;    // [pixels][4] the emission's sums
};

struct Multi;  // multi.h
}  // namespace srr

struct srr_renderer {
  int device = 0;
  // srr_renderer_create_multi: this handle renders over several devices through
  // their own renderers (multi.cpp); its single-device state below stays unused
  srr::Multi* multi = nullptr;
  srr::SceneView view{};
  srr::DeviceBag scene_bufs;  // what `view` points to
  int n_lanes = 2;
  srr::Lane lanes[srr::kMaxLanes];
  hipStream_t acc_st = nullptr;
  hipEvent_t ev_beg = nullptr, ev_end = nullptr;
  // frame buffers
  srr::DeviceMem<float> acc;  // [pixels][3], sized with the pixel list
  int64_t acc_npix = 0;     // pixels the running sums cover (SRR_FLAG_CONTINUE)
  int64_t acc_samples = 0;  // samples per pixel accumulated in them
  // the frame and shard the running sums belong to: {nx, ny, shard_index,
  // shard_count, tile}; all -1 after srr_accum_set (only npix is known then)
  int acc_key[5] = {-1, -1, -1, -1, -1};
  srr::DeviceMem<unsigned long long> visits;  // SRR_FLAG_COUNT_VISITS counters
  // path-resident engine (render_paths)
  int pw_lanes = 0;
  bool diffuse_only = false;  // no beckmann / specular materials: lean kernel variant
  int walk_q_default = 0;     // suspendable mesh walks unless SRR_WALK_Q says otherwise (renderer.cpp)
  bool has_meshes = false;
  srr::FrameSlot sync_slot;         // srr_render_device (stream acc_st, sums in acc)
  srr::FrameSlot async_slots[2];    // srr_render_device_async, alternating
  int64_t next_ticket = 0;
  std::vector<srr::DoneTicket> done_tickets;
  hipEvent_t ev_async_in = nullptr;  // orders an async frame after the caller's legacy-stream work
  // renderers sharing this device under one multi-device handle (multi.cpp): each takes
  // 1/window_share of the sample-window budget (SRR_WINDOW_MB)
  int window_share = 1;
  srr::DeviceMem<unsigned long long> pw_wave_times;  // SRR_WAVE_TIMES diagnostics, 4 words per wave
  srr::DeviceMem<float> pw_slow;  // diagnostics build (-DSRR_SLOW_RAYS): slow world-hit records + count
  srr::DeviceMem<int32_t> pixels;
  // the shard whose pixel list (srr_shard_pixels) the renderer holds: {nx, ny,
  // shard_index, shard_count, tile}, its pixel count, and whether it is the
  // identity (then `pixels` is not read); key[0] = -1: none.  srr_render_device
  // passes pix = nullptr to render_device when the shard is this one.
  int pix_key[5] = {-1, -1, -1, -1, -1};
  int64_t pix_n = 0;
  bool pix_identity = false;
  srr::DeviceMem<double> sobol;
  int sobol_n = 0;
  // SRR_FLAG_KEEP_PATHS: [path][3] radiance and [path] ray counts, both or neither (renderer.cpp ensure_kept)
  srr::DeviceMem<float> raw_all;
  srr::DeviceMem<uint8_t> rays_all;
  int64_t kept_paths = 0;
  srr::AdaptiveState adaptive;
  srr::AovState aov;
  ~srr_renderer();
};

namespace srr {
int renderer_create(const Scene& s, int device, srr_renderer** out, std::string& err);
// the same from an already flattened scene (a multi-device renderer flattens once)
int renderer_create_flat(const Flat& F, int device, srr_renderer** out, std::string& err);
// pix: the shard's npix pixel indices, or nullptr when the renderer already holds
// them (srr_renderer::pix_key)
int render_device(srr_renderer* r, const srr_params* p, const int32_t* pix, int64_t npix, float* d_mean,
                  srr_stats* stats, std::string& err);
int render_device_async(srr_renderer* r, const srr_params* p, const int32_t* pix, int64_t npix, float* d_mean,
                        int64_t* ticket, std::string& err);
// srr_render_adaptive on a one-device renderer, its arguments already validated (capi.cpp)
// resume: srr_render_adaptive_resume, the renderer's adaptive state being valid and this frame's
int render_adaptive(srr_renderer* r, const srr_params* p, const srr_adaptive_params* a, const int32_t* pix,
                    int64_t npix, float* d_mean, int32_t* d_count, srr_adaptive_stats* stats, bool resume,
                    std::string& err);
// srr_adaptive_state_get / _set on a one-device renderer, arguments validated (capi.cpp);
// get copies the valid_npix slots of the buffers asked for (nullptr: not asked for)
int adaptive_state_get(srr_renderer* r, float* sums, float* mom, int32_t* count, std::string& err);
int adaptive_state_set(srr_renderer* r, const srr_params* p, const float* sums, const float* mom,
                       const int32_t* count, int64_t npix, std::string& err);
// srr_adaptive_variance on a one-device renderer that holds a valid adaptive frame (capi.cpp)
int adaptive_variance(srr_renderer* r, const int32_t* d_count, float* d_var, std::string& err);
// srr_render_aov on a one-device renderer, its arguments already validated (capi.cpp);
// a nullptr buffer is not asked for
int render_aov(srr_renderer* r, const srr_params* p, const int32_t* pix, int64_t npix, float* d_albedo,
               float* d_normal, float* d_depth, std::string& err);
// srr_render_aov_through likewise; stats may be nullptr
int render_aov_through(srr_renderer* r, const srr_params* p, const int32_t* pix, int64_t npix, float* d_albedo,
                       float* d_normal, float* d_depth, srr_aov_stats* stats, std::string& err);
// srr_render_aov_emission likewise: d_emission != nullptr adds the emission buffer (folded over
// the first d_count[i] samples of the range per pixel when d_count != nullptr), through != 0
// takes render_aov_through's chain; stats may be nullptr (first hit: paths and world_rays)
int render_aov_emission(srr_renderer* r, const srr_params* p, const int32_t* pix, int64_t npix, int through,
                        float* d_albedo, float* d_normal, float* d_depth, float* d_emission, const int32_t* d_count,
                        srr_aov_stats* stats, std::string& err);
// The pixel list and the running sums hold npix pixels (contents not preserved).  Growing
// replaces both buffers, and the held list (pix_key) and the running sums' bookkeeping
// (acc_npix, acc_samples, acc_key) are forgotten with them; on failure both are empty.
hipError_t ensure_pixels(srr_renderer* r, int64_t npix);
int render_wait(srr_renderer* r, int64_t ticket, srr_stats* stats, std::string& err);
void drain_async(srr_renderer* r);  // finish every async frame in flight (results kept for render_wait)
// the event recorded after async frame `ticket`'s last operation (its slot's frame end),
// or nullptr when that frame is no longer in flight (multi.cpp orders its exchange by it)
hipEvent_t render_ticket_event(srr_renderer* r, int64_t ticket);
}  // namespace srr
