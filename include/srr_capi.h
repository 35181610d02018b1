/* srr -- MI355X-native path tracer: C-ABI drop-in boundary.
 *
 * The reference (truemeat001/Simple-Raytracing-Render) has no FFI: its
 * "operator API" is a C++ class hierarchy that scene builders instantiate with
 * `new` (Raytracing_n.cpp:108-711) and a render driver walks on 8 CPU threads
 * (renderthread, Raytracing_n.cpp:815-879).  This header is that boundary as a
 * flat C ABI: one constructor per reference class (same argument order and
 * meaning), returning integer handles, plus the render entry points that
 * replace renderthread/main.  Plain pointers and sizes only; no C++ or torch
 * types.  Every function returns >= 0 on success and a negative errno-style code
 * on failure (srr_last_error() has the message); nothing calls exit()
 * (the reference's sobol_points does, Raytracing_n.cpp:724-727).
 *
 * Threading: a scene / renderer handle is used by one host thread at a time.
 * The C++ source-compatible headers in include/srr/ are a thin layer over this
 * ABI (see INTEGRATION.md for the ctypes / C++ bindings).
 */
#ifndef SRR_CAPI_H
#define SRR_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRR_OK 0
#define SRR_EINVAL (-22)
#define SRR_ENOMEM (-12)
#define SRR_ENODEV (-19)
#define SRR_ENOTSUP (-95)
#define SRR_EIO (-5)

typedef struct srr_scene srr_scene;
typedef struct srr_renderer srr_renderer;

/* Thread-local message for the last failing call on this thread. */
const char* srr_last_error(void);
/* Library version / build string ("srr 0.1 gfx950 ..."). */
const char* srr_version(void);

/* ------------------------------------------------------------ scene lifetime */
srr_scene* srr_scene_create(void);
void srr_scene_destroy(srr_scene* s);
/* Parse an srr scene description v1 into a new scene. */
int srr_scene_from_text(const char* text, srr_scene** out);
/* Handle of the hitable a parsed description named `obj <text_id>`. */
int srr_scene_text_handle(const srr_scene* s, int text_id);
/* State of the scene-build LCG (the reference's global drand48 seed,
 * mathf.h:12) that the next srr_bvh_node() consumes; default is the
 * post-Perlin state 24561125610955 (perlin.h:94-97). */
int srr_scene_set_lcg(srr_scene* s, uint64_t state);
/* FNV-1a-64 digest of the scene's flattened device tables (no GPU needed): two
 * scenes with equal digests render identically (used to pin scene builders).
 * parts: NULL or SRR_DIGEST_PARTS per-table digests (objects, n_world,
 * transforms, spheres, rects, triangles, meshes, BVH2, BVH4, triangle
 * positions, triangle shading, media, object BVHs, their children, materials,
 * textures, image bytes, Perlin vectors, Perlin permutations, lights, camera). */
#define SRR_DIGEST_PARTS 21
int srr_scene_digest(const srr_scene* s, uint64_t* out, uint64_t* parts);
uint64_t srr_scene_get_lcg(const srr_scene* s);
/* drand48() on the scene LCG (mathf.h:14-19), for builders that draw. */
double srr_scene_drand48(srr_scene* s);

/* ------------------------------------------------------------------ textures
 * texture.h:25-33 constant_texture(vec3) */
int srr_constant_texture(srr_scene* s, float r, float g, float b);
/* texture.h:48-70 image_texture(unsigned char* pixels, int nx, int ny): RGB8,
 * row 0 = top; the bytes are copied (the reference borrows them). */
int srr_image_texture(srr_scene* s, const unsigned char* rgb, int nx, int ny);
/* image_texture(stbi_load(path, &tx, &ty, &tn, 0), tx, ty), the builders' idiom
 * (Raytracing_n.cpp:269-270, :614-616, :631-632): decodes PNG / baseline JPEG /
 * TGA as stb_image v2.19 does (byte-identical, tests/test_imageio.py) and keeps
 * the 3 bytes per texel image_texture addresses. */
int srr_image_texture_file(srr_scene* s, const char* path);
/* Synthetic RGB8 image (stand-in for stbi_load'ed assets; kind 0 sky, 1 wood,
 * 2 checker), identical bytes on every consumer. */
int srr_image_texture_gen(srr_scene* s, int nx, int ny, uint32_t seed, int kind);
/* texture.h:9-23 checker_texture(texture* t0 (even), texture* t1 (odd)) */
int srr_checker_texture(srr_scene* s, int even_tex, int odd_tex);
/* texture.h:35-46 noise_texture(float scale) (Perlin tables of perlin.h:67-97) */
int srr_noise_texture(srr_scene* s, float scale);

/* ----------------------------------------------------------------- materials
 * (material.h); a material handle of -1 is the reference's null material* */
int srr_lambertian(srr_scene* s, int albedo_tex);                       /* :95-114  */
int srr_orennayar(srr_scene* s, int albedo_tex, float sigma_deg);       /* :127-149 */
int srr_beckmann(srr_scene* s, int albedo_tex, float roughx, float roughy); /* :151-199 */
int srr_metal(srr_scene* s, float r, float g, float b, float fuzz);     /* :243-261 */
int srr_dielectric(srr_scene* s, float ref_idx);                        /* :282-339 */
int srr_diffuse_light(srr_scene* s, int emit_tex);                      /* :341-356 */
int srr_isotropic(srr_scene* s, int albedo_tex);                        /* :359-369 */

/* ------------------------------------------------------------------ hitables */
int srr_sphere(srr_scene* s, const float center[3], float radius, int mat);        /* sphere.h:21 */
int srr_moving_sphere(srr_scene* s, const float c0[3], const float c1[3], float t0, float t1, float radius,
                      int mat);                                                     /* moving_sphere.h:8 */
int srr_xy_rect(srr_scene* s, float x0, float x1, float y0, float y1, float k, int mat); /* aarect.h:8 */
int srr_xz_rect(srr_scene* s, float x0, float x1, float z0, float z1, float k, int mat); /* aarect.h:38 */
int srr_yz_rect(srr_scene* s, float y0, float y1, float z0, float z1, float k, int mat); /* aarect.h:69 */
int srr_box(srr_scene* s, const float p0[3], const float p1[3], int mat);          /* box.h:18-29 */
/* triangle.h:13-50: uv (3 x vec3) and normals (3 x vec3) may be NULL; without
 * normals the face normal is used (SURVEY Q5 build definition). */
int srr_triangle(srr_scene* s, const float p[9], int mat, const float* uv9, const float* n9);
int srr_flip_normals(srr_scene* s, int child);                                     /* aarect.h:149-171 */
int srr_translate(srr_scene* s, int child, const float offset[3]);                 /* hitable.h:35-61 */
int srr_rotate_y(srr_scene* s, int child, float angle_deg);                        /* hitable.h:65-132 */
int srr_rotate_x(srr_scene* s, int child, float angle_deg);                        /* hitable.h:135-203 */
int srr_constant_medium(srr_scene* s, int boundary, float density, int tex);       /* constant_medium.h:6 */
int srr_hitable_list(srr_scene* s, const int* children, int n);                    /* hitable_list.h:11 */
/* bvh.h:96-119 bvh_node(hitable** l, int n, float time0, float time1): built
 * eagerly with the reference's random-axis median split, consuming the scene
 * LCG exactly like the reference (one draw per node). */
int srr_bvh_node(srr_scene* s, const int* children, int n, float time0, float time1);
/* Utah teapot (teapot.h:76-166) with `divs` subdivisions: creates 2*32*divs^2
 * triangle handles, first_handle .. first_handle+count-1, returns count. */
int srr_teapot(srr_scene* s, float scale, int divs, int mat, int* first_handle);

/* model.h:27-102 (assimp replaced by srr's PLY / binary-FBX readers): the file's
 * first mesh (model::genhitablemodel returns mesh 0 only) as triangles built like
 * geometry.h:55-77: positions scaled per component, UV channel 0 (v -> 1 - v with
 * flip_uvs), index order reversed with flip_winding, polygons fanned.  Creates
 * count triangle handles first_handle .. first_handle+count-1 and returns count.
 * Files without normals get face normals (SURVEY Q19 build definition). */
int srr_model(srr_scene* s, const char* path, int flip_uvs, int flip_winding, int mat, const float scale[3],
              int* first_handle);
/* The same triangles without a scene: per triangle 9 floats each of positions,
 * uvs (u, v, 0 per corner) and normals (zeros when the file has none; the scene
 * then uses face normals).  Buffers may be NULL to ask for the count.
 * flags_out (may be NULL): bit 0 file has normals, bit 1 file has UVs. */
int srr_mesh_file_triangles(const char* path, int flip_uvs, int flip_winding, const float scale[3], float* pos9,
                            float* uv9, float* nrm9, int* flags_out);

/* camera.h:33-48, 9-argument constructor */
int srr_camera(srr_scene* s, const float lookfrom[3], const float lookat[3], const float vup[3], float vfov,
               float aspect, float aperture, float focus_dist, float t0, float t1);
/* world: the hitable passed as `world` to renderthread (Raytracing_n.cpp:815);
 * lights: `hlist`, must be a hitable_list (cast at Raytracing_n.cpp:75). */
int srr_scene_set_world(srr_scene* s, int obj);
int srr_scene_set_lights(srr_scene* s, int list_obj);

/* ----------------------------------------------------------------- rendering */
typedef struct srr_params {
  int nx, ny;          /* image size (Raytracing_n.cpp:39-40)                  */
  int spp;             /* samples per pixel, ns (:41)                          */
  int max_depth;       /* maxDepth (:42)                                       */
  int tile;            /* tile edge for sharding, e.g. 32                      */
  int shard_index;     /* this renderer renders tiles t (in tile row tr) with  */
  int shard_count;     /*   (t + tr) % shard_count == shard_index */
  int batch_paths;     /* paths in flight per wavefront batch (0 = auto)       */
  uint64_t base_seed;  /* per-path seed salt; 0 = SURVEY §8(d) definition      */
  int flags;           /* SRR_FLAG_*                                           */
  int sample_begin;    /* global index of sample 0: a sample shard renders     */
                       /*   samples [sample_begin, sample_begin + spp)         */
} srr_params;

#define SRR_FLAG_SORT_MATERIALS 1 /* material-sorted shading (perf only)      */
#define SRR_FLAG_KEEP_PATHS 2     /* keep per-path radiance for parity tests   */
#define SRR_FLAG_COUNT_VISITS 4   /* count mesh box / triangle tests (slower)    */
#define SRR_FLAG_WAVEFRONT 8      /* use the wavefront engine (per-bounce kernels) */
                                  /* instead of the path-resident persistent one  */
#define SRR_FLAG_CONTINUE 16      /* progressive rendering: add this render's      */
                                  /* samples to the renderer's per-pixel running   */
                                  /* sums (set sample_begin to the samples already */
                                  /* in them); the mean covers all of them         */
#define SRR_FLAG_SUMS 32          /* srr_render_device writes the per-pixel sample */
                                  /* SUMS (the running sums) instead of the means: */
                                  /* sample-sharded frames reduce these over ranks */

typedef struct srr_stats {
  int64_t world_rays;   /* world->hit calls (the metric's samples)             */
  int64_t paths;        /* camera paths                                        */
  int64_t trace_launches;
  double trace_ms;      /* summed HIP-event time of the trace kernel launches  */
  double shade_ms;
  double total_ms;      /* render wall time on the device stream               */
  int64_t bounces;      /* bounce iterations launched                          */
  int64_t box_tests;    /* SRR_FLAG_COUNT_VISITS: mesh BVH boxes tested        */
  int64_t tri_tests;    /*   triangle tests (a 1-triangle leaf counts 2, as    */
                        /*   the reference tests it twice, bvh.h:104-105)      */
  int64_t stack_overflows; /* rays re-walked on the stackless BVH2             */
  int64_t deep_traversals; /* path engine: mesh traversals whose stack went past */
                           /* its LDS part into the global extension           */
  int64_t mixture_capped;  /* path engine: resampling loops (Raytracing_n.cpp:79-83) */
                           /* stopped by the 100,000-attempt cap   */
  int64_t walks_suspended; /* path engine: mesh walks continued in a later wave-  */
                           /* iteration (SRR_WALK_Q)              */
} srr_stats;

/* Flatten the scene and upload it to HIP device `device`. */
int srr_renderer_create(const srr_scene* s, int device, srr_renderer** out);
void srr_renderer_destroy(srr_renderer* r);
/* One renderer over n_devices GPUs: the replacement for the
 * reference's 8 renderthreads in one process (Raytracing_n.cpp:932-941) at node
 * scale.  The scene is flattened once and uploaded to every device.  srr_render,
 * srr_render_device, srr_render_device_async and srr_render_wait on the handle
 * render the WHOLE frame (shard_index / shard_count must be 0 / 0 or 1): tiles of
 * edge p->tile (<= 0: 32) dealt round-robin over the devices, each tile row
 * rotated by one (srr_shard_pixels with shard_count = n_devices), all devices at
 * once, then ONE frame-end gather of the packed shard slabs to device_ids[0] over
 * RCCL (ncclCommInitAll communicator, ncclSend / ncclRecv in one group) and a
 * scatter into the image there: d_mean is a device_ids[0] pointer of nx*ny*3
 * floats, bitwise the one-device frame.  srr_render / srr_render_device return
 * after the gather; srr_render_device_async enqueues the gather on the GPU behind
 * the shards' frames (and behind the caller's legacy-stream work on device_ids[0])
 * and returns at once -- the host waits only in srr_render_wait.
 * device_ids may repeat a device (a rehearsal on one GPU): the gather is then
 * device copies, as with SRR_MULTI_TRANSPORT=copy.  No KEEP_PATHS / CONTINUE
 * (SRR_EINVAL); srr_accum_* and srr_copy_paths are single-device. */
int srr_renderer_create_multi(const srr_scene* s, int n_devices, const int* device_ids, srr_renderer** out);
/* Devices a renderer renders on (1 for srr_renderer_create), ids into
 * device_ids[0 .. cap) (may be NULL). */
int srr_renderer_devices(const srr_renderer* r, int* device_ids, int cap);
/* The frame-end transport of a renderer: "rccl", "copy", or "none" (one device). */
const char* srr_renderer_transport(const srr_renderer* r);
/* The multi-device frame's bookkeeping, host only (no GPU): shard k's pixels are
 * srr_shard_pixels({.., shard_index k, shard_count n_devices}); the gather packs
 * the shards' slabs in shard order, so packed entry i is image pixel
 * gather_index[i] (nx*ny entries, may be NULL) and shard k's slab starts at
 * shard_offsets[k] (n_devices + 1 entries, may be NULL).  Returns nx*ny. */
int64_t srr_multi_plan(const srr_params* p, int n_devices, int32_t* gather_index, int64_t* shard_offsets);
/* Number of pixels this shard renders, and their PPM-order indices (row 0 =
 * top, Raytracing_n.cpp:873-876) into pixel_index[] (may be NULL). */
int64_t srr_shard_pixels(const srr_params* p, int32_t* pixel_index);
/* Render this shard.  d_mean: DEVICE pointer, n_shard_pixels*3 floats -- the
 * per-pixel mean of de_nan'd samples before the sqrt (Raytracing_n.cpp:841-848),
 * in srr_shard_pixels() order.  Inputs are resident on the device; the call
 * returns after the device work finished. */
int srr_render_device(srr_renderer* r, const srr_params* p, float* d_mean, srr_stats* stats);
/* Frame pipelining (no reference counterpart: the reference renders one frame
 * per run).  Enqueue the same frame as srr_render_device and return at once with
 * a ticket; the renderer keeps two frames in flight on two streams, so a frame's
 * persistent blocks start on the CUs the previous frame's last paths free.  Fresh
 * frames of the path engine only (no CONTINUE, KEEP_PATHS, COUNT_VISITS,
 * WAVEFRONT: SRR_EINVAL).  d_mean must not be read, and must not be the target
 * of another frame in flight, before srr_render_wait(ticket) returns; enqueueing
 * a third frame first finishes the oldest (its stats stay for its wait).
 * Device memory: each frame in flight holds its own sample window (all shard
 * pixels x the window's samples x 12 B, at most SRR_WINDOW_MB, default 16 GiB),
 * bounce records (16 B x max_depth per persistent lane) and sums; the
 * synchronous slot keeps its own window too, so alternating the two modes
 * reallocates nothing (the other mode's windows are given back only when an
 * allocation would run the device out of memory).  Per renderer the windows are
 * thus at most 3 x SRR_WINDOW_MB; the peers of a multi-device renderer that share
 * a device (device_ids repeating it) split SRR_WINDOW_MB between them, so a
 * device holds at most 3 x SRR_WINDOW_MB of windows either way. */
int srr_render_device_async(srr_renderer* r, const srr_params* p, float* d_mean, int64_t* ticket);
/* Wait for an async frame and return its stats (each ticket once). */
int srr_render_wait(srr_renderer* r, int64_t ticket, srr_stats* stats);
/* Host convenience (the CRender::Run of Render.h:16-51): the shard's pixels
 * (the whole image when shard_count <= 1) as mean radiance (npix*3, may be NULL)
 * and 8-bit tone-mapped rgb8 (npix*3, Raytracing_n.cpp:850-867, may be NULL). */
int srr_render(srr_renderer* r, const srr_params* p, float* mean, unsigned char* rgb8, srr_stats* stats);
/* ---- Adaptive sampling (no reference counterpart: the reference gives every
 * pixel ns samples, Raytracing_n.cpp:41).  The frame is rendered in passes; in
 * each pass every still-active pixel receives w = min(batch_spp, p->spp - n)
 * samples with the global sample indices [n, n + w), n being the samples it holds
 * (the same for every active pixel: pixels only ever retire).  After a pass a
 * pixel retires when n reached the budget p->spp, or when n >= min_spp,
 * rel_tol > 0 and the convergence rule below holds; the frame ends when no pixel
 * is active.  A pixel that ends with n_i samples holds bitwise the value a
 * fixed-spp frame of spp = n_i gives it.
 *
 * Convergence rule.  Per sample (after de_nan) the luminance is
 *   y = (0.2126f*r + 0.7152f*g) + 0.0722f*b          (Rec. 709 weights)
 * and the pixel keeps s1 += y, s2 += y*y, folded in sample order in float32.
 * With nf = (float)n the pixel is converged iff, every operation in float32,
 * evaluated in exactly this order and without fused multiply-add,
 *   (s2*nf - s1*s1) <= ((rel_tol*rel_tol) * (nf - 1.0f)) * ((s1 + abs_eps*nf) * (s1 + abs_eps*nf))
 * Origin (nothing of it is the reference's): the standard error of the mean of n
 * samples is sem = sqrt(var / n) with the unbiased var = (s2 - s1*s1/n) / (n - 1);
 * the test sem <= rel_tol * (mean + abs_eps), mean = s1/n, squared and multiplied
 * through by n*n*(n - 1), is the inequality above: no division, no square root.
 * rel_tol = 0 never retires a pixel early (the rule itself holds for a pixel of
 * zero variance, so the pass loop does not ask it then).  Early stopping biases
 * dark pixels lit by rare events: min_spp is the guard. */
typedef struct srr_adaptive_params {
  uint32_t struct_size; /* sizeof(srr_adaptive_params) of the caller              */
  int batch_spp;        /* samples every still-active pixel receives per pass, >= 1 */
  int min_spp;          /* no pixel retires with fewer samples than this, >= 1    */
  float rel_tol;        /* target relative standard error of the pixel's mean     */
                        /*   luminance; 0 = never retire                          */
  float abs_eps;        /* luminance floor added to the mean in the test, >= 0    */
} srr_adaptive_params;

typedef struct srr_adaptive_stats {
  uint32_t struct_size;    /* sizeof(srr_adaptive_stats) of the caller (set before the call) */
  int32_t passes;          /* k_paths passes actually launched                    */
  int64_t paths;           /* camera paths traced = sum of the per-pixel counts   */
  int64_t world_rays;
  int64_t pixels_retired;  /* pixels that met the tolerance before the budget     */
  double total_ms;
} srr_adaptive_stats;

/* Render this shard adaptively: p->spp is the per-pixel budget, p->sample_begin
 * must be 0.  d_mean: DEVICE pointer, n_shard_pixels*3 floats, pixel i's mean over
 * its own n_i samples (sum * (float)(1.0 / (float)n_i), the division of a
 * fixed-spp frame); d_count: DEVICE pointer, n_shard_pixels int32 (n_i), may be
 * NULL; both in srr_shard_pixels() order.  Synchronous, one device, path engine
 * only: SRR_EINVAL, before anything is enqueued, for a multi-device renderer, for
 * SRR_FLAG_CONTINUE / KEEP_PATHS / COUNT_VISITS / WAVEFRONT / SUMS, for
 * batch_spp < 1, min_spp < 1, a negative or NaN rel_tol or abs_eps, and for a
 * struct_size smaller than the struct above.  The call invalidates the renderer's
 * progressive running sums: no SRR_FLAG_CONTINUE render may follow it without a
 * fresh render or srr_accum_set first. */
int srr_render_adaptive(srr_renderer* r, const srr_params* p, const srr_adaptive_params* a, float* d_mean,
                        int32_t* d_count, srr_adaptive_stats* stats);
/* Host convenience, as srr_render is to srr_render_device: the shard's means
 * (npix*3, may be NULL), counts (npix, may be NULL) and tone-mapped rgb8 (npix*3,
 * may be NULL) in host buffers. */
int srr_render_adaptive_host(srr_renderer* r, const srr_params* p, const srr_adaptive_params* a, float* mean,
                             int32_t* count, unsigned char* rgb8, srr_adaptive_stats* stats);
/* The convergence rule above on the host (no GPU): 1 converged, 0 not. */
int srr_adaptive_converged(int32_t n, float s1, float s2, float rel_tol, float abs_eps);

/* ---- Resuming an adaptive frame.  The ADAPTIVE STATE of a renderer is, per slot i
 * of the shard's pixel list (srr_shard_pixels() order): n_i, the samples held
 * (int32); sums_i, the rgb sums (3 floats); (s1_i, s2_i), the luminance moments.  A
 * successful srr_render_adaptive leaves it, and so do a successful
 * srr_render_adaptive_resume and srr_adaptive_state_set.
 *
 * For the parameters of a call (B = p->spp, batch_spp, min_spp, rel_tol, abs_eps) a
 * slot is RETIRED iff n_i >= B, or n_i >= min_spp, rel_tol > 0 and
 * srr_adaptive_converged(n_i, s1_i, s2_i, rel_tol, abs_eps).  The resume loop: while
 * some slot is not retired,
 *   1. n = the smallest n_i over the slots that are not retired;
 *   2. the pass's active list is the not retired slots with n_i == n, in ascending
 *      slot order;
 *   3. w = min(batch_spp, B - n);
 *   4. each active slot receives the samples with the global indices [n, n + w),
 *      folded in sample order by the fold of the fresh frame;
 *   5. n_i = n + w.
 * Retirement is evaluated afresh from the state after every pass, so slots that
 * retired at different counts can become active again under a tighter tolerance,
 * and levels merge as the lower one catches up.  Samples are never removed: a slot
 * with n_i > B (the budget was lowered) is simply retired.  A slot with n_i == 0
 * starts from zero sums and moments, whatever the state holds for it.  From an
 * all-zero state this loop is exactly the loop of srr_render_adaptive.  A path
 * depends only on (pixel, global sample index), so a slot that ends with n_i samples
 * holds bitwise the fixed-spp frame of spp = n_i, however many calls it took.
 *
 * srr_render_adaptive_resume: arguments as srr_render_adaptive.  On return d_mean
 * and d_count (may be NULL) are written for EVERY slot, also for those that never
 * became active in this call: sum * (float)(1.0 / (float)n_i), and n_i.  stats:
 * passes, paths and world_rays cover this call only; pixels_retired is the number of
 * slots that end with n_i < p->spp (for a fresh frame that is the same number).
 * SRR_EINVAL, before anything is enqueued: in every case in which
 * srr_render_adaptive refuses; for a renderer that holds no valid adaptive state;
 * for a frame whose nx, ny, tile, shard_index or shard_count differs from the one
 * the state belongs to; and for a state whose rgb sums have been overwritten since:
 * they live in the progressive accumulator, which a synchronous srr_render /
 * srr_render_device and srr_accum_set write (srr_adaptive_variance, which needs only
 * the moments, keeps working after those).  max_depth, base_seed and the scene are
 * not checked: continuing with others is the caller's responsibility, as with
 * srr_accum_set.  A resume that fails after it has started leaves no valid state. */
int srr_render_adaptive_resume(srr_renderer* r, const srr_params* p, const srr_adaptive_params* a, float* d_mean,
                               int32_t* d_count, srr_adaptive_stats* stats);
/* Host convenience, as srr_render_adaptive_host. */
int srr_render_adaptive_resume_host(srr_renderer* r, const srr_params* p, const srr_adaptive_params* a, float* mean,
                                    int32_t* count, unsigned char* rgb8, srr_adaptive_stats* stats);
/* The adaptive state into host buffers: sums (npix*3), mom (npix*2: s1, s2) and
 * count (npix), any of which may be NULL; *npix (may be NULL) = its slots.
 * SRR_EINVAL for a multi-device renderer, a renderer without a valid state, and for
 * sums != NULL when the rgb sums have been overwritten since. */
int srr_adaptive_state_get(srr_renderer* r, float* sums, float* mom, int32_t* count, int64_t* npix);
/* Install a state from host buffers (none may be NULL).  p names the frame it belongs
 * to (nx, ny, tile, shard_index, shard_count; nothing else of p is read); SRR_EINVAL
 * unless npix == srr_shard_pixels(p) and every count >= 0, and for a multi-device
 * renderer.  Like srr_render_adaptive it invalidates the progressive running sums. */
int srr_adaptive_state_set(srr_renderer* r, const srr_params* p, const float* sums, const float* mom,
                           const int32_t* count, int64_t npix);

/* ---- Speculative passes: the same adaptive frame in fewer, larger passes.  After the
 * first pass only a few slots stay active, and a pass of few paths is bound by k_paths'
 * ramp and drain and by the host round trip behind it.  Under this setting a pass at
 * level n (the count its n_active slots hold) gives every slot
 *   kmax = max(1, pass_spp_max / batch_spp)                      (integer division)
 *   k    = clamp(fill_paths / (n_active * batch_spp), 1, kmax)   (integer division, 64-bit)
 *   w    = min(k * batch_spp, B - n)
 * samples in one k_paths launch, and its fold asks the retirement rule at every count
 * n + batch_spp, n + 2*batch_spp, ... and n + w: a slot stops at the first of them where
 * it is retired, and the samples traced for it beyond that count are thrown away; a
 * slot that reaches n + w unretired stays live there.  k = 1 is the pass of the loops
 * above.  A slot is asked at exactly the counts at which those loops ask it, from
 * moments folded from the same samples in the same order, and nothing past its stop is
 * folded: the state and every output of a frame are bit for bit what they are without
 * speculation, whatever pass_spp_max and fill_paths are.
 *
 * srr_adaptive_speculate sets it for srr_render_adaptive / _resume (and their _host
 * forms) on this renderer, from the next such call on, until changed.  pass_spp_max: the
 * most samples a pass may give a slot; a value below 2 * batch_spp of a call (0, the
 * default, among them) switches speculation off for that call, which then launches
 * exactly what it launches today.  fill_paths: the pass size the schedule aims at, in
 * paths; 0 = srr_adaptive_fill_default().  SRR_EINVAL for a negative argument and for
 * a multi-device renderer.
 *
 * srr_adaptive_stats under speculation: paths stays the samples added to the per-pixel
 * counts in the call (paths_traced - paths_discarded below); pixels_retired keeps its
 * meaning and value; passes counts the passes launched, so it shrinks; world_rays counts
 * the rays of every traced path, the discarded ones included, so identities between
 * world_rays and those of fixed-spp frames hold only with speculation off (or where
 * nothing was discarded).
 *
 * srr_adaptive_last_spec_stats: the launches of the most recent successful adaptive or
 * resume call on the renderer, with or without speculation.  SRR_EINVAL for a NULL
 * argument, a struct_size smaller than the struct, a multi-device renderer, and before
 * any such call has succeeded.
 * srr_adaptive_pass_width: w of the schedule above on the host (no GPU); SRR_EINVAL
 * unless n_active >= 1, 0 <= n < budget, batch_spp >= 1, pass_spp_max >= 0 and
 * fill_paths >= 0. */
int srr_adaptive_speculate(srr_renderer* r, int pass_spp_max, int64_t fill_paths);
typedef struct srr_adaptive_spec_stats {
  uint32_t struct_size;     /* sizeof(srr_adaptive_spec_stats) of the caller (set before the call) */
  int32_t windows;          /* k_paths launches of the most recent adaptive call */
  int64_t paths_traced;     /* camera paths those launches traced                 */
  int64_t paths_discarded;  /* of them, traced past their slot's stopping count   */
} srr_adaptive_spec_stats;
int srr_adaptive_last_spec_stats(const srr_renderer* r, srr_adaptive_spec_stats* out);
int srr_adaptive_pass_width(int64_t n_active, int n, int budget, int batch_spp, int pass_spp_max,
                            int64_t fill_paths);
/* The fill_paths that 0 stands for. */
int64_t srr_adaptive_fill_default(void);

/* ---- Variance of a pixel's mean luminance, from the moments (s1, s2) that the
 * adaptive frame keeps for the rule above, for a pixel that holds n samples.  Every
 * operation in float32, in exactly this order, without fused multiply-add; rdiv is
 * IEEE division.  With nf = (float)n:
 *   n < 2:     v = s1*s1
 *   otherwise: d = s2*nf - s1*s1;  if !(d > 0) then d = 0  (this also catches NaN);
 *              v = rdiv(d, (nf*nf) * (nf - 1.0f))
 * Origin, as for the convergence rule: var(mean) = (s2 - s1*s1/n) / (n (n - 1)), the
 * unbiased sample variance over n, multiplied through by n so that one division is
 * left.  n < 2 has no sample variance: a one-sample pixel gets the prior of 100 %
 * relative error, v = mean^2 = s1*s1.
 * srr_variance_of_mean evaluates it on the host (no GPU) by the code the kernel runs.
 *
 * srr_adaptive_variance reads the moments left by the most recent SUCCESSFUL
 * srr_render_adaptive (or resume, or srr_adaptive_state_set: the adaptive state above)
 * on this renderer (npix = that frame's shard pixel count) and
 * d_count[i], that frame's counts (DEVICE pointer, npix int32: what the frame wrote
 * to its d_count), and writes d_var[i] (DEVICE pointer, npix floats), both in
 * srr_shard_pixels() order.  One small kernel on the renderer's synchronous stream;
 * the call returns after it.  SRR_EINVAL, before anything is enqueued, for a NULL
 * argument, a multi-device renderer, and a renderer that holds no valid adaptive
 * frame (none rendered yet, or the most recent one failed after it had started).  No
 * other render entry touches the moments: srr_render_device, srr_render_aov and the
 * async frames may run in between.
 * A fixed-spp frame with variance is srr_render_adaptive with rel_tol = 0 and
 * batch_spp = min_spp = spp: one pass, whose image and world rays are bitwise those
 * of srr_render_device at that spp. */
float srr_variance_of_mean(int32_t n, float s1, float s2);
int srr_adaptive_variance(srr_renderer* r, const int32_t* d_count, float* d_var);
/* The same with host buffers. */
int srr_adaptive_variance_host(srr_renderer* r, const int32_t* count, float* var);

/* ---- First-hit feature buffers (AOVs) for a denoiser (no reference counterpart).
 * For every shard pixel and every sample of [p->sample_begin, p->sample_begin +
 * p->spp) the PRIMARY ray of the beauty frame is traced (the same per-path seed,
 * Sobol point, lens draw and time as that sample of srr_render_device) and tested
 * with world->hit(r, 0.001, FLT_MAX).  Per sample:
 *   albedo  by the hit's material: lambertian, orennayar, beckmann, diffuse_light,
 *           isotropic: the material's texture at the hit's (u, v, p); metal: its
 *           colour; dielectric: (1, 1, 1); a null material or a miss: (0, 0, 0).
 *           It does not depend on the face that was hit.
 *   normal  the hit record's normal as color() sees it (after the instance
 *           transforms and flip_normals); (0, 0, 0) for a miss and for a
 *           constant_medium hit (whose normal the reference sets arbitrarily).
 *   depth   sqrtf(dot(p - o, p - o)), o the ray origin, p the hit point; 0 for a miss.
 * Every component is de_nan'd and summed per pixel in sample order in float32;
 * the result is sum * (float)(1.0 / (float)spp), the fold of the beauty frame: a
 * buffer is a pure function of (scene, pixel, sample range).
 * d_albedo, d_normal: DEVICE pointers of n_shard_pixels*3 floats; d_depth: DEVICE
 * pointer of n_shard_pixels floats; all in srr_shard_pixels() order; a buffer may
 * be NULL when its bit in `which` is clear.  p->max_depth and p->batch_paths
 * (paths per batch, 0 = auto) are read as by srr_render_device.  Synchronous.
 * SRR_EINVAL, before anything is allocated or enqueued, for a multi-device
 * renderer, for SRR_FLAG_CONTINUE / KEEP_PATHS / COUNT_VISITS / SUMS, for which ==
 * 0 or unknown bits in it, and for a needed pointer that is NULL.  The call uses
 * buffers and a stream of its own: the renderer's progressive running sums, held
 * pixel list and async frames are untouched (a SRR_FLAG_CONTINUE render after it
 * continues as if it had not happened). */
#define SRR_AOV_ALBEDO 1
#define SRR_AOV_NORMAL 2
#define SRR_AOV_DEPTH 4
int srr_render_aov(srr_renderer* r, const srr_params* p, int which, float* d_albedo, float* d_normal,
                   float* d_depth);
/* The same with host buffers. */
int srr_render_aov_host(srr_renderer* r, const srr_params* p, int which, float* albedo, float* normal, float* depth);

/* ---- First-diffuse-hit feature buffers: the AOVs above, traced through mirrors and
 * glass to the first hit that is neither metal nor dielectric (what OIDN, OptiX and
 * SVGF call guides "at the first non-specular hit").  No reference counterpart.
 * Chain.  For every shard pixel and sample the path starts as that sample of
 * srr_render_device starts (per-path seed, Sobol point, lens draw, time) and keeps that
 * path's RNG streams from then on.  depth = 0, ray r_0 = the primary ray; then, as
 * color() (Raytracing_n.cpp:56-105):
 *   1. world->hit(r_depth, 0.001, FLT_MAX); a constant_medium draws inside hit what it
 *      draws in the beauty frame.  o_j is the origin of r_j, p_j its hit point.
 *   2. While the hit's material is metal or dielectric AND depth < p->max_depth: a_depth
 *      = the metal's colour or (1, 1, 1); the material's scatter draws exactly what it
 *      draws in the beauty frame (metal: random_in_unit_sphere; dielectric: one drand)
 *      and gives r_(depth+1), time 0; depth += 1; step 1 again.
 *   3. Any other result is TERMINAL, k = depth bounces behind it: a miss, a null
 *      material, a non-specular material (isotropic is not followed: a medium is a
 *      terminal hit), or a metal / dielectric reached with depth == p->max_depth.
 * Per sample:
 *   albedo  e = the terminal hit's albedo by srr_render_aov's rule, but (0, 0, 0) for a
 *           metal or dielectric at the depth limit (color() returns emitted() there);
 *           albedo = a_0 * (a_1 * ( ... (a_(k-1) * e))), folded back to front,
 *           componentwise in float32 -- the order in which the recursion returns.
 *   normal  the terminal hit's normal as color() sees it (world space, not reflected
 *           back); (0, 0, 0) for a miss, a constant_medium and a chain stopped at the
 *           depth limit.
 *   depth   d_j = sqrtf(dot(p_j - o_j, p_j - o_j)) per segment, summed front to back in
 *           float32, ((d_0 + d_1) + d_2) + ... + d_k; 0 when the last segment misses.
 * De_nan, the per-pixel fold in sample order and sum * (float)(1.0 / (float)spp) are
 * exactly srr_render_aov's.  Consequences: on a scene without metal and dielectric the
 * three buffers are bitwise srr_render_aov's; a buffer is a pure function of (scene,
 * pixel, sample range, max_depth), whatever p->batch_paths; and the albedo is, bit for
 * bit, the beauty image of the scene's "specular twin" (every material but metal and
 * dielectric replaced by a two-sided diffuse_light of its albedo) at the same max_depth.
 * stats (may be NULL; set stats->struct_size = sizeof(srr_aov_stats) before the call):
 * paths = primary rays; world_rays = world->hit calls, primary rays included;
 * chained_paths = paths that took at least one specular step (first hit metal or
 * dielectric, max_depth > 0); longest_chain = the most steps any path took.
 * Buffers, `which`, p->max_depth (0..64) and p->batch_paths as for srr_render_aov; with
 * batch_paths = 0 the batch is min(2^20, 256 MiB / (172 + 12 * max_depth) B) paths, so
 * that the per-path state of this call's batch (172 B + 12 B per bounce of max_depth)
 * stays within 256 MiB; the 160 B per path of it that are srr_render_aov's buffers are
 * shared with that call and keep the largest batch either has used.  Synchronous.
 * SRR_EINVAL, before
 * anything is allocated or enqueued, in every case srr_render_aov refuses, and for a
 * stats->struct_size smaller than the struct.  Like srr_render_aov the call uses buffers
 * and a stream of its own and leaves running sums, the held pixel list, adaptive state
 * and async frames untouched. */
typedef struct srr_aov_stats {
  uint32_t struct_size;   /* sizeof(srr_aov_stats) of the caller, set before the call */
  int32_t  longest_chain; /* most specular bounces any path followed */
  int64_t  paths;         /* primary rays traced */
  int64_t  world_rays;    /* world->hit calls, primary rays included */
  int64_t  chained_paths; /* paths whose first hit was metal or dielectric (and was followed) */
} srr_aov_stats;
int srr_render_aov_through(srr_renderer* r, const srr_params* p, int which, float* d_albedo, float* d_normal,
                           float* d_depth, srr_aov_stats* stats /* may be NULL */);
/* The same with host buffers. */
int srr_render_aov_through_host(srr_renderer* r, const srr_params* p, int which, float* albedo, float* normal,
                                float* depth, srr_aov_stats* stats /* may be NULL */);

/* ---- Emission buffer: the light a camera path sees before its first diffuse bounce, the
 * part of a frame a denoiser should take out before it filters (SVGF filters emission
 * apart).  No reference counterpart.  srr_render_aov_emission is srr_render_aov
 * (through_specular == 0) or srr_render_aov_through (through_specular == 1) with a fourth
 * buffer: `which` is a non-empty set of the four SRR_AOV_* bits, d_albedo, d_normal, d_depth
 * and stats mean exactly what they mean in that call (first hit: paths = world_rays = primary
 * rays, chained_paths = longest_chain = 0), and d_emission is a DEVICE pointer of
 * n_shard_pixels*3 floats in srr_shard_pixels() order.  Per sample:
 *   First hit.  emission = emitted() of the primary ray's hit as color() evaluates it
 *     (Raytracing_n.cpp:61, material.h:348-354): the diffuse_light's texture at the hit's
 *     (u, v, p) when dot(normal, ray direction) < 0; (0, 0, 0) for every other material, a
 *     null material, the back of a light and a miss.  Unlike the albedo it depends on the
 *     face that was hit.
 *   Through specular.  e = emitted() of the terminal hit of srr_render_aov_through's chain,
 *     (0, 0, 0) for a metal or dielectric reached at the depth limit;
 *     emission = a_0 * (a_1 * ( ... (a_(k-1) * e))), folded back to front, componentwise in
 *     float32: the same records in the same order as the albedo.
 * De_nan, the per-pixel fold in sample order over [p->sample_begin, p->sample_begin + p->spp)
 * and sum * (float)(1.0 / (float)n) are srr_render_aov's.  Consequences: the first-hit
 * emission is bitwise srr_render_device at max_depth = 0; the through-specular emission is
 * bitwise the beauty frame of the scene's "emission twin" (metal, dielectric and
 * diffuse_light kept, every other material replaced by a diffuse_light of a constant
 * (0, 0, 0) texture) at the same max_depth, on every pixel, with no lit-pixel mask; on a
 * scene without metal and dielectric the two emissions are bitwise equal.  An isotropic
 * terminal hit emits 0.
 * d_count (DEVICE pointer, n_shard_pixels int32, may be NULL; read for the emission buffer
 * only): pixel i's emission is folded over its first n_i = d_count[i] samples of the range
 * and divided by n_i, the division of a fixed-spp frame of that count, so that an adaptive
 * frame, where pixel i holds n_i samples, can subtract the emission of exactly the samples
 * it holds.  A count outside 1..p->spp is clamped into it (the _host form refuses it
 * instead).  NULL means p->spp for every pixel.  Albedo, normal and depth ignore it.
 * Batches: with batch_paths = 0, first hit as srr_render_aov; through specular
 * min(2^20, 256 MiB / (188 + 12 * max_depth) B) paths when bit 8 is set (a path's emission
 * values are 16 B of their own, allocated the first time bit 8 is asked for; the state and
 * default batches of the two calls above are unchanged), else as srr_render_aov_through.
 * Synchronous.  SRR_EINVAL, before anything is allocated or enqueued, in every case those
 * calls refuse (with the fourth bit known), for a NULL d_emission with bit 8 set, for
 * through_specular outside 0 / 1, and in the _host form for a count outside 1..p->spp.  Like
 * them it uses the AOV stream and buffers and leaves running sums, the held pixel list,
 * adaptive state and async frames untouched. */
#define SRR_AOV_EMISSION 8
int srr_render_aov_emission(srr_renderer* r, const srr_params* p, int which, int through_specular, float* d_albedo,
                            float* d_normal, float* d_depth, float* d_emission,
                            const int32_t* d_count /* may be NULL */, srr_aov_stats* stats /* may be NULL */);
/* The same with host buffers. */
int srr_render_aov_emission_host(srr_renderer* r, const srr_params* p, int which, int through_specular, float* albedo,
                                 float* normal, float* depth, float* emission,
                                 const int32_t* count /* may be NULL */, srr_aov_stats* stats /* may be NULL */);

/* ---- Feature-guided denoiser: an edge-avoiding a-trous wavelet filter (Dammertz,
 * Sewtz, Hanika, Lensch 2010) over a colour image and the AOVs above.  Nothing of it
 * is the reference's.  Inputs and the output are whole images in PPM order on HIP
 * device `device`: nx*ny*3 floats (colour, albedo, normal, output), nx*ny floats
 * (depth).  d_out must not overlap an input.
 *
 * Definition: every operation in float32, in exactly this order, without fused
 * multiply-add; rdiv is IEEE division, rexp the float exponential of the host libm
 * (expf), both as srr_device_libm exposes them.  c colour, a albedo, n normal, z depth.
 *   Demodulate (SRR_DENOISE_DEMODULATE): per channel x = rdiv(c, a + 1e-3f); else x = c.
 *   Iteration k = 0 .. iterations-1, step s = 1 << k, kc = k_c * 4^k (the factor is a
 *   power of two: exact).  For pixel p visit the taps (dy, dx), dy = -2..2 outer,
 *   dx = -2..2 inner, q = p + s*(dx, dy); a tap outside the image is skipped.
 *     h  = B[|dx|] * B[|dy|],  B = {0.375f, 0.25f, 0.0625f}  (exact products)
 *     dc = ((xq.r-xp.r)^2 + (xq.g-xp.g)^2) + (xq.b-xp.b)^2   (x of this iteration's input)
 *     dn = the same form on the normals
 *     dz = rdiv((zp-zq)*(zp-zq), (zp*zp + zq*zq) + 1e-20f)
 *     w  = h * rexp(-((dc*kc + dn*k_n) + dz*k_z))
 *     sum.ch += w * xq.ch per channel (r, g, b);  wsum += w      (both start at 0)
 *   x'p.ch = rdiv(sum.ch, wsum)   (the centre tap makes wsum >= 9/64)
 *   Remodulate (SRR_DENOISE_DEMODULATE): out = x * (a + 1e-3f); else out = x.
 * tests/denoise_ref.py restates this in numpy, bit for bit.
 * SRR_EINVAL, before the GPU is touched, for nx or ny outside 1..65536 or nx*ny > 2^28,
 * iterations outside 1..6, a negative or non-finite k_c / k_n / k_z, unknown flags,
 * a struct_size smaller than the struct below, a NULL buffer, and an output that
 * overlaps an input. */
#define SRR_DENOISE_DEMODULATE 1
typedef struct srr_denoise_params {
  uint32_t struct_size; /* sizeof(srr_denoise_params) of the caller */
  int iterations;       /* 1..6 */
  float k_c, k_n, k_z;  /* edge-stopping strengths of colour, normal, depth: >= 0, finite */
  int flags;            /* SRR_DENOISE_DEMODULATE */
} srr_denoise_params;
/* The defaults (the sweep of DESIGN.md §4.2): struct_size, 3 iterations, k_c 256, k_n 32,
 * k_z 64, no flags (SRR_DENOISE_DEMODULATE wins at 64 spp and loses at 16: see there). */
int srr_denoise_defaults(srr_denoise_params* dp);
int srr_denoise(int device, int nx, int ny, const srr_denoise_params* dp, const float* d_color,
                const float* d_albedo, const float* d_normal, const float* d_depth, float* d_out);
/* The same with host buffers. */
int srr_denoise_host(int device, int nx, int ny, const srr_denoise_params* dp, const float* color,
                     const float* albedo, const float* normal, const float* depth, float* out);

/* ---- Variance-guided denoiser: the a-trous filter above with the colour term of
 * Schied, Kaplanyan, Wyman et al. 2017 (SVGF), section 4.4: the luminance tolerance of
 * a pixel is the standard deviation of its own estimate, and the variance is carried
 * through the iterations.  Nothing of it is the reference's.  Images as for
 * srr_denoise; d_var and d_var_out hold nx*ny floats, the variance of each pixel's
 * mean luminance (srr_adaptive_variance, scattered into PPM order) and that of the
 * filtered pixel; d_var_out may be NULL.  d_out and d_var_out must overlap neither
 * an input nor each other.
 *
 * Definition: every operation in float32, in exactly this order, without fused
 * multiply-add; rdiv and rexp as in srr_denoise, rsqrt the correctly rounded square
 * root; lum(x) = (0.2126f*x.r + 0.7152f*x.g) + 0.0722f*x.b.
 *   Set-up.  Without SRR_DENOISE_DEMODULATE x = c and v = var.  With it, per channel
 *     m.ch = a.ch + 1e-3f, x.ch = rdiv(c.ch, m.ch);  la = lum(m);  v = rdiv(var, la*la).
 *   Iteration k = 0 .. iterations-1, s = 1 << k.  For pixel p:
 *     Variance prefilter, always over the ADJACENT pixels (not the dilated ones): taps
 *       (dy, dx), dy = -1..1 outer, dx = -1..1 inner, a tap outside the image skipped;
 *       G = {0.25f centre, 0.125f edge, 0.0625f corner};  gs += G*vq;  gw += G
 *       (both start at 0);  vbar = rdiv(gs, gw).
 *     den = k_l * rsqrt(vbar) + 1e-6f;  lp = lum(xp).
 *     Wavelet taps exactly as in srr_denoise: dy = -2..2 outer, dx inner,
 *       q = p + s*(dx, dy), a tap outside the image skipped, h = B[|dx|]*B[|dy|].
 *       dl = fabsf(lum(xq) - lp);  wl = rdiv(dl, den)
 *       dn, dz as in srr_denoise
 *       w  = h * rexp(-((wl + dn*k_n) + dz*k_z))
 *       sum.ch += w*xq.ch;  wsum += w;  vsum += (w*w)*vq      (all start at 0)
 *     x'p.ch = rdiv(sum.ch, wsum);  v'p = rdiv(vsum, wsum*wsum)
 *       (the centre tap makes wsum >= 9/64)
 *   Output.  out = x, or x.ch * m.ch with SRR_DENOISE_DEMODULATE;
 *            var_out = v, or v * (la*la) with it.
 * (k_l = 0 leaves den = 1e-6f: pixels then average only with neighbours of their own
 * luminance.  A large k_l, not 0, switches the luminance term off.)
 * tests/denoise_var_ref.py restates this in numpy, bit for bit.
 * SRR_EINVAL, before the GPU is touched, for the sizes srr_denoise refuses, iterations
 * outside 1..6, a negative or non-finite k_l / k_n / k_z, unknown flags, a struct_size
 * smaller than the struct below, a NULL buffer other than d_var_out, and an output
 * that overlaps an input or the other output. */
typedef struct srr_denoise_var_params {
  uint32_t struct_size; /* sizeof(srr_denoise_var_params) of the caller */
  int iterations;       /* 1..6 */
  float k_l, k_n, k_z;  /* luminance tolerance in standard deviations; normal, depth strengths: >= 0, finite */
  int flags;            /* SRR_DENOISE_DEMODULATE */
} srr_denoise_var_params;
/* The defaults (the sweep of DESIGN.md §4.3): struct_size, 3 iterations, k_l 2, k_n 128,
 * k_z 64, SRR_DENOISE_DEMODULATE (the plain filter scores better on the 16-spp frame of
 * the sweep's scene and smears a light that is in view: see there). */
int srr_denoise_var_defaults(srr_denoise_var_params* dp);
int srr_denoise_var(int device, int nx, int ny, const srr_denoise_var_params* dp, const float* d_color,
                    const float* d_var, const float* d_albedo, const float* d_normal, const float* d_depth,
                    float* d_out, float* d_var_out);
/* The same with host buffers. */
int srr_denoise_var_host(int device, int nx, int ny, const srr_denoise_var_params* dp, const float* color,
                         const float* var, const float* albedo, const float* normal, const float* depth, float* out,
                         float* var_out);

/* ---- Emission-separated filtering: srr_denoise / srr_denoise_var on the colour less the
 * emission buffer above, which is added back unfiltered.  A pixel on the rim of a light in
 * view averages samples of 0 and of the light; with the emission taken out, the step is gone
 * from the signal the filter sees and the light's edge stays where the renderer put it.
 * d_emission: nx*ny*3 floats in PPM order (srr_render_aov_emission over the samples the
 * colour holds).  The definitions are those above with two changes, in float32, without
 * fused multiply-add:
 *   Set-up.  Per channel c' = c - e, and c' takes the place of c: x = c - e, or with
 *     SRR_DENOISE_DEMODULATE x = rdiv(c - e, a + 1e-3f).
 *   Output.  Per channel out = y + e, y being what the unchanged definition writes (with
 *     the flag the remodulated x * (a + 1e-3f): the multiply and the add are two roundings).
 * The variance input and var_out are unchanged: var is the variance of lum(c), emission
 * included, so at a light's rim it overstates the variance of c - e, and the filter is more
 * permissive there, on a signal that no longer has the step.
 * tests/denoise_emission_ref.py restates both in numpy, bit for bit.
 * SRR_EINVAL as in the base calls; d_emission must not be NULL, and no output may overlap it. */
int srr_denoise_emission(int device, int nx, int ny, const srr_denoise_params* dp, const float* d_color,
                         const float* d_emission, const float* d_albedo, const float* d_normal, const float* d_depth,
                         float* d_out);
int srr_denoise_emission_host(int device, int nx, int ny, const srr_denoise_params* dp, const float* color,
                              const float* emission, const float* albedo, const float* normal, const float* depth,
                              float* out);
int srr_denoise_var_emission(int device, int nx, int ny, const srr_denoise_var_params* dp, const float* d_color,
                             const float* d_var, const float* d_emission, const float* d_albedo,
                             const float* d_normal, const float* d_depth, float* d_out, float* d_var_out);
int srr_denoise_var_emission_host(int device, int nx, int ny, const srr_denoise_var_params* dp, const float* color,
                                  const float* var, const float* emission, const float* albedo, const float* normal,
                                  const float* depth, float* out, float* var_out);

/* Progressive rendering with resume: the renderer's per-pixel running sums
 * (3 floats per shard pixel, in srr_shard_pixels order) and the samples per pixel
 * they hold.  get: sums may be NULL to query npix / samples.  set: restores a saved
 * state, after which renders with SRR_FLAG_CONTINUE and sample_begin = samples
 * continue it (bitwise the image of one render of all the samples). */
int srr_accum_get(srr_renderer* r, float* sums, int64_t* npix, int64_t* samples);
int srr_accum_set(srr_renderer* r, const float* sums, int64_t npix, int64_t samples);
/* After a render with SRR_FLAG_KEEP_PATHS: per-path raw radiance (before
 * de_nan) and world-ray counts, [n_shard_pixels][spp]. */
int srr_copy_paths(srr_renderer* r, float* radiance, unsigned char* rays);
/* ---- MERL measured isotropic BRDF tables (brdf.h).  The reference reads a
 * table (brdf::read_brdf, brdf.h:156-185) and looks values up by half/difference
 * angles (brdf::lookup_brdf_val, :190-214); its only user, brdfmaterial
 * (material.h:201-241), never sets a pdf and is never placed in a scene
 * (SURVEY Q23), so the lookup is exposed on its own. */
typedef struct srr_merl srr_merl;
/* brdf::read_brdf: int32 dims[3], then 3 * dims[0]*dims[1]*dims[2] doubles
 * (channel-major); the product must be 90*90*180 (else SRR_EINVAL, the
 * reference's "Dimensions don't match").  Uploads the table to HIP device `device`. */
int srr_merl_load(const char* path, int device, srr_merl** out);
/* The same from memory: n_doubles must be 3*90*90*180. */
int srr_merl_create(const double* table, int64_t n_doubles, int device, srr_merl** out);
void srr_merl_destroy(srr_merl* m);
/* brdf::lookup_brdf_val for n queries on the device.  angles: 4n doubles
 * (theta_in, fi_in, theta_out, fi_out); rgb: 3n doubles out (RED/GREEN/BLUE_SCALE
 * applied, brdf.h:11-13); cell: n table indices out (may be NULL).  Host buffers.
 * (The reference's "Below horizon." stderr message is not printed.) */
int srr_merl_lookup(srr_merl* m, int64_t n, const double* angles, double* rgb, int32_t* cell);

/* Tone map (Raytracing_n.cpp:850-867): 8-bit = clamp(int(255.99*sqrt(m))). */
int srr_tonemap(const float* mean, int64_t n_pixels, unsigned char* rgb8);
/* Write an ASCII P3 PPM (Raytracing_n.cpp:886, 873-876). */
int srr_write_ppm(const char* path, int nx, int ny, const unsigned char* rgb8);

/* PNG (8-bit RGB) of the tone-mapped image -- the output option next to PPM. */
int srr_write_png(const char* path, int nx, int ny, const unsigned char* rgb8);
/* stbi_load(path, x, y, comp, req_comp) (stb_image.h v2.19, used throughout
 * Raytracing_n.cpp): PNG, baseline JPEG, TGA.  *comp = the file's channels;
 * returns the channels in *out (req_comp, or *comp when req_comp is 0) or a
 * negative code.  Free *out with srr_image_free. */
int srr_image_load(const char* path, int req_comp, int* x, int* y, int* comp, unsigned char** out);
void srr_image_free(unsigned char* pixels);

/* Test infrastructure: run the device (HIP) implementation of one reference
 * function on KAT records laid out as oracle/ref/kat.inc writes them (inputs
 * first, outputs overwritten in place): "erf", "beckmann11", "beckmann_dist",
 * "beckmann_pdf", "cosine_pdf", "orennayar_pdf", "dielectric", "metal",
 * "triangle", "aabb", "camera", "lights", "light_list"; "sqrt" (records x,
 * sqrtf(x)); and the scene KATs, whose objects are built by the host scene calls
 * and flattened like a scene's: "sphere", "moving_sphere", "rect", "box", "xform",
 * "medium", "isotropic", "texture_checker", "texture_noise", "texture_image"
 * (layouts: tests/golden/README.md).  Needs a GPU. */
int srr_device_kat(const char* name, int n, int width, float* records);

/* Test infrastructure: the mesh walkers on the `mesh` KAT's records (width 21:
 * mesh o(3) d(3) tmin tmax is_medium | hit t tri p(3) n(3) u v; layouts and the
 * fixture scene: tests/golden/README.md).  scene_text's world is a list of `bvh`
 * objects over triangles, mesh m being its m-th; it is parsed, flattened and
 * uploaded as for a render, and one kernel runs the walker of `variant` on
 * every record: 0 the threaded BVH2 walk, 1 the 4-wide walk without pruning,
 * 2 with pruning (the default walk), 3 the quad-cooperative walk (n is padded to
 * whole waves of 64 with copies of the last record; a wave in which more than
 * quad_max lanes enter one mesh falls back to the per-lane walk).  stack_cap is
 * the LDS stack's depth (1 .. 8), use_gstack adds the per-lane global extension;
 * a deeper walk ends in the exact BVH2 re-walk.  tri is the triangle's position
 * in its bvh command.  Outputs are written in place.  Needs a GPU. */
int srr_device_mesh_kat(const char* scene_text, int variant, int quad_max, int stack_cap, int use_gstack, int n,
                        int width, float* records);

/* Test infrastructure: the world-list walk on the `world` KAT's records (width 24:
 * world o(3) d(3) time tmin tmax is_medium | hit t obj p(3) n(3) u v, two spare;
 * layouts and the fixture scene: tests/golden/README.md).  Text object 100000 + w of
 * scene_text, a list, is world w.  Each world that a record names is flattened and
 * uploaded on its own, exactly as a render of a scene with that world would be
 * (sphere runs grouped, object BVHs built), and one kernel per world runs the
 * frames' world hit and hit record on its records over [tmin, tmax]; an is_medium
 * record runs the list walk a medium makes over its boundary, which gives hit and t
 * only (refused on a world with a sphere group: a boundary's spheres are never
 * grouped).  tables 0 reads the world tables from global memory, 1 from the copy
 * staged in LDS (the default of the path kernel; each world must fit it).  obj is the
 * winning primitive's position in the depth-first listing of its world's leaves in
 * the file's order (a box is six rects), -1 on a miss.  Outputs are written in
 * place.  Needs a GPU. */
int srr_device_world_kat(const char* scene_text, int tables, int n, int width, float* records);

/* Test infrastructure, no GPU: how world `world` of a world-KAT scene flattens.
 * counts[0] objects in the flattened world list, [1] sphere groups among them,
 * [2] object BVHs among them, [3] primitives (leaves), [4] bytes of the packed
 * world tables (staged in LDS up to 8 KiB). */
int srr_world_kat_counts(const char* scene_text, int world, int32_t* counts);

/* Test infrastructure: one shading bounce on the `bounce` KAT's records (width 43:
 * l m p(3) n(3) u v o(3) d(3) time depth maxDepth lcg(2) pcg(4) | scattered
 * origin(3) dir(3) time colour(3) attempts lcg(2) pcg(4); layouts and the fixture
 * scene: tests/golden/README.md).  Text object 200000 + l of scene_text, a list, is
 * light list l, and material m is the scene's m-th `mat` line (every material must
 * be placed in the world, so that flattening keeps it).  Each light list that a
 * record names is flattened and uploaded with the scene's materials and textures
 * exactly as a render would, and one kernel per list runs its records: variant 0
 * through the wavefront engine's family_of, hit_emitted and scatter<family>, variant
 * 1 with diffuse records going through the path kernel's split bounce (set-up,
 * bsdf_dead, one skip_mixture round, coop_mixture with deep_tries, record), 64
 * records to a wave.  colour is the bounce record folded over a white next colour
 * as the path kernel folds it (a terminal record: its emission).  The attempts
 * column is left as it is.  Outputs are written in place.  Needs a GPU. */
int srr_device_bounce_kat(const char* scene_text, int variant, int deep_tries, int n, int width, float* records);

/* Test infrastructure, no GPU: how light list `list` of a bounce-KAT scene
 * flattens.  counts[0] lights, counts[1 + k] those of LightKind k (0 none: pdf 0
 * and no draws, 1 xz_rect, 2 sphere, 3 triangle), counts[5] materials kept. */
int srr_bounce_kat_counts(const char* scene_text, int list, int32_t* counts);

/* Test infrastructure: one math routine of the device build over n elements
 * (host buffers; one thread per element).  float elements: the wrappers the
 * kernels call, "rsin", "rcos", "rexp", "rlog", "rpow" (x, y), "racos", "rasin",
 * "ratan2" (y = x[], x = y[]: out0 = atan2f(x[i], y[i])), "rdiv" (x / y),
 * "atanf", and "sincosf" (out0 = sine, out1 = cosine).  double elements: the
 * MERL lookup's "sin64", "cos64", "sincos64" (two outputs), "acos64", "atan2_64"
 * (out0 = atan2(x[i], y[i])), the medium's "log64", and the device libm's raw
 * results, "ocml_sin", "ocml_cos", "ocml_pow5" (pow(x, 5.0)) behind the path
 * kernels' three double calls that use it, and "ocml_log".  y / out1 may be NULL
 * where the routine has one operand / one result.  Unknown names and bad
 * arguments: SRR_EINVAL, decided before the GPU is touched.  Otherwise needs a GPU. */
int srr_device_libm(const char* fn, int64_t n, const void* x, const void* y, void* out0, void* out1);

/* Test infrastructure: the kernels that turn samples into pixels, one launch wrapper
 * of kernels.h per call on host buffers (stream 0), so that what runs is what a frame
 * launches, the choice between a wrapper's kernels included.  One argument block serves
 * every kind; a kind reads the fields listed for it and ignores the rest.  Arrays
 * marked "io" are uploaded as given and downloaded after the launch, so what a kernel
 * leaves alone comes back as it went in.  "opt" arrays may be NULL.
 *
 *   "window"  launch_accumulate_window: sample[rows][spp][3]; sums io [n_slots][3] is acc
 *       (n_slots >= rows: the rows beyond are the caller's sentinel), init; mean opt io
 *       [n_slots][3] is `out`: the raw sums with ns == 0, else sums * (float)(1.0 / ns).
 *   "adaptive_fold"  launch_adaptive_fold (kernels.h AdaptiveFold): sample[rows][spp][3],
 *       rows = n_active, active_slot opt [rows] into the n_slots slots (NULL: slot j,
 *       n_slots >= rows); sums io [n_slots][3], mom io [n_slots][2], mean io [n_slots][3],
 *       count opt io [n_slots], keep io [rows]; init, decide, n_new, budget, rel_tol, abs_eps.
 *   "adaptive_fold_spec"  launch_adaptive_fold_spec (AdaptiveSpecFold), one window: the
 *       fields of "adaptive_fold" without init, decide and n_new, count not optional, and
 *       n, w, s0, batch_spp, min_spp, ctr io [2] (discarded, stopped).
 *   "level_finish"  launch_adaptive_level_select, then launch_adaptive_finish, over n_slots
 *       slots: count [n_slots], mom [n_slots][2], sums [n_slots][3] and the rule (budget,
 *       min_spp, rel_tol, abs_eps) in; live io [n_slots], keep io [n_slots], lvl io [4]
 *       (words: active, level, live, below; the first is left alone), mean io [n_slots][3],
 *       count_out opt io [n_slots].
 *   "compact"  launch_adaptive_compact: keep [rows], active_slot opt [rows] into n_slots,
 *       pixels opt [n_slots] with values in [0, n_image); slot_out io [rows], pixel_out io
 *       [rows], n_out io [1].
 *   "aov_fold"  launch_aov_fold (AovFold): sample[rows][spp][8] is val, sums io [rows][8] is
 *       acc; init, finish, ns, p0; albedo opt io [n_shard][3], normal opt io [n_shard][3],
 *       depth opt io [n_shard].
 *   "aov_fold_emission"  launch_aov_fold_emission (AovEmissionFold): sample[rows][spp][4] is
 *       emit, s0, sums io [rows][4] is acc, ns, p0, count opt [n_shard] (any value: the
 *       kernel clamps it into 1..ns), emission io [n_shard][3].
 *   "finish"  launch_finish: sums [rows][3] in, ns, mean io [rows][3].
 *   "scatter"  launch_scatter_pixels: sample[rows][3] is packed, index [rows] into the
 *       n_image pixels of image io [n_image][3].
 *
 * misalign (0..3; "window" and the two adaptive folds) uploads the samples that many
 * floats into a larger 16-byte-aligned allocation, which is how a test reaches the
 * wrappers' route for samples that are not 16-byte aligned.
 *
 * SRR_EINVAL, decided before the GPU is touched: an unknown kind; a NULL array that is
 * not optional; rows, spp, n_slots, n_shard or n_image not positive where the kind
 * reads them, rows or n_slots above 2^24, spp above 2^16, or more than 2^28 sample
 * floats (so no byte count overflows); misalign outside 0..3; n_slots < rows without
 * active_slot; an active_slot entry outside [0, n_slots) or repeated; a pixels entry
 * outside [0, n_image); an index entry outside [0, n_image); p0 < 0 or p0 + rows >
 * n_shard; ns < 1 where a mean is taken ("window": ns < 0); n_new < 1, budget < 1,
 * batch_spp < 1, min_spp < 0, n < 0, s0 < 0, s0 + spp > w, or n + w above 2^30; in a
 * window with s0 > 0, a count of an active slot outside [0, n + w]; for "level_finish",
 * a count outside [0, budget].  Otherwise needs a GPU. */
typedef struct srr_fold_kat {
  const float* sample;
  int32_t rows, spp, misalign;
  const int32_t* active_slot;
  int32_t n_slots;
  float* sums;
  float* mom;
  float* mean;
  int32_t* count;
  int32_t* count_out;
  uint8_t* keep;
  uint8_t* live;
  int32_t* lvl;
  uint64_t* ctr;
  int32_t init, decide, finish;
  int32_t n, w, s0, n_new;
  int32_t batch_spp, min_spp, budget, ns;
  float rel_tol, abs_eps;
  const int32_t* pixels;
  const int32_t* index;
  int32_t n_image;
  int32_t* slot_out;
  int32_t* pixel_out;
  int32_t* n_out;
  int32_t p0, n_shard;
  float* albedo;
  float* normal;
  float* depth;
  float* emission;
  float* image;
} srr_fold_kat;
int srr_device_fold_kat(const char* kind, const srr_fold_kat* a);

/* Sobol (0,2)-points of Raytracing_n.cpp:721-812, out[n][2]. */
int srr_sobol_points(int n, double* out);

/* Host-side inspection (no GPU needed) -------------------------------------
 * Teapot triangles (p0 p1 p2, 9 floats each) as srr_teapot would create them;
 * returns the triangle count (out may be NULL to query it). */
int srr_teapot_vertices(float scale, int divs, float* out);
/* Topology of the bvh_node `obj` in preorder, one line per node: "N" for an
 * interior node, "L a b" for a leaf over children a, b (indices into the
 * children array given to srr_bvh_node; a == b for a one-child leaf), after a
 * first line "box minx miny minz maxx maxy maxz".  Returns bytes needed. */
int64_t srr_bvh_topology(const srr_scene* s, int obj, char* buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SRR_CAPI_H */
