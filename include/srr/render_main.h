/* The reference's program, main() (Raytracing_n.cpp:882-952), over srr, in C++:
 * pick a scene builder by sceneid (:893-919), build it with the reference's
 * builder signature `void f(hitable** scene, camera** cam, hitable** hlist, float
 * aspect)` against include/srr/ref_api.h, render nx x ny x ns with maxDepth on
 * the GPU(s) (the 8 render threads of :923-932 become one srr_render, over
 * --gpus N devices of the node with one RCCL gather at frame end), print the
 * elapsed milliseconds (:934-937) and write the ASCII P3 image (:848-886).
 *
 *     int main(int argc, char** argv) {
 *       static const srr::ref::scene_entry scenes[] = {{2, "ball_scenes", ball_scenes}, ...};
 *       return srr::ref::render_main(argc, argv, scenes, sizeof scenes / sizeof scenes[0]);
 *     }
 *
 * Options (defaults are the reference's globals, Raytracing_n.cpp:39-43):
 *   --sceneid N | --scene NAME   which builder (default sceneid 2)
 *   --scene-text FILE            instead of a builder: an srr scene description
 *                                (srr_scene_from_text), e.g. one of the reference's
 *                                builders written by python -m srr.ref_scenes
 *   --nx 1000 --ny 1000 --ns 50 --max-depth 50 --device 0 --out out.ppm
 *   --gpus N                     render on devices device .. device+N-1
 *                                (srr_renderer_create_multi: tiles of --tile
 *                                pixels, default 1, dealt round-robin, one RCCL
 *                                gather to the first device); bitwise the 1-GPU image
 *   --devices 0,1,2,3            the same with an explicit device list (a list of
 *                                one device still goes through the RCCL gather)
 *   --dry-run                    build the scene and print its digest
 *                                (srr_scene_digest), no GPU
 *   --adaptive REL_TOL           adaptive sampling (srr_render_adaptive, one GPU):
 *                                --ns is the per-pixel budget; a pixel stops once
 *                                the relative standard error of its mean luminance
 *                                is at most REL_TOL
 *   --batch-spp 16 --min-spp 16  its samples per pass / fewest samples per pixel
 *   --count-map FILE             its per-pixel sample counts as a PNG of grey
 *                                levels 255 * count / ns
 *   --adaptive-pass-spp N        speculative passes of up to N samples per pixel
 *                                (srr_adaptive_speculate): the same image in fewer
 *                                passes; 0 = off
 *   --adaptive-fill P            the pass size, in paths, they aim at (0: the
 *                                library's default)
 *   --denoise                    one GPU, with fixed spp or --adaptive: filter the
 *                                frame with srr_denoise (its defaults) over the
 *                                first-hit AOVs of srr_render_aov; --out is then
 *                                the tone-mapped denoised frame
 *   --denoise-var                the same with srr_denoise_var (its defaults), guided
 *                                by the variance of every pixel's mean luminance
 *                                (srr_adaptive_variance); not with --denoise.  With
 *                                --adaptive the variance is that frame's; without,
 *                                the frame is rendered by srr_render_adaptive with
 *                                rel_tol 0 and batch_spp = min_spp = ns: one pass,
 *                                bitwise the fixed-spp frame
 *   --aov-spp N                  samples of the AOVs (default min(ns, 16))
 *   --aov-out PREFIX             write PREFIX_albedo.png (255.99 * albedo, clamped),
 *                                PREFIX_normal.png (255.99 * (n / 2 + 1/2)) and
 *                                PREFIX_depth.png (grey 255 * depth / max depth)
 *   --aov-through-specular       one GPU, with --denoise, --denoise-var or --aov-out:
 *                                their AOVs are those of the first hit that is neither
 *                                metal nor dielectric (srr_render_aov_through)
 *   --denoise-emission           one GPU, with --denoise or --denoise-var: the filter
 *                                runs on the frame less its emission and adds it back
 *                                (srr_denoise_emission / srr_denoise_var_emission).  The
 *                                emission is rendered by srr_render_aov_emission in a
 *                                call of its own over the frame's samples (ns, not
 *                                --aov-spp; with --adaptive every pixel's own count),
 *                                through specular with --aov-through-specular;
 *                                --aov-out also writes PREFIX_emission.png, tone-mapped
 *                                like the frame
 * Differences, all forced by the reference: its render threads race on shared
 * state and its pixel mapping scrambles non-square frames (Q12);
 * srr renders every (pixel, sample) path with its per-path seed.  Exit codes:
 * 0, 1 on an srr error (message on stderr), 2 on bad arguments. */
#pragma once

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ref_api.h"

namespace srr {
namespace ref {

using builder_fn = void (*)(hitable** scene, camera** cam, hitable** hlist, float aspect);

struct scene_entry {
  int sceneid;
  const char* name;
  builder_fn build;
};

inline int render_main(int argc, char** argv, const scene_entry* scenes, int n_scenes) {
  int nx = 1000, ny = 1000, ns = 50, max_depth = 50, sceneid = 2, device = 0;  // Raytracing_n.cpp:39-43
  int gpus = 1, tile = 1;
  std::vector<int> devices;
  std::string name, out = "out.ppm", text_path;
  bool dry = false;
  double adaptive = -1;  // --adaptive REL_TOL (< 0: fixed spp)
  int batch_spp = 16, min_spp = 16;
  std::string count_map;
  int pass_spp = 0;         // --adaptive-pass-spp
  long long fill_paths = 0;  // --adaptive-fill
  bool denoise = false, denoise_var = false;
  int aov_spp = 0;  // 0: min(ns, 16)
  std::string aov_out;
  bool aov_through = false;  // --aov-through-specular
  bool denoise_emission = false;
  auto usage = [&]() {
    std::fprintf(stderr, "usage: %s [--sceneid N | --scene NAME] [--nx N] [--ny N] [--ns N] [--max-depth N] "
                         "[--device N] [--gpus N | --devices a,b,..] [--tile N] [--out FILE] [--dry-run] "
                         "[--adaptive REL_TOL [--batch-spp N] [--min-spp N] [--count-map FILE] "
                         "[--adaptive-pass-spp N [--adaptive-fill P]]] "
                         "[--denoise | --denoise-var] [--aov-spp N] [--aov-out PREFIX] "
                         "[--aov-through-specular] [--denoise-emission]\nscenes:",
                 argv[0]);
    for (int k = 0; k < n_scenes; ++k) std::fprintf(stderr, " %d:%s", scenes[k].sceneid, scenes[k].name);
    std::fprintf(stderr, "\n");
    return 2;
  };
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto num = [&](int& v) {
      if (i + 1 >= argc) return false;
      v = std::atoi(argv[++i]);
      return true;
    };
    bool ok = true;
    if (a == "--sceneid") ok = num(sceneid);
    else if (a == "--scene" && i + 1 < argc) name = argv[++i];
    else if (a == "--scene-text" && i + 1 < argc) text_path = argv[++i];
    else if (a == "--nx") ok = num(nx);
    else if (a == "--ny") ok = num(ny);
    else if (a == "--ns") ok = num(ns);
    else if (a == "--max-depth") ok = num(max_depth);
    else if (a == "--device") ok = num(device);
    else if (a == "--gpus") ok = num(gpus) && gpus >= 1;
    else if (a == "--tile") ok = num(tile) && tile >= 1;
    else if (a == "--devices" && i + 1 < argc) {
      std::stringstream ds(argv[++i]);
      for (std::string t; std::getline(ds, t, ',');) devices.push_back(std::atoi(t.c_str()));
      ok = !devices.empty();
    }
    else if (a == "--out" && i + 1 < argc) out = argv[++i];
    else if (a == "--dry-run") dry = true;
    else if (a == "--adaptive" && i + 1 < argc) ok = (adaptive = std::atof(argv[++i])) >= 0;
    else if (a == "--batch-spp") ok = num(batch_spp) && batch_spp >= 1;
    else if (a == "--min-spp") ok = num(min_spp) && min_spp >= 1;
    else if (a == "--count-map" && i + 1 < argc) count_map = argv[++i];
    else if (a == "--adaptive-pass-spp") ok = num(pass_spp) && pass_spp >= 0;
    else if (a == "--adaptive-fill" && i + 1 < argc) ok = (fill_paths = std::atoll(argv[++i])) >= 0;
    else if (a == "--denoise") denoise = true;
    else if (a == "--denoise-var") denoise_var = true;
    else if (a == "--aov-spp") ok = num(aov_spp) && aov_spp >= 1;
    else if (a == "--aov-out" && i + 1 < argc) aov_out = argv[++i];
    else if (a == "--aov-through-specular") aov_through = true;
    else if (a == "--denoise-emission") denoise_emission = true;
    else ok = false;
    if (!ok) return usage();
  }
  const scene_entry* e = nullptr;
  for (int k = 0; k < n_scenes; ++k)
    if (name.empty() ? scenes[k].sceneid == sceneid : name == scenes[k].name) e = &scenes[k];
  if ((!e && text_path.empty()) || nx < 1 || ny < 1 || ns < 1) return usage();
  if (adaptive < 0 && !count_map.empty()) return usage();
  if (adaptive < 0 && (pass_spp || fill_paths)) return usage();
  if (denoise && denoise_var) return usage();
  if ((denoise || denoise_var || !aov_out.empty()) && (gpus > 1 || !devices.empty())) return usage();  // one GPU
  if (aov_through && !(denoise || denoise_var || !aov_out.empty())) return usage();
  if (aov_through && (gpus > 1 || !devices.empty())) return usage();  // one GPU
  if (denoise_emission && !(denoise || denoise_var)) return usage();
  if (aov_spp == 0) aov_spp = ns < 16 ? ns : 16;
  const char* scene_name = text_path.empty() ? e->name : text_path.c_str();

  srr_scene* s = nullptr;
  if (!text_path.empty()) {
    std::ifstream f(text_path);
    std::stringstream ss;
    ss << f.rdbuf();
    if (!f || srr_scene_from_text(ss.str().c_str(), &s) < 0) {
      std::fprintf(stderr, "%s: %s\n", text_path.c_str(), f ? srr_last_error() : "cannot read");
      return 1;
    }
  } else {
    s = srr_scene_create();
    if (!s) return 1;
    hitable *world = nullptr, *hlist = nullptr;
    camera* cam = nullptr;
    try {
      scene_scope scope(s);
      e->build(&world, &cam, &hlist, float(nx) / float(ny));  // :894-919
      if (!world) throw error(SRR_EINVAL, "the builder set no world");
      capture(world, hlist);
    } catch (const error& x) {
      std::fprintf(stderr, "%s\n", x.what());
      srr_scene_destroy(s);
      return 1;
    }
  }
  if (dry) {
    uint64_t d = 0;
    if (srr_scene_digest(s, &d, nullptr) < 0) {
      std::fprintf(stderr, "%s\n", srr_last_error());
      srr_scene_destroy(s);
      return 1;
    }
    std::printf("%s %016llx\n", scene_name, (unsigned long long)d);
    srr_scene_destroy(s);
    return 0;
  }
  const bool multi = !devices.empty() || gpus > 1;  // an explicit --devices list: multi even for one device
  if (devices.empty())
    for (int k = 0; k < gpus; ++k) devices.push_back(device + k);
  srr_renderer* r = nullptr;
  const int rc0 = multi ? srr_renderer_create_multi(s, (int)devices.size(), devices.data(), &r)
                        : srr_renderer_create(s, devices[0], &r);
  if (rc0 < 0) {
    std::fprintf(stderr, "%s\n", srr_last_error());
    srr_scene_destroy(s);
    return 1;
  }
  srr_params p{};
  p.nx = nx;
  p.ny = ny;
  p.spp = ns;
  p.max_depth = max_depth;
  p.tile = tile;
  p.shard_count = 1;
  const size_t npix = (size_t)nx * ny;
  std::vector<unsigned char> rgb8(3 * npix);
  const bool want_aov = denoise || denoise_var || !aov_out.empty();
  std::vector<float> mean(want_aov ? 3 * npix : 0);
  srr_stats st{};
  const auto t0 = std::chrono::steady_clock::now();
  int rc;
  srr_adaptive_stats ast{};
  std::vector<int32_t> count;
  if (adaptive >= 0 || denoise_var) {
    // (--denoise-var without --adaptive: the fixed-spp frame as one adaptive pass, which keeps its moments)
    srr_adaptive_params ap{};
    ap.struct_size = sizeof ap;
    ap.batch_spp = adaptive >= 0 ? batch_spp : ns;
    ap.min_spp = adaptive >= 0 ? min_spp : ns;
    ap.rel_tol = adaptive >= 0 ? (float)adaptive : 0.f;
    ap.abs_eps = 1e-3f;
    ast.struct_size = sizeof ast;
    count.resize((size_t)nx * ny);
    rc = pass_spp || fill_paths ? srr_adaptive_speculate(r, pass_spp, (int64_t)fill_paths) : 0;
    if (rc == 0)
      rc = srr_render_adaptive_host(r, &p, &ap, want_aov ? mean.data() : nullptr, count.data(), rgb8.data(), &ast);
    st.world_rays = ast.world_rays;
  } else {
    rc = srr_render(r, &p, want_aov ? mean.data() : nullptr, rgb8.data(), &st);
  }
  std::vector<float> albedo, normal, depth;
  if (rc == 0 && want_aov) {
    albedo.resize(3 * npix);
    normal.resize(3 * npix);
    depth.resize(npix);
    srr_params pa = p;
    pa.spp = aov_spp;
    const int which = SRR_AOV_ALBEDO | SRR_AOV_NORMAL | SRR_AOV_DEPTH;
    rc = aov_through
             ? srr_render_aov_through_host(r, &pa, which, albedo.data(), normal.data(), depth.data(), nullptr)
             : srr_render_aov_host(r, &pa, which, albedo.data(), normal.data(), depth.data());
  }
  std::vector<float> emission;
  if (rc == 0 && denoise_emission) {  // the emission of exactly the samples the frame holds
    emission.resize(3 * npix);
    rc = srr_render_aov_emission_host(r, &p, SRR_AOV_EMISSION, aov_through ? 1 : 0, nullptr, nullptr, nullptr,
                                      emission.data(), adaptive >= 0 ? count.data() : nullptr, nullptr);
  }
  if (rc == 0 && denoise_var) {
    srr_denoise_var_params dp{};
    std::vector<float> var(npix), den(3 * npix);
    rc = srr_adaptive_variance_host(r, count.data(), var.data());
    if (rc == 0) rc = srr_denoise_var_defaults(&dp);
    if (rc == 0)
      rc = denoise_emission
               ? srr_denoise_var_emission_host(devices[0], nx, ny, &dp, mean.data(), var.data(), emission.data(),
                                               albedo.data(), normal.data(), depth.data(), den.data(), nullptr)
               : srr_denoise_var_host(devices[0], nx, ny, &dp, mean.data(), var.data(), albedo.data(), normal.data(),
                                      depth.data(), den.data(), nullptr);
    if (rc == 0) rc = srr_tonemap(den.data(), (int64_t)npix, rgb8.data());
  }
  if (rc == 0 && denoise) {
    srr_denoise_params dp{};
    std::vector<float> den(3 * npix);
    rc = srr_denoise_defaults(&dp);
    if (rc == 0)
      rc = denoise_emission
               ? srr_denoise_emission_host(devices[0], nx, ny, &dp, mean.data(), emission.data(), albedo.data(),
                                           normal.data(), depth.data(), den.data())
               : srr_denoise_host(devices[0], nx, ny, &dp, mean.data(), albedo.data(), normal.data(), depth.data(),
                                  den.data());
    if (rc == 0) rc = srr_tonemap(den.data(), (int64_t)npix, rgb8.data());
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (rc == 0) rc = srr_write_ppm(out.c_str(), nx, ny, rgb8.data());
  if (rc == 0 && !aov_out.empty()) {
    std::vector<unsigned char> img(3 * npix);
    auto byte = [](float v) {  // 255.99 * v, clamped (the tone map's conversion without its sqrt)
      const int k = (int)(255.99f * v);
      return (unsigned char)(k < 0 ? 0 : k > 255 ? 255 : k);
    };
    for (size_t i = 0; i < 3 * npix; ++i) img[i] = byte(albedo[i]);
    rc = srr_write_png((aov_out + "_albedo.png").c_str(), nx, ny, img.data());
    for (size_t i = 0; i < 3 * npix; ++i) img[i] = byte(normal[i] * 0.5f + 0.5f);
    if (rc == 0) rc = srr_write_png((aov_out + "_normal.png").c_str(), nx, ny, img.data());
    float zmax = 0.f;
    for (size_t i = 0; i < npix; ++i) zmax = depth[i] > zmax ? depth[i] : zmax;
    for (size_t i = 0; i < npix; ++i)
      img[3 * i] = img[3 * i + 1] = img[3 * i + 2] = byte(zmax > 0.f ? depth[i] / zmax : 0.f);
    if (rc == 0) rc = srr_write_png((aov_out + "_depth.png").c_str(), nx, ny, img.data());
    if (rc == 0 && denoise_emission) {
      rc = srr_tonemap(emission.data(), (int64_t)npix, img.data());
      if (rc == 0) rc = srr_write_png((aov_out + "_emission.png").c_str(), nx, ny, img.data());
    }
  }
  if (rc == 0 && !count_map.empty()) {  // grey level 255 * count / ns, rounded down
    std::vector<unsigned char> grey(3 * count.size());
    for (size_t i = 0; i < count.size(); ++i) {
      const long long g = (long long)count[i] * 255 / ns;
      grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = (unsigned char)(g < 0 ? 0 : g > 255 ? 255 : g);
    }
    rc = srr_write_png(count_map.c_str(), nx, ny, grey.data());
  }
  if (rc == 0 && adaptive >= 0) {
    srr_adaptive_spec_stats sp{};
    sp.struct_size = sizeof sp;
    rc = srr_adaptive_last_spec_stats(r, &sp);
    std::fprintf(stderr, "adaptive: %lld of %lld samples in %d passes, %lld pixels stopped early; %lld traced, "
                         "%lld discarded\n",
                 (long long)ast.paths, (long long)nx * ny * ns, (int)ast.passes, (long long)ast.pixels_retired,
                 (long long)sp.paths_traced, (long long)sp.paths_discarded);
  }
  if (rc < 0) std::fprintf(stderr, "%s\n", srr_last_error());
  else {
    std::printf("%dms\n", (int)ms);  // :934-937
    std::fprintf(stderr, "%s: %dx%dx%d, %lld world rays, %.1f Msamples/s on %d GPU(s) (%s) -> %s\n", scene_name, nx,
                 ny, ns, (long long)st.world_rays, st.world_rays / (ms * 1e3), (int)devices.size(),
                 srr_renderer_transport(r), out.c_str());
  }
  srr_renderer_destroy(r);
  srr_scene_destroy(s);
  return rc < 0 ? 1 : 0;
}

}  // namespace ref
}  // namespace srr
