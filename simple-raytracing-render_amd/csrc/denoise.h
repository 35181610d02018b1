// Launch shims of the a-trous filters (denoise.hip) behind srr_denoise and
// srr_denoise_var (capi.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace srr {

// the edge-stopping function of the weight's colour term, and the fourth word of x:
// kColourStop: srr_denoise, |colour difference|^2 * k, x = (r, g, b, 0);
// kVarianceStop: srr_denoise_var, |luminance difference| / (k * sqrt(prefiltered
// variance) + 1e-6f), x = (r, g, b, v), v the variance of the pixel's luminance
enum AtrousStop : int { kColourStop = 0, kVarianceStop = 1 };

// One iteration of a filter over an nx x ny image: x_in -> x_out (one float4 per
// pixel), or, when out != nullptr (the last iteration), -> out (3 floats per pixel)
// and var_out (1 float; kVarianceStop only, may be nullptr), remodulated by
// albedo + 1e-3f when albedo != nullptr, then plus emission when emission != nullptr
// (3 floats per pixel; the last iteration only).
struct AtrousIter {
  int nx, ny, step;
  float k, kn, kz;      // k: k_c * 4^iteration (kColourStop), k_l (kVarianceStop)
  const float4* x_in;
  const float4* guide;  // normal.xyz, depth
  float4* x_out;
  float* out;
  float* var_out;
  const float* albedo;
  const float* emission;
};

enum DnVariant : int { kDnAuto = 0, kDnTile = 1, kDnGather = 2 };

// x = (colour, 0 or var[i]), the colour less emission when emission != nullptr, then
// demodulated when albedo != nullptr; g = (normal, depth).  var is read by kVarianceStop only.
void launch_atrous_pack(AtrousStop stop, int64_t n, const float* color, const float* var, const float* emission,
                        const float* albedo, const float* normal, const float* depth, float4* x, float4* g,
                        hipStream_t st);
// variant: kDnAuto = the LDS tile for steps 1 and 2, the direct gather above;
// kDnTile / kDnGather force one (the tile exists for steps 1 and 2 only)
void launch_atrous_iter(AtrousStop stop, const AtrousIter& I, int variant, hipStream_t st);

}  // namespace srr
