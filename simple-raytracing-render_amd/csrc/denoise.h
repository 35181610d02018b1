// Launch shims of the a-trous denoiser (denoise.hip) behind srr_denoise (capi.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace srr {

// One iteration of the filter over an nx x ny image: x_in -> x_out (float4 r, g, b, 0
// per pixel), or, when out != nullptr (the last iteration), -> out (3 floats per
// pixel), multiplied by albedo + 1e-3f when albedo != nullptr (remodulation).
struct DnIter {
  int nx, ny, step;
  float kc, kn, kz;     // kc already scaled by 4^k
  const float4* x_in;
  const float4* guide;  // normal.xyz, depth
  float4* x_out;
  float* out;
  const float* albedo;
};

enum DnVariant : int { kDnAuto = 0, kDnTile = 1, kDnGather = 2 };

// x = colour (divided by albedo + 1e-3f when albedo != nullptr), g = (normal, depth)
void launch_denoise_pack(int64_t n, const float* color, const float* albedo, const float* normal, const float* depth,
                         float4* x, float4* g, hipStream_t st);
// variant: kDnAuto = the LDS tile for steps 1 and 2, the direct gather above;
// kDnTile / kDnGather force one (the tile exists for steps 1 and 2 only)
void launch_denoise_iter(const DnIter& I, int variant, hipStream_t st);

}  // namespace srr
