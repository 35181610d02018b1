// Launch shims of the variance-guided a-trous filter (denoise_var.hip) behind
// srr_denoise_var (capi.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "denoise.h"

namespace srr {

// One iteration of the filter over an nx x ny image: x_in -> x_out (float4 r, g, b, v
// per pixel, v the variance of the pixel's luminance), or, when out != nullptr (the
// last iteration), -> out (3 floats per pixel) and var_out (1 float, may be nullptr),
// remodulated by albedo + 1e-3f when albedo != nullptr.
struct DnvIter {
  int nx, ny, step;
  float kl, kn, kz;
  const float4* x_in;
  const float4* guide;  // normal.xyz, depth
  float4* x_out;
  float* out;
  float* var_out;
  const float* albedo;
};

// x = (colour, variance), demodulated when albedo != nullptr; g = (normal, depth)
void launch_denoise_var_pack(int64_t n, const float* color, const float* var, const float* albedo,
                             const float* normal, const float* depth, float4* x, float4* g, hipStream_t st);
// variant: a DnVariant, as launch_denoise_iter reads it
void launch_denoise_var_iter(const DnvIter& I, int variant, hipStream_t st);

}  // namespace srr
