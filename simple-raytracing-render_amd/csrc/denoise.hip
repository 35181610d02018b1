// srr_denoise and srr_denoise_var: the edge-avoiding a-trous wavelet filters of
// include/srr_capi.h on gfx950, one kernel family with two edge-stopping policies.
//
// Layout.  A tap needs the neighbour's colour (3 floats), normal (3) and depth (1).
// They are packed once (k_atrous_pack) into two float4 images: x = (r, g, b, fourth),
// the colour that the iterations ping-pong, and g = (n.x, n.y, n.z, z), the guides,
// which never change.  A tap is then two 16-byte loads, and a wave's 64 lanes (two
// rows of 32 pixels) read two contiguous 512-byte runs per load instruction.
//
// Two variants of one iteration, the same atrous_pixel over two tap sources:
//   k_atrous_tile<P, S> (steps 1 and 2): the block's 32x8 pixels and their halo of 2*S
//     pixels are staged in LDS, (32+4S) x (8+4S) entries of 32 bytes (13.5 / 20 KiB):
//     every global word is read once per block, the 25 taps read LDS with 16-byte
//     loads at consecutive addresses (no bank conflicts: a row of lanes reads a row).
//     The halo is 41 % of the staged tile at step 1 and 60 % at step 2;
//   k_atrous_gather<P> (steps >= 4): at step 4 the halo would be 78 % of the tile and
//     the taps of one pixel land 4..16 pixels apart, so the block reads its taps
//     straight from global memory: each load instruction is still two contiguous runs,
//     and the 25-fold reuse is left to the L2.
// No kernel waits on another block; the iterations are separate launches on one
// stream.  The last iteration writes the 3-float output, remodulated.
// Emission-separated filtering (srr_denoise_emission, srr_denoise_var_emission): pack
// subtracts the emission image from the colour and the last store adds it back; the
// iterations are the same kernels on the same words.
//
// The policies.  ColourStop (srr_denoise) weighs a tap by its squared colour
// difference and leaves x's fourth word 0.  VarianceStop (srr_denoise_var; the
// edge-stopping of Schied et al. 2017, SVGF, section 4.4, on one frame) keeps the
// variance of the pixel's luminance in that word, so it rides in a load the tap
// makes anyway, weighs a tap by its luminance difference over the standard deviation
// that a 3x3 prefilter of the variance gives, and filters the variance with the
// squared weights.  The prefilter reads ADJACENT pixels through the same tap source:
// the tile's halo of 2*S >= 2 already holds them, nine more LDS reads and no global
// one.  Its last iteration also writes the 1-float variance, when asked.
//
// Numerics: the translation unit is compiled with -ffp-contract=off (and says so
// again below), rexp / rdiv are the wrappers tests/test_device_libm.py proves
// bit-equal to the host's expf and IEEE division, the square root is rsqrt_exact,
// and the taps are visited in the header's order, so the outputs equal
// tests/denoise_ref.py and tests/denoise_var_ref.py bit for bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "denoise.h"
#include "devmath.h"

#pragma clang fp contract(off)

namespace srr {
namespace dev {

constexpr int kTileW = 32, kTileH = 8;  // pixels per block, one per thread

struct RgbSums {  // the running sums of one pixel that both policies keep
  float sr, sg, sb, ws;
};

SRR_D float atrous_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// the weight of one tap (include/srr_capi.h): h = B[|dx|] * B[|dy|], wc the policy's
// colour term; added to the sums that both policies keep
SRR_D float atrous_weigh(RgbSums& a, float h, float wc, float4 gp, float4 xq, float4 gq, const AtrousIter& I) {
  const float nr = gq.x - gp.x, ng = gq.y - gp.y, nb = gq.z - gp.z;
  const float dn = (nr * nr + ng * ng) + nb * nb;
  const float zd = gp.w - gq.w;
  const float dz = rdiv(zd * zd, (gp.w * gp.w + gq.w * gq.w) + 1e-20f);
  const float w = h * rexp(-((wc + dn * I.kn) + dz * I.kz));
  a.sr += w * xq.x;
  a.sg += w * xq.y;
  a.sb += w * xq.z;
  a.ws += w;
  return w;
}

// A policy is constructed per pixel from the centre (px, py), its colour xp and the
// tap source; tap() adds one neighbour to the sums, finish() makes the filtered x of
// them, and in4 / demod4 / remod4 / out4 are what pack and the last store do with
// the fourth word (m = albedo + 1e-3f).
struct ColourStop {
  using Sums = RgbSums;
  template <class Src>
  SRR_D ColourStop(const AtrousIter&, int, int, float4, const Src&) {}
  SRR_D void tap(Sums& a, float h, float4 xp, float4 gp, float4 xq, float4 gq, const AtrousIter& I) const {
    const float cr = xq.x - xp.x, cg = xq.y - xp.y, cb = xq.z - xp.z;
    const float dc = (cr * cr + cg * cg) + cb * cb;
    atrous_weigh(a, h, dc * I.k, gp, xq, gq, I);
  }
  static SRR_D float4 finish(const Sums& a) {
    return make_float4(rdiv(a.sr, a.ws), rdiv(a.sg, a.ws), rdiv(a.sb, a.ws), 0.f);
  }
  static SRR_D float in4(const float*, int64_t) { return 0.f; }
  static SRR_D float demod4(float v, float, float, float) { return v; }
  static SRR_D float remod4(float v, float, float, float) { return v; }
  static SRR_D void out4(const AtrousIter&, size_t, float) {}
};

struct VarianceStop {
  struct Sums : RgbSums {
    float vs;
  };
  float den, lp;  // k_l * (the prefiltered standard deviation) + 1e-6f, lum(xp)
  template <class Src>
  SRR_D VarianceStop(const AtrousIter& I, int px, int py, float4 xp, const Src& src) {
    float gs = 0.f, gw = 0.f;  // the 3x3 prefilter: centre 1/4, edges 1/8, corners 1/16
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
      if (py + dy < 0 || py + dy >= I.ny) continue;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if (px + dx < 0 || px + dx >= I.nx) continue;
        const float G = (dx == 0 && dy == 0) ? 0.25f : ((dx == 0 || dy == 0) ? 0.125f : 0.0625f);
        gs += G * src.at(dx, dy).x.w;
        gw += G;
      }
    }
    den = I.k * rsqrt_exact(rdiv(gs, gw)) + 1e-6f;
    lp = atrous_lum(xp.x, xp.y, xp.z);
  }
  SRR_D void tap(Sums& a, float h, float4, float4 gp, float4 xq, float4 gq, const AtrousIter& I) const {
    const float dl = fabsf(atrous_lum(xq.x, xq.y, xq.z) - lp);
    const float w = atrous_weigh(a, h, rdiv(dl, den), gp, xq, gq, I);
    a.vs += (w * w) * xq.w;
  }
  static SRR_D float4 finish(const Sums& a) {
    return make_float4(rdiv(a.sr, a.ws), rdiv(a.sg, a.ws), rdiv(a.sb, a.ws), rdiv(a.vs, a.ws * a.ws));
  }
  static SRR_D float in4(const float* var, int64_t i) { return var[i]; }
  static SRR_D float demod4(float v, float mr, float mg, float mb) {
    const float la = atrous_lum(mr, mg, mb);
    return rdiv(v, la * la);
  }
  static SRR_D float remod4(float v, float mr, float mg, float mb) {
    const float la = atrous_lum(mr, mg, mb);
    return v * (la * la);
  }
  static SRR_D void out4(const AtrousIter& I, size_t pi, float v) {
    if (I.var_out) I.var_out[pi] = v;
  }
};

// Where a neighbour's x and g come from, (ox, oy) pixels from the centre: the staged
// tile (c the centre's entry, TW entries per row) or the images themselves.
struct Tap {
  float4 x, g;
};

template <int TW>
struct TileTaps {
  const float4 *sx, *sg;
  int c;
  SRR_D Tap at(int ox, int oy) const { return {sx[c + oy * TW + ox], sg[c + oy * TW + ox]}; }
};

struct GlobalTaps {
  const AtrousIter& I;
  int px, py;
  SRR_D Tap at(int ox, int oy) const {  // (a pixel inside the image, and nx * ny <= 2^28: 32 bits hold its index)
    const unsigned qi = (unsigned)(py + oy) * (unsigned)I.nx + (unsigned)(px + ox);
    return {I.x_in[qi], I.guide[qi]};
  }
};

SRR_D float atrous_b(int d) {  // B[|d|], d in -2..2
  return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}

// The filtered pixel (px, py): its 25 taps at spacing s, those outside the image
// skipped, to the next scratch image, or (the last iteration) to the outputs.
template <class P, class Src>
SRR_D void atrous_pixel(const AtrousIter& I, int px, int py, int s, const Src& src) {
  const Tap p0 = src.at(0, 0);
  const float4 xp = p0.x, gp = p0.g;
  const P p(I, px, py, xp, src);
  typename P::Sums a{};
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = py + s * dy;
    if (qy < 0 || qy >= I.ny) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = px + s * dx;
      if (qx < 0 || qx >= I.nx) continue;
      const Tap q = src.at(s * dx, s * dy);
      p.tap(a, atrous_b(dx) * atrous_b(dy), xp, gp, q.x, q.g, I);
    }
  }
  float4 v = P::finish(a);
  const size_t pi = (size_t)py * I.nx + px;
  if (I.out) {
    if (I.albedo) {
      const float mr = I.albedo[3 * pi] + 1e-3f, mg = I.albedo[3 * pi + 1] + 1e-3f, mb = I.albedo[3 * pi + 2] + 1e-3f;
      v = make_float4(v.x * mr, v.y * mg, v.z * mb, P::remod4(v.w, mr, mg, mb));
    }
    if (I.emission) {  // emission-separated: what pack took out goes back in, one more rounding
      v.x = v.x + I.emission[3 * pi];
      v.y = v.y + I.emission[3 * pi + 1];
      v.z = v.z + I.emission[3 * pi + 2];
    }
    I.out[3 * pi] = v.x;
    I.out[3 * pi + 1] = v.y;
    I.out[3 * pi + 2] = v.z;
    P::out4(I, pi, v.w);
  } else {
    I.x_out[pi] = v;
  }
}

template <class P>
__global__ void __launch_bounds__(256) k_atrous_pack(int64_t n, const float* __restrict__ color,
                                                     const float* __restrict__ var, const float* __restrict__ emission,
                                                     const float* __restrict__ albedo,
                                                     const float* __restrict__ normal, const float* __restrict__ depth,
                                                     float4* __restrict__ x, float4* __restrict__ g) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float4 v = make_float4(color[3 * i], color[3 * i + 1], color[3 * i + 2], P::in4(var, i));
  if (emission) {  // emission-separated (srr_denoise_emission): c - e takes the place of c
    v.x = v.x - emission[3 * i];
    v.y = v.y - emission[3 * i + 1];
    v.z = v.z - emission[3 * i + 2];
  }
  if (albedo) {  // demodulate
    const float mr = albedo[3 * i] + 1e-3f, mg = albedo[3 * i + 1] + 1e-3f, mb = albedo[3 * i + 2] + 1e-3f;
    v = make_float4(rdiv(v.x, mr), rdiv(v.y, mg), rdiv(v.z, mb), P::demod4(v.w, mr, mg, mb));
  }
  x[i] = v;
  g[i] = make_float4(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], depth[i]);
}

// Steps 1 and 2: the tile and its halo through LDS.
template <class P, int S>
__global__ void __launch_bounds__(256) k_atrous_tile(AtrousIter I) {
  constexpr int HALO = 2 * S, TW = kTileW + 2 * HALO, TH = kTileH + 2 * HALO;
  __shared__ float4 s_x[TH * TW];
  __shared__ float4 s_g[TH * TW];
  const int x0 = blockIdx.x * kTileW - HALO, y0 = blockIdx.y * kTileH - HALO;
  for (int e = threadIdx.x; e < TH * TW; e += 256) {
    const int ty = e / TW, tx = e - ty * TW;
    const int gx = x0 + tx, gy = y0 + ty;
    float4 vx = make_float4(0.f, 0.f, 0.f, 0.f), vg = vx;  // outside the image: never read as a tap
    if (gx >= 0 && gx < I.nx && gy >= 0 && gy < I.ny) {
      const size_t qi = (size_t)gy * I.nx + gx;
      vx = I.x_in[qi];
      vg = I.guide[qi];
    }
    s_x[e] = vx;
    s_g[e] = vg;
  }
  __syncthreads();
  const int lx = threadIdx.x % kTileW, ly = threadIdx.x / kTileW;
  const int px = blockIdx.x * kTileW + lx, py = blockIdx.y * kTileH + ly;
  if (px >= I.nx || py >= I.ny) return;
  atrous_pixel<P>(I, px, py, S, TileTaps<TW>{s_x, s_g, (ly + HALO) * TW + lx + HALO});
}

// Steps >= 4: the taps straight from global memory.
template <class P>
__global__ void __launch_bounds__(256) k_atrous_gather(AtrousIter I) {
  const int lx = threadIdx.x % kTileW, ly = threadIdx.x / kTileW;
  const int px = blockIdx.x * kTileW + lx, py = blockIdx.y * kTileH + ly;
  if (px >= I.nx || py >= I.ny) return;
  atrous_pixel<P>(I, px, py, I.step, GlobalTaps{I, px, py});
}

template <class P>
void launch_iter(const AtrousIter& I, int variant, hipStream_t st) {
  const dim3 grid((I.nx + kTileW - 1) / kTileW, (I.ny + kTileH - 1) / kTileH);
  const bool tile = variant == kDnTile || (variant == kDnAuto && I.step <= 2);
  if (tile && I.step == 1) hipLaunchKernelGGL((k_atrous_tile<P, 1>), grid, dim3(256), 0, st, I);
  else if (tile && I.step == 2) hipLaunchKernelGGL((k_atrous_tile<P, 2>), grid, dim3(256), 0, st, I);
  else hipLaunchKernelGGL(k_atrous_gather<P>, grid, dim3(256), 0, st, I);
}

}  // namespace dev

void launch_atrous_pack(AtrousStop stop, int64_t n, const float* color, const float* var, const float* emission,
                        const float* albedo, const float* normal, const float* depth, float4* x, float4* g,
                        hipStream_t st) {
  const auto k = stop == kVarianceStop ? dev::k_atrous_pack<dev::VarianceStop> : dev::k_atrous_pack<dev::ColourStop>;
  hipLaunchKernelGGL(k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, color, var, emission, albedo, normal,
                     depth, x, g);
}

void launch_atrous_iter(AtrousStop stop, const AtrousIter& I, int variant, hipStream_t st) {
  if (stop == kVarianceStop) dev::launch_iter<dev::VarianceStop>(I, variant, st);
  else dev::launch_iter<dev::ColourStop>(I, variant, st);
}

}  // namespace srr
