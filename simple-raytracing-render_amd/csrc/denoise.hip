// srr_denoise: the edge-avoiding a-trous wavelet filter of include/srr_capi.h on gfx950.
//
// Layout.  A tap needs the neighbour's colour (3 floats), normal (3) and depth (1).
// They are packed once (k_dn_pack) into two float4 images: x = (r, g, b, 0), the
// colour that the iterations ping-pong, and g = (n.x, n.y, n.z, z), the guides,
// which never change.  A tap is then two 16-byte loads, and a wave's 64 lanes (two
// rows of 32 pixels) read two contiguous 512-byte runs per load instruction.
//
// Two variants of one iteration:
//   k_dn_tile<S> (steps 1 and 2): the block's 32x8 pixels and their halo of 2*S
//     pixels are staged in LDS, (32+4S) x (8+4S) entries of 32 bytes (13.5 / 20 KiB):
//     every global word is read once per block, the 25 taps read LDS with 16-byte
//     loads at consecutive addresses (no bank conflicts: a row of lanes reads a row).
//     The halo is 41 % of the staged tile at step 1 and 60 % at step 2;
//   k_dn_gather (steps >= 4): at step 4 the halo would be 78 % of the tile and the
//     taps of one pixel land 4..16 pixels apart, so the block reads its taps straight
//     from global memory: each load instruction is still two contiguous runs, and the
//     25-fold reuse is left to the L2.
// No kernel waits on another block; the iterations are separate launches on one
// stream.  The last iteration writes the 3-float output, remodulated.
//
// Numerics: the translation unit is compiled with -ffp-contract=off (and says so
// again below), rexp / rdiv are the wrappers tests/test_device_libm.py proves
// bit-equal to the host's expf and IEEE division, and the taps are visited in the
// header's order, so the output equals tests/denoise_ref.py bit for bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "denoise.h"
#include "devmath.h"

#pragma clang fp contract(off)

namespace srr {
namespace dev {

constexpr int kDnTileW = 32, kDnTileH = 8;  // pixels per block, one per thread

struct DnTap {  // the running sums of one pixel
  float sr, sg, sb, ws;
};

// one tap of the filter (include/srr_capi.h): h = B[|dx|] * B[|dy|]
SRR_D void dn_tap(DnTap& a, float h, float4 xp, float4 gp, float4 xq, float4 gq, float kc, float kn, float kz) {
  const float cr = xq.x - xp.x, cg = xq.y - xp.y, cb = xq.z - xp.z;
  const float dc = (cr * cr + cg * cg) + cb * cb;
  const float nr = gq.x - gp.x, ng = gq.y - gp.y, nb = gq.z - gp.z;
  const float dn = (nr * nr + ng * ng) + nb * nb;
  const float zd = gp.w - gq.w;
  const float dz = rdiv(zd * zd, (gp.w * gp.w + gq.w * gq.w) + 1e-20f);
  const float w = h * rexp(-((dc * kc + dn * kn) + dz * kz));
  a.sr += w * xq.x;
  a.sg += w * xq.y;
  a.sb += w * xq.z;
  a.ws += w;
}

SRR_D float dn_b(int d) {  // B[|d|], d in -2..2
  return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}

// the filtered pixel: to the next scratch image, or (the last iteration) to the output
SRR_D void dn_store(const DnIter& I, size_t pi, const DnTap& a) {
  float r = rdiv(a.sr, a.ws), g = rdiv(a.sg, a.ws), b = rdiv(a.sb, a.ws);
  if (I.out) {
    if (I.albedo) {
      r = r * (I.albedo[3 * pi] + 1e-3f);
      g = g * (I.albedo[3 * pi + 1] + 1e-3f);
      b = b * (I.albedo[3 * pi + 2] + 1e-3f);
    }
    I.out[3 * pi] = r;
    I.out[3 * pi + 1] = g;
    I.out[3 * pi + 2] = b;
  } else {
    I.x_out[pi] = make_float4(r, g, b, 0.f);
  }
}

__global__ void __launch_bounds__(256) k_dn_pack(int64_t n, const float* __restrict__ color,
                                                 const float* __restrict__ albedo, const float* __restrict__ normal,
                                                 const float* __restrict__ depth, float4* __restrict__ x,
                                                 float4* __restrict__ g) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float r = color[3 * i], gg = color[3 * i + 1], b = color[3 * i + 2];
  if (albedo) {  // demodulate
    r = rdiv(r, albedo[3 * i] + 1e-3f);
    gg = rdiv(gg, albedo[3 * i + 1] + 1e-3f);
    b = rdiv(b, albedo[3 * i + 2] + 1e-3f);
  }
  x[i] = make_float4(r, gg, b, 0.f);
  g[i] = make_float4(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], depth[i]);
}

// Steps 1 and 2: the tile and its halo through LDS.
template <int S>
__global__ void __launch_bounds__(256) k_dn_tile(DnIter I) {
  constexpr int HALO = 2 * S, TW = kDnTileW + 2 * HALO, TH = kDnTileH + 2 * HALO;
  __shared__ float4 s_x[TH * TW];
  __shared__ float4 s_g[TH * TW];
  const int x0 = blockIdx.x * kDnTileW - HALO, y0 = blockIdx.y * kDnTileH - HALO;
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
  const int lx = threadIdx.x % kDnTileW, ly = threadIdx.x / kDnTileW;
  const int px = blockIdx.x * kDnTileW + lx, py = blockIdx.y * kDnTileH + ly;
  if (px >= I.nx || py >= I.ny) return;
  const int c = (ly + HALO) * TW + lx + HALO;
  const float4 xp = s_x[c], gp = s_g[c];
  DnTap a{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = py + S * dy;
    if (qy < 0 || qy >= I.ny) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = px + S * dx;
      if (qx < 0 || qx >= I.nx) continue;
      const int q = c + S * dy * TW + S * dx;
      dn_tap(a, dn_b(dx) * dn_b(dy), xp, gp, s_x[q], s_g[q], I.kc, I.kn, I.kz);
    }
  }
  dn_store(I, (size_t)py * I.nx + px, a);
}

// Steps >= 4: the taps straight from global memory.
__global__ void __launch_bounds__(256) k_dn_gather(DnIter I) {
  const int lx = threadIdx.x % kDnTileW, ly = threadIdx.x / kDnTileW;
  const int px = blockIdx.x * kDnTileW + lx, py = blockIdx.y * kDnTileH + ly;
  if (px >= I.nx || py >= I.ny) return;
  const size_t pi = (size_t)py * I.nx + px;
  const float4 xp = I.x_in[pi], gp = I.guide[pi];
  const int s = I.step;
  DnTap a{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = py + s * dy;
    if (qy < 0 || qy >= I.ny) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = px + s * dx;
      if (qx < 0 || qx >= I.nx) continue;
      const size_t qi = (size_t)qy * I.nx + qx;
      dn_tap(a, dn_b(dx) * dn_b(dy), xp, gp, I.x_in[qi], I.guide[qi], I.kc, I.kn, I.kz);
    }
  }
  dn_store(I, pi, a);
}

}  // namespace dev

void launch_denoise_pack(int64_t n, const float* color, const float* albedo, const float* normal, const float* depth,
                         float4* x, float4* g, hipStream_t st) {
  const int64_t grid = (n + 255) / 256;
  hipLaunchKernelGGL(dev::k_dn_pack, dim3((unsigned)grid), dim3(256), 0, st, n, color, albedo, normal, depth, x, g);
}

void launch_denoise_iter(const DnIter& I, int variant, hipStream_t st) {
  const dim3 grid((I.nx + dev::kDnTileW - 1) / dev::kDnTileW, (I.ny + dev::kDnTileH - 1) / dev::kDnTileH);
  const bool tile = variant == kDnTile || (variant == kDnAuto && I.step <= 2);
  if (tile && I.step == 1) hipLaunchKernelGGL(dev::k_dn_tile<1>, grid, dim3(256), 0, st, I);
  else if (tile && I.step == 2) hipLaunchKernelGGL(dev::k_dn_tile<2>, grid, dim3(256), 0, st, I);
  else hipLaunchKernelGGL(dev::k_dn_gather, grid, dim3(256), 0, st, I);
}

}  // namespace srr
