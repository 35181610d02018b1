// srr_denoise_var: the variance-guided a-trous filter of include/srr_capi.h on gfx950
// (the edge-stopping of Schied et al. 2017, SVGF, section 4.4, on one frame).
//
// Layout: that of denoise.hip, with the variance of the pixel's luminance in the
// fourth word that k_dn_pack leaves 0: x = (r, g, b, v), g = (n.x, n.y, n.z, z).  A
// tap is the same two 16-byte loads, and the variance rides in one of them.
//
// Two variants of one iteration, split as in denoise.hip:
//   k_dnv_tile<S> (steps 1 and 2): the same (32+4S) x (8+4S) LDS tile of two float4
//     images (13.5 / 20 KiB).  The 3x3 variance prefilter reads ADJACENT pixels, and
//     the halo of 2*S >= 2 already holds them: nine more LDS reads, no global one;
//   k_dnv_gather (steps >= 4): taps and prefilter straight from global memory.
// No kernel waits on another block; the iterations are separate launches on one
// stream.  The last iteration writes the 3-float colour and, when asked, the 1-float
// variance, both remodulated.
//
// Numerics: as denoise.hip (-ffp-contract=off, rexp / rdiv bit-equal to the host's),
// the square root is rsqrt_exact, and taps are visited in the header's order, so
// both outputs equal tests/denoise_var_ref.py bit for bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "denoise_var.h"
#include "devmath.h"

#pragma clang fp contract(off)

namespace srr {
namespace dev {

constexpr int kDnvTileW = 32, kDnvTileH = 8;  // pixels per block, one per thread

struct DnvTap {  // the running sums of one pixel
  float sr, sg, sb, ws, vs;
};

SRR_D float dnv_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// one tap of the filter (include/srr_capi.h): h = B[|dx|] * B[|dy|], lp = lum(xp)
SRR_D void dnv_tap(DnvTap& a, float h, float lp, float den, float4 gp, float4 xq, float4 gq, float kn, float kz) {
  const float dl = fabsf(dnv_lum(xq.x, xq.y, xq.z) - lp);
  const float wl = rdiv(dl, den);
  const float nr = gq.x - gp.x, ng = gq.y - gp.y, nb = gq.z - gp.z;
  const float dn = (nr * nr + ng * ng) + nb * nb;
  const float zd = gp.w - gq.w;
  const float dz = rdiv(zd * zd, (gp.w * gp.w + gq.w * gq.w) + 1e-20f);
  const float w = h * rexp(-((wl + dn * kn) + dz * kz));
  a.sr += w * xq.x;
  a.sg += w * xq.y;
  a.sb += w * xq.z;
  a.ws += w;
  a.vs += (w * w) * xq.w;
}

SRR_D float dnv_b(int d) {  // B[|d|], d in -2..2
  return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f);
}

SRR_D float dnv_g(int dx, int dy) {  // G of the 3x3 prefilter: centre, edge, corner
  return (dx == 0 && dy == 0) ? 0.25f : ((dx == 0 || dy == 0) ? 0.125f : 0.0625f);
}

// the filtered pixel: to the next scratch image, or (the last iteration) to the outputs
SRR_D void dnv_store(const DnvIter& I, size_t pi, const DnvTap& a) {
  float r = rdiv(a.sr, a.ws), g = rdiv(a.sg, a.ws), b = rdiv(a.sb, a.ws);
  float v = rdiv(a.vs, a.ws * a.ws);
  if (I.out) {
    if (I.albedo) {
      const float mr = I.albedo[3 * pi] + 1e-3f, mg = I.albedo[3 * pi + 1] + 1e-3f, mb = I.albedo[3 * pi + 2] + 1e-3f;
      const float la = dnv_lum(mr, mg, mb);
      r = r * mr;
      g = g * mg;
      b = b * mb;
      v = v * (la * la);
    }
    I.out[3 * pi] = r;
    I.out[3 * pi + 1] = g;
    I.out[3 * pi + 2] = b;
    if (I.var_out) I.var_out[pi] = v;
  } else {
    I.x_out[pi] = make_float4(r, g, b, v);
  }
}

__global__ void __launch_bounds__(256) k_dnv_pack(int64_t n, const float* __restrict__ color,
                                                  const float* __restrict__ var, const float* __restrict__ albedo,
                                                  const float* __restrict__ normal, const float* __restrict__ depth,
                                                  float4* __restrict__ x, float4* __restrict__ g) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float r = color[3 * i], gg = color[3 * i + 1], b = color[3 * i + 2], v = var[i];
  if (albedo) {  // demodulate
    const float mr = albedo[3 * i] + 1e-3f, mg = albedo[3 * i + 1] + 1e-3f, mb = albedo[3 * i + 2] + 1e-3f;
    const float la = dnv_lum(mr, mg, mb);
    r = rdiv(r, mr);
    gg = rdiv(gg, mg);
    b = rdiv(b, mb);
    v = rdiv(v, la * la);
  }
  x[i] = make_float4(r, gg, b, v);
  g[i] = make_float4(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], depth[i]);
}

// Steps 1 and 2: the tile and its halo through LDS.
template <int S>
__global__ void __launch_bounds__(256) k_dnv_tile(DnvIter I) {
  constexpr int HALO = 2 * S, TW = kDnvTileW + 2 * HALO, TH = kDnvTileH + 2 * HALO;
  __shared__ float4 s_x[TH * TW];
  __shared__ float4 s_g[TH * TW];
  const int x0 = blockIdx.x * kDnvTileW - HALO, y0 = blockIdx.y * kDnvTileH - HALO;
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
  const int lx = threadIdx.x % kDnvTileW, ly = threadIdx.x / kDnvTileW;
  const int px = blockIdx.x * kDnvTileW + lx, py = blockIdx.y * kDnvTileH + ly;
  if (px >= I.nx || py >= I.ny) return;
  const int c = (ly + HALO) * TW + lx + HALO;
  const float4 xp = s_x[c], gp = s_g[c];
  float gs = 0.f, gw = 0.f;  // the prefilter: adjacent pixels, inside the halo (HALO >= 2)
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
    if (py + dy < 0 || py + dy >= I.ny) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      if (px + dx < 0 || px + dx >= I.nx) continue;
      const float G = dnv_g(dx, dy);
      gs += G * s_x[c + dy * TW + dx].w;
      gw += G;
    }
  }
  const float den = I.kl * rsqrt_exact(rdiv(gs, gw)) + 1e-6f;
  const float lp = dnv_lum(xp.x, xp.y, xp.z);
  DnvTap a{0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = py + S * dy;
    if (qy < 0 || qy >= I.ny) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = px + S * dx;
      if (qx < 0 || qx >= I.nx) continue;
      const int q = c + S * dy * TW + S * dx;
      dnv_tap(a, dnv_b(dx) * dnv_b(dy), lp, den, gp, s_x[q], s_g[q], I.kn, I.kz);
    }
  }
  dnv_store(I, (size_t)py * I.nx + px, a);
}

// Steps >= 4: the taps and the prefilter straight from global memory.
__global__ void __launch_bounds__(256) k_dnv_gather(DnvIter I) {
  const int lx = threadIdx.x % kDnvTileW, ly = threadIdx.x / kDnvTileW;
  const int px = blockIdx.x * kDnvTileW + lx, py = blockIdx.y * kDnvTileH + ly;
  if (px >= I.nx || py >= I.ny) return;
  const size_t pi = (size_t)py * I.nx + px;
  const float4 xp = I.x_in[pi], gp = I.guide[pi];
  float gs = 0.f, gw = 0.f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
    if (py + dy < 0 || py + dy >= I.ny) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      if (px + dx < 0 || px + dx >= I.nx) continue;
      const float G = dnv_g(dx, dy);
      gs += G * I.x_in[(size_t)(py + dy) * I.nx + (px + dx)].w;
      gw += G;
    }
  }
  const float den = I.kl * rsqrt_exact(rdiv(gs, gw)) + 1e-6f;
  const float lp = dnv_lum(xp.x, xp.y, xp.z);
  const int s = I.step;
  DnvTap a{0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = py + s * dy;
    if (qy < 0 || qy >= I.ny) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = px + s * dx;
      if (qx < 0 || qx >= I.nx) continue;
      const size_t qi = (size_t)qy * I.nx + qx;
      dnv_tap(a, dnv_b(dx) * dnv_b(dy), lp, den, gp, I.x_in[qi], I.guide[qi], I.kn, I.kz);
    }
  }
  dnv_store(I, pi, a);
}

}  // namespace dev

void launch_denoise_var_pack(int64_t n, const float* color, const float* var, const float* albedo,
                             const float* normal, const float* depth, float4* x, float4* g, hipStream_t st) {
  const int64_t grid = (n + 255) / 256;
  hipLaunchKernelGGL(dev::k_dnv_pack, dim3((unsigned)grid), dim3(256), 0, st, n, color, var, albedo, normal, depth, x,
                     g);
}

void launch_denoise_var_iter(const DnvIter& I, int variant, hipStream_t st) {
  const dim3 grid((I.nx + dev::kDnvTileW - 1) / dev::kDnvTileW, (I.ny + dev::kDnvTileH - 1) / dev::kDnvTileH);
  const bool tile = variant == kDnTile || (variant == kDnAuto && I.step <= 2);
  if (tile && I.step == 1) hipLaunchKernelGGL(dev::k_dnv_tile<1>, grid, dim3(256), 0, st, I);
  else if (tile && I.step == 2) hipLaunchKernelGGL(dev::k_dnv_tile<2>, grid, dim3(256), 0, st, I);
  else hipLaunchKernelGGL(dev::k_dnv_gather, grid, dim3(256), 0, st, I);
}

}  // namespace srr
