// gsr_imgloss.hip.h -- kernels of the fused image losses (gsr_imgloss).  The per-pixel arithmetic is gsr_imgloss.h's, shared
// with the host harness.  No float atomics: every sum has one order, the same input gives the same bits on every run.
//
//   k_imgloss_tile   one workgroup per IMGLOSS_TH x IMGLOSS_TW tile of one (image, channel) plane, one thread per pixel.  The
//                    tile and a 5-pixel halo of both images are staged in LDS (zeros beyond the image, the clamp applied on
//                    the way in), the row pass writes the five window sums of x, y, x^2, y^2, xy for the tile's columns and
//                    all its rows + halo into LDS, the column pass gives every pixel its five statistics.  Written: ssim_map,
//                    the three derivative maps (workspace, only when a gradient is wanted), and the tile's sums of |d|, d^2
//                    and map: lanes by a butterfly, waves in index order, one thread stores.
//   k_imgloss_sum    one workgroup per image: its tiles' partials in a fixed order (per-thread strided runs in double, an LDS
//                    tree), then the four terms.
//   k_imgloss_grad   the tile pass again over the three derivative maps (zeros beyond the image): a gather, rows then
//                    columns, then gsr_imgloss.h's grad_point.
//
// LDS: 25.4 KiB (tile pass) and 23.1 KiB (gradient pass) per 512-thread workgroup: four workgroups -- the 32 waves a CU
// holds -- take 102 of 160 KiB, so occupancy is set by registers.  A half-wave reads 32 consecutive floats of one LDS row in
// both passes: conflict-free for ds_read_b32 whatever the row stride.
#pragma once
#include <hip/hip_runtime.h>

#include "gsr_imgloss.h"

namespace gsr_il {

constexpr int TH = IMGLOSS_TH, TW = IMGLOSS_TW;
constexpr int IL_THREADS = TH * TW;                       // 512
constexpr int IL_WAVES = IL_THREADS / 64;                 // 8
constexpr int SH = TH + 2 * HALO, SW = TW + 2 * HALO;     // 26 x 42
constexpr int SUM_THREADS = 256;

struct Args {
  int32_t B, C, H, W;
  float w_l1, w_l2, w_ssim;
  uint32_t flags;
  const float* img;    // [B,C,H,W]
  const float* ref;
  float* part;         // workspace: [3][B * C * tpp] sums of |d|, d^2, map per tile
  float* dmaps;        // workspace: [3][B,C,H,W] d map / d mu1, d e11, d e12; null without a gradient
  float* terms;        // [B,4]
  float* grad;         // [B,C,H,W] or null
  float* ssim_map;     // [B,C,H,W] or null
  int32_t tiles_x, tpp;   // tiles per row and per plane
  float inv_n;            // 1 / (C H W)
};

struct TilePos {
  size_t plane_off;    // first element of the (image, channel) plane
  int y0, x0;          // the tile's first pixel
};

__device__ __forceinline__ TilePos tile_pos(const Args& ar) {
  const unsigned bx = blockIdx.x, tpp = (unsigned)ar.tpp;
  const unsigned plane = bx / tpp, t = bx - plane * tpp;
  const unsigned trow = t / (unsigned)ar.tiles_x;
  return TilePos{(size_t)plane * (size_t)ar.H * (size_t)ar.W, (int)trow * TH, (int)(t - trow * (unsigned)ar.tiles_x) * TW};
}

__device__ __forceinline__ float wave_sum(float v) {      // a butterfly: every lane ends with the same sum, one fixed order
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ void __launch_bounds__(IL_THREADS) k_imgloss_tile(Args ar) {
  __shared__ float s_x[SH][SW], s_y[SH][SW];
  __shared__ float s_row[5][SH][TW];
  __shared__ float s_red[3][IL_WAVES];
  const int tid = (int)threadIdx.x, H = ar.H, W = ar.W;
  const TilePos tp = tile_pos(ar);
  const float* px = ar.img + tp.plane_off;
  const float* py = ar.ref + tp.plane_off;
  const bool clamp = (ar.flags & FLAG_CLAMP01) != 0u;

  for (int i = tid; i < SH * SW; i += IL_THREADS) {
    const int r = i / SW, c = i - r * SW;
    const int gy = tp.y0 - HALO + r, gx = tp.x0 - HALO + c;
    float xv = 0.0f, yv = 0.0f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const size_t e = (size_t)gy * (size_t)W + (size_t)gx;
      xv = px[e];
      yv = py[e];
      if (clamp) { xv = clamp01<float>(xv); yv = clamp01<float>(yv); }
    }
    s_x[r][c] = xv;
    s_y[r][c] = yv;
  }
  __syncthreads();
  for (int i = tid; i < SH * TW; i += IL_THREADS) {
    const int r = i / TW, c = i - r * TW;
    float o[5];
    row_stats<float>(&s_x[r][c], &s_y[r][c], o);
#pragma unroll
    for (int q = 0; q < 5; ++q) s_row[q][r][c] = o[q];
  }
  __syncthreads();

  const int ly = tid / TW, lx = tid - ly * TW;
  const int gy = tp.y0 + ly, gx = tp.x0 + lx;
  float v_abs = 0.0f, v_sq = 0.0f, v_map = 0.0f;
  if (gy < H && gx < W) {
    const float mu1 = win11<float>(&s_row[0][ly][lx], TW), mu2 = win11<float>(&s_row[1][ly][lx], TW);
    const float e11 = win11<float>(&s_row[2][ly][lx], TW), e22 = win11<float>(&s_row[3][ly][lx], TW);
    const float e12 = win11<float>(&s_row[4][ly][lx], TW);
    float d_mu1, d_e11, d_e12;
    v_map = ssim_point<float>(mu1, mu2, e11, e22, e12, d_mu1, d_e11, d_e12);
    const float d = diff<float>(s_x[ly + HALO][lx + HALO], s_y[ly + HALO][lx + HALO]);
    v_abs = fabsf(d);
    v_sq = sq<float>(d);
    const size_t e = tp.plane_off + (size_t)gy * (size_t)W + (size_t)gx;
    if (ar.ssim_map) ar.ssim_map[e] = v_map;
    if (ar.dmaps) {
      const size_t n_all = (size_t)ar.B * (size_t)ar.C * (size_t)H * (size_t)W;
      ar.dmaps[e] = d_mu1;
      ar.dmaps[n_all + e] = d_e11;
      ar.dmaps[2 * n_all + e] = d_e12;
    }
  }
  v_abs = wave_sum(v_abs);
  v_sq = wave_sum(v_sq);
  v_map = wave_sum(v_map);
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) { s_red[0][wave] = v_abs; s_red[1][wave] = v_sq; s_red[2][wave] = v_map; }
  __syncthreads();
  if (tid < 3) {
    float acc = s_red[tid][0];
    for (int w = 1; w < IL_WAVES; ++w) acc += s_red[tid][w];
    ar.part[(size_t)tid * ((size_t)ar.B * (size_t)ar.C * (size_t)ar.tpp) + (size_t)blockIdx.x] = acc;
  }
}

__global__ void __launch_bounds__(SUM_THREADS) k_imgloss_sum(Args ar) {
  __shared__ double s_acc[3][SUM_THREADS];
  const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
  const size_t per_img = (size_t)ar.C * (size_t)ar.tpp, all = (size_t)ar.B * per_img;
  const float* p = ar.part + (size_t)b * per_img;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (size_t i = (size_t)tid; i < per_img; i += SUM_THREADS) {
    a0 += (double)p[i];
    a1 += (double)p[all + i];
    a2 += (double)p[2 * all + i];
  }
  s_acc[0][tid] = a0; s_acc[1][tid] = a1; s_acc[2][tid] = a2;
  __syncthreads();
  for (int half = SUM_THREADS / 2; half >= 1; half >>= 1) {
    if (tid < half) {
#pragma unroll
      for (int q = 0; q < 3; ++q) s_acc[q][tid] += s_acc[q][tid + half];
    }
    __syncthreads();
  }
  if (tid == 0) {
    float out[4];
    finish_terms(s_acc[0][0], s_acc[1][0], s_acc[2][0], (int64_t)ar.C * (int64_t)ar.H * (int64_t)ar.W, ar.w_l1, ar.w_l2, ar.w_ssim, out);
#pragma unroll
    for (int k = 0; k < 4; ++k) ar.terms[(size_t)b * 4 + (size_t)k] = out[k];
  }
}

__global__ void __launch_bounds__(IL_THREADS) k_imgloss_grad(Args ar) {
  __shared__ float s_m[3][SH][SW];
  __shared__ float s_row[3][SH][TW];
  const int tid = (int)threadIdx.x, H = ar.H, W = ar.W;
  const TilePos tp = tile_pos(ar);
  const size_t n_all = (size_t)ar.B * (size_t)ar.C * (size_t)H * (size_t)W;

  for (int i = tid; i < SH * SW; i += IL_THREADS) {
    const int r = i / SW, c = i - r * SW;
    const int gy = tp.y0 - HALO + r, gx = tp.x0 - HALO + c;
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const size_t e = tp.plane_off + (size_t)gy * (size_t)W + (size_t)gx;
      v0 = ar.dmaps[e];
      v1 = ar.dmaps[n_all + e];
      v2 = ar.dmaps[2 * n_all + e];
    }
    s_m[0][r][c] = v0;
    s_m[1][r][c] = v1;
    s_m[2][r][c] = v2;
  }
  __syncthreads();
  for (int i = tid; i < SH * TW; i += IL_THREADS) {
    const int r = i / TW, c = i - r * TW;
#pragma unroll
    for (int q = 0; q < 3; ++q) s_row[q][r][c] = win11<float>(&s_m[q][r][c], 1);
  }
  __syncthreads();

  const int ly = tid / TW, lx = tid - ly * TW;
  const int gy = tp.y0 + ly, gx = tp.x0 + lx;
  if (gy >= H || gx >= W) return;
  const float gm = win11<float>(&s_row[0][ly][lx], TW), g11 = win11<float>(&s_row[1][ly][lx], TW);
  const float g12 = win11<float>(&s_row[2][ly][lx], TW);
  const size_t e = tp.plane_off + (size_t)gy * (size_t)W + (size_t)gx;
  float xv = ar.img[e], yv = ar.ref[e], mask = 1.0f;
  if ((ar.flags & FLAG_CLAMP01) != 0u) {
    mask = clamp_mask<float>(xv);
    xv = clamp01<float>(xv);
    yv = clamp01<float>(yv);
  }
  ar.grad[e] = grad_point<float>(xv, yv, gm, g11, g12, ar.w_l1, ar.w_l2, ar.w_ssim, ar.inv_n, mask);
}

}  // namespace gsr_il
