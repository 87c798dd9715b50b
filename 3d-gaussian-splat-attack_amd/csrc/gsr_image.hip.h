// gsr_image.hip.h -- kernels of the image front end (gsr_image_resample, its backward, gsr_image_to_u8).
// The arithmetic is gsr_image.h's, the same source the host harness compiles: results are bit for bit the host's.
//
//   k_image_resample      one thread per destination pixel, every channel in it (indices and weights once); lanes run
//                         along the destination row, so the stores are coalesced.
//   k_image_resample_bwd  GATHER: one thread per 4 source pixels of a row, every channel in it; each source pixel sums
//                         the destination pixels that sample it in a fixed order and is written exactly once -- no
//                         atomics, no memset, the same bits on every run.  VEC: the 4 pixels are adjacent and leave as
//                         one 16-byte store per channel (W % 4 == 0 and 16-byte aligned bases); otherwise the 4 pixels
//                         are 64 apart, so that the lanes of each 4-byte store are adjacent.
//   k_image_to_u8         [B,3,H,W] float -> [B,H,W,3] uint8, 4 pixels (12 bytes, three 4-byte stores) per thread.
#pragma once
#include <hip/hip_runtime.h>

#include "gsr_image.h"

namespace gsr_image {

constexpr int IMG_BX = 64, IMG_BY = 4;     // a workgroup: 4 rows of one wave each

// workgroup number -> (column block, row block, image); the grid is flat so that no dimension meets the 65535 limit
__device__ __forceinline__ void img_block(unsigned nbx, unsigned nby, unsigned& bx, unsigned& by, unsigned& b) {
  const unsigned i = blockIdx.x;
  bx = i % nbx;
  const unsigned r = i / nbx;
  by = r % nby;
  b = r / nby;
}

__global__ void __launch_bounds__(IMG_BX * IMG_BY) k_image_resample(Spec sp, const float* __restrict__ src,
                                                                    float* __restrict__ dst, unsigned nbx, unsigned nby) {
  unsigned bx, by, b;
  img_block(nbx, nby, bx, by, b);
  const int ox = (int)(bx * IMG_BX + threadIdx.x), oy = (int)(by * IMG_BY + threadIdx.y);
  if (ox >= sp.out_w || oy >= sp.out_h) return;
  const size_t splane = (size_t)sp.H * (size_t)sp.W, oplane = (size_t)sp.out_h * (size_t)sp.out_w;
  float out[MAX_C];
  forward_pixel(sp, src + (size_t)b * (size_t)sp.C * splane, oy, ox, out);
  float* d = dst + (size_t)b * (size_t)sp.C * oplane + (size_t)oy * (size_t)sp.out_w + (size_t)ox;
#pragma unroll
  for (int c = 0; c < MAX_C; ++c)
    if (c < sp.C) d[(size_t)c * oplane] = out[c];
}

template <bool VEC>
__global__ void __launch_bounds__(IMG_BX * IMG_BY) k_image_resample_bwd(Spec sp, const float* __restrict__ src,
                                                                        const float* __restrict__ grad_dst,
                                                                        float* __restrict__ grad_src, int accumulate,
                                                                        unsigned nbx, unsigned nby) {
  unsigned bx, by, b;
  img_block(nbx, nby, bx, by, b);
  const int y = (int)(by * IMG_BY + threadIdx.y);
  if (y >= sp.H) return;
  const int xbase = (int)(bx * (IMG_BX * 4));            // a workgroup's row covers 256 source pixels
  const int x0 = VEC ? xbase + 4 * (int)threadIdx.x : xbase + (int)threadIdx.x;
  const int xstep = VEC ? 1 : IMG_BX;
  if (x0 >= sp.W) return;
  const size_t splane = (size_t)sp.H * (size_t)sp.W, oplane = (size_t)sp.out_h * (size_t)sp.out_w;
  const float* g = grad_dst + (size_t)b * (size_t)sp.C * oplane;
  const size_t row = (size_t)b * (size_t)sp.C * splane + (size_t)y * (size_t)sp.W;
  int ylo, yhi;
  axis_range(sp.sy, sp.H, sp.rh, y, ylo, yhi);
  const bool clamp = (sp.flags & CLAMP01) != 0u;
  if (VEC) {                                             // W % 4 == 0: x0 + 3 < W
    float acc[4][MAX_C];
#pragma unroll
    for (int k = 0; k < 4; ++k) backward_pixel(sp, g, y, x0 + k, ylo, yhi, acc[k]);
#pragma unroll
    for (int c = 0; c < MAX_C; ++c) {
      if (c >= sp.C) break;
      const size_t o = row + (size_t)c * splane + (size_t)x0;
      float4 old = make_float4(0.f, 0.f, 0.f, 0.f), v = old;
      if (accumulate) old = *reinterpret_cast<const float4*>(grad_src + o);
      if (clamp) v = *reinterpret_cast<const float4*>(src + o);
      float4 r;
      r.x = finish_grad(sp, c, acc[0][c], &v.x, old.x, accumulate != 0);
      r.y = finish_grad(sp, c, acc[1][c], &v.y, old.y, accumulate != 0);
      r.z = finish_grad(sp, c, acc[2][c], &v.z, old.z, accumulate != 0);
      r.w = finish_grad(sp, c, acc[3][c], &v.w, old.w, accumulate != 0);
      *reinterpret_cast<float4*>(grad_src + o) = r;
    }
  } else {
    for (int k = 0; k < 4; ++k) {
      const int x = x0 + k * xstep;
      if (x >= sp.W) break;
      float acc[MAX_C];
      backward_pixel(sp, g, y, x, ylo, yhi, acc);
#pragma unroll
      for (int c = 0; c < MAX_C; ++c) {
        if (c >= sp.C) break;
        const size_t o = row + (size_t)c * splane + (size_t)x;
        const float old = accumulate ? grad_src[o] : 0.f;
        const float v = clamp ? src[o] : 0.f;
        grad_src[o] = finish_grad(sp, c, acc[c], &v, old, accumulate != 0);
      }
    }
  }
}

__global__ void __launch_bounds__(256) k_image_to_u8(const float* __restrict__ src, size_t plane, uint8_t* __restrict__ dst,
                                                     unsigned nbx, int aligned) {
  const unsigned bx = blockIdx.x % nbx, b = blockIdx.x / nbx;
  const size_t p0 = ((size_t)bx * 256 + threadIdx.x) * 4;
  if (p0 >= plane) return;
  const float* s = src + (size_t)b * 3 * plane;
  uint8_t* d = dst + ((size_t)b * plane + p0) * 3;
  if (aligned && p0 + 4 <= plane) {                      // 12 bytes from a 4-byte boundary
    const float4 r = *reinterpret_cast<const float4*>(s + p0);
    const float4 g = *reinterpret_cast<const float4*>(s + plane + p0);
    const float4 bl = *reinterpret_cast<const float4*>(s + 2 * plane + p0);
    const uint32_t r0 = to_u8(r.x), g0 = to_u8(g.x), b0 = to_u8(bl.x), r1 = to_u8(r.y), g1 = to_u8(g.y), b1 = to_u8(bl.y);
    const uint32_t r2 = to_u8(r.z), g2 = to_u8(g.z), b2 = to_u8(bl.z), r3 = to_u8(r.w), g3 = to_u8(g.w), b3 = to_u8(bl.w);
    uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
    d4[0] = r0 | (g0 << 8) | (b0 << 16) | (r1 << 24);
    d4[1] = g1 | (b1 << 8) | (r2 << 16) | (g2 << 24);
    d4[2] = b2 | (r3 << 8) | (g3 << 16) | (b3 << 24);
  } else {
    for (size_t p = p0; p < plane && p < p0 + 4; ++p) {
      uint8_t* q = dst + ((size_t)b * plane + p) * 3;
      q[0] = to_u8(s[p]);
      q[1] = to_u8(s[plane + p]);
      q[2] = to_u8(s[2 * plane + p]);
    }
  }
}

}  // namespace gsr_image
