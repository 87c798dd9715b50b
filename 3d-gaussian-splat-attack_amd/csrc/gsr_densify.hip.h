// gsr_densify.hip.h -- adaptive density control (reference scene/gaussian_model.py:591-712) as one launch chain:
//   k_densify_stats      the statistics of a batch of views, one lane per Gaussian
//   k_densify_classify   one lane per row: its class code and its three 0/1 counts (scanned by scan_exclusive_u32);
//                        k_densify_classify_mask writes the same from a byte mask (prune_points)
//   k_densify_move       every tensor, its moments, the row mask and origin / kind to their new rows in ONE launch
// The move is bandwidth-bound like the Adam step and walks like k_adam_step_multi: a by-value table of up to 8 tensors of
// <= 48 columns, a workgroup is one wave and owns DENS_SPAN consecutive floats of ONE source tensor (16-byte loads where the
// bases allow, 4-byte otherwise, a scalar tail).  Each element looks up its row's code and offsets and stores to the row's
// destinations: its kept row, its clone, or its N children.  A span whose rows yield nothing returns after reading their
// codes.  No atomics, no barriers, no LDS; every destination element is written exactly once (the destinations of distinct
// source rows are distinct rows), so the outputs need no clearing.  Unlike the Adam step the loads are not staged ahead in
// register arrays: the per-element emit is too large to unroll, and the waves of a SIMD (8) overlap each other's loads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_densify.h"   // the scalar source (shared with tests/host_math/densify_host.cpp) and the non-finite contract

namespace gsr {

// grad [B, P, 3] (x and y read), radii int32 [B, P] or null, filter uint8 [B, P] or null (null: radii > 0); the views in order
__global__ void __launch_bounds__(256) k_densify_stats(const float* __restrict__ grad, const int32_t* __restrict__ radii,
                                                       const uint8_t* __restrict__ filter, int B, unsigned P,
                                                       float* __restrict__ accum, float* __restrict__ denom,
                                                       float* __restrict__ max_radii) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P) return;
  float a = accum[i], d = denom[i];
  float mr = max_radii ? max_radii[i] : 0.f;
  bool any = false;
  for (int b = 0; b < B; ++b) {
    const size_t k = (size_t)b * P + i;
    const int32_t r = radii ? radii[k] : 0;
    const bool on = filter ? filter[k] != 0 : r > 0;
    if (!on) continue;
    any = true;
    dens_stat_update(a, d, grad[3 * k], grad[3 * k + 1]);
    if (radii) mr = dens_max_radius(mr, r);
  }
  if (!any) return;
  accum[i] = a;
  denom[i] = d;
  if (max_radii && radii) max_radii[i] = mr;
}

__global__ void __launch_bounds__(256) k_densify_classify(const float* __restrict__ accum, const float* __restrict__ denom,
                                                          const float* __restrict__ scaling, const float* __restrict__ opacity,
                                                          const float* __restrict__ max_radii, unsigned P, DensParams p,
                                                          uint8_t* __restrict__ code, uint32_t* __restrict__ f_keep,
                                                          uint32_t* __restrict__ f_clone, uint32_t* __restrict__ f_split) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P) return;
  const float g = dens_mean_grad(accum[i], denom[i]);
  const float smax = dens_max3(scaling[3 * (size_t)i], scaling[3 * (size_t)i + 1], scaling[3 * (size_t)i + 2]);
  const float radius = (p.flags & DENS_SCREEN_PRUNE) ? max_radii[i] : 0.f;
  const int c = dens_classify(g, smax, opacity[i], radius, p);
  code[i] = (uint8_t)c;
  f_keep[i] = (c & DENS_KEEP) ? 1u : 0u;
  f_clone[i] = (c & DENS_CLONE) ? 1u : 0u;
  f_split[i] = (c & DENS_KIDS) ? 1u : 0u;
}

// a plain prune: the class of a row from a byte mask (non-zero = the row goes), no clone, no split
__global__ void __launch_bounds__(256) k_densify_classify_mask(const uint8_t* __restrict__ prune_mask, unsigned P, uint8_t* __restrict__ code,
                                                               uint32_t* __restrict__ f_keep, uint32_t* __restrict__ f_clone,
                                                               uint32_t* __restrict__ f_split) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P) return;
  const bool keep = prune_mask[i] == 0;
  code[i] = keep ? (uint8_t)DENS_KEEP : (uint8_t)0;
  f_keep[i] = keep ? 1u : 0u;
  f_clone[i] = 0u;
  f_split[i] = 0u;
}

struct DensMove {
  const float* src[DENS_MAX_TENSORS];
  float* dst[DENS_MAX_TENSORS];
  const float* m_src[DENS_MAX_TENSORS];       // null: the group has no state
  const float* v_src[DENS_MAX_TENSORS];
  float* m_dst[DENS_MAX_TENSORS];
  float* v_dst[DENS_MAX_TENSORS];
  unsigned first[DENS_MAX_TENSORS + 1];       // first workgroup of tensor t; first[n] = the first row-table workgroup
  int cols[DENS_MAX_TENSORS];
  int role[DENS_MAX_TENSORS];
  unsigned P;                                 // source rows
  unsigned n_keep, n_clone, n_split;
  const uint8_t* code;
  const uint32_t* off_keep;
  const uint32_t* off_clone;
  const uint32_t* off_split;
  const float* xyz;                           // the children's inputs: the sources of the XYZ and SCALE tensors and the rotation
  const float* rot;
  const float* scale;
  const float* normals;                       // [P, N, 3] or null: keyed by seed
  uint32_t seed;
  float c;
  int N;
  const uint8_t* mask_in;                     // the optimiser's row mask [P] or null
  uint8_t* mask_out;                          // [P'] or null
  int32_t* origin;                            // [P'] or null
  int32_t* kind;
  int n;
};

__device__ __forceinline__ float dens_child_value(const DensMove& a, int role, unsigned r, int col, int j, float val) {
  if (role == DENS_COPY) return val;
  if (role == DENS_SCALE) return dens_child_scale(val, a.c);
  const float q[4] = {a.rot[4 * (size_t)r], a.rot[4 * (size_t)r + 1], a.rot[4 * (size_t)r + 2], a.rot[4 * (size_t)r + 3]};
  const float s[3] = {a.scale[3 * (size_t)r], a.scale[3 * (size_t)r + 1], a.scale[3 * (size_t)r + 2]};
  float z[3];
  if (a.normals) {
    const float* zp = a.normals + ((size_t)r * (size_t)a.N + (size_t)j) * 3;
    z[0] = zp[0]; z[1] = zp[1]; z[2] = zp[2];
  } else {
    z[0] = dens_normal(a.seed, r, j, 0); z[1] = dens_normal(a.seed, r, j, 1); z[2] = dens_normal(a.seed, r, j, 2);
  }
  return dens_child_axis(val, q, s, z, col);
}

__device__ __forceinline__ float dens_pick(const float4& v, int c) { return c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w)); }

template <bool STATE>
__device__ __forceinline__ void dens_emit(const DensMove& a, int t, int cols, int role, unsigned r, int col, float val, float mv,
                                          float vv) {
  const int code = a.code[r];
  if (code == 0) return;
  float* dst = a.dst[t];
  if (code & DENS_KEEP) {
    const size_t d = (size_t)dens_row_keep(a.off_keep[r]) * (size_t)cols + (size_t)col;
    dst[d] = val;
    if (STATE) { a.m_dst[t][d] = mv; a.v_dst[t][d] = vv; }
  }
  if (code & DENS_CLONE) {
    const size_t d = (size_t)dens_row_clone(a.off_clone[r], a.n_keep) * (size_t)cols + (size_t)col;
    dst[d] = val;
    if (STATE) { a.m_dst[t][d] = 0.f; a.v_dst[t][d] = 0.f; }
  }
  if (code & DENS_KIDS) {
    const unsigned k = a.off_split[r];
    for (int j = 0; j < a.N; ++j) {
      const size_t d = (size_t)dens_row_child(k, j, a.n_keep, a.n_clone, a.n_split) * (size_t)cols + (size_t)col;
      dst[d] = dens_child_value(a, role, r, col, j, val);
      if (STATE) { a.m_dst[t][d] = 0.f; a.v_dst[t][d] = 0.f; }
    }
  }
}

// the row table's workgroups (blocks first[n] ...): DENS_SPAN rows each; the mask, origin and kind of every row a row yields
__device__ __forceinline__ void dens_row_table(const DensMove& a, unsigned b) {
  const unsigned r0 = b * (unsigned)DENS_SPAN;
  for (unsigned r = r0 + threadIdx.x; r < a.P && r < r0 + (unsigned)DENS_SPAN; r += DENS_BLOCK) {
    const int code = a.code[r];
    if (code == 0) continue;
    auto put = [&](unsigned d, int kind, uint8_t m) {
      if (a.mask_out) a.mask_out[d] = m;
      if (a.origin) { a.origin[d] = (int32_t)r; a.kind[d] = kind; }
    };
    if (code & DENS_KEEP) put(dens_row_keep(a.off_keep[r]), DENS_KIND_KEEP, a.mask_in ? (uint8_t)(a.mask_in[r] != 0) : (uint8_t)1);
    if (code & DENS_CLONE) put(dens_row_clone(a.off_clone[r], a.n_keep), DENS_KIND_CLONE, (uint8_t)1);
    if (code & DENS_KIDS)
      for (int j = 0; j < a.N; ++j) put(dens_row_child(a.off_split[r], j, a.n_keep, a.n_clone, a.n_split), DENS_KIND_CHILD + j, (uint8_t)1);
  }
}

template <bool STATE>
__device__ __forceinline__ void dens_move_span(const DensMove& a, int t) {
  const int cols = a.cols[t];
  const int role = a.role[t];
  const unsigned long long n = (unsigned long long)a.P * (unsigned long long)cols;
  const unsigned long long e0 = (unsigned long long)(blockIdx.x - a.first[t]) * (unsigned long long)DENS_SPAN;
  const int span = (int)min((unsigned long long)DENS_SPAN, n - e0);      // 1 .. DENS_SPAN floats
  const int lane = threadIdx.x;
  // wave- (= workgroup-) uniform, before anything else: does any row of [r0, r1] yield a row?
  const unsigned r0 = (unsigned)adam_row_of(e0, cols);
  const int rem0 = (int)(e0 - (unsigned long long)r0 * (unsigned long long)cols);
  const unsigned r1 = r0 + (unsigned)((rem0 + span - 1) / cols);
  int any = 0;
  for (unsigned r = r0 + (unsigned)lane; r <= r1; r += DENS_BLOCK) any |= a.code[r];
  if (__ballot(any != 0) == 0ull) return;
  const float* x = a.src[t] + e0;
  const float* m = STATE ? a.m_src[t] + e0 : nullptr;
  const float* v = STATE ? a.v_src[t] + e0 : nullptr;
  auto scalar = [&](int o) {
    const int q = (rem0 + o) / cols;
    dens_emit<STATE>(a, t, cols, role, r0 + (unsigned)q, rem0 + o - q * cols, x[o], STATE ? m[o] : 0.f, STATE ? v[o] : 0.f);
  };
  // (e0 is a multiple of 4 floats: the span is as aligned as the tensor)
  uintptr_t bases = reinterpret_cast<uintptr_t>(a.src[t]);
  if (STATE) bases |= reinterpret_cast<uintptr_t>(a.m_src[t]) | reinterpret_cast<uintptr_t>(a.v_src[t]);
  if ((bases & 15u) != 0u) {
#pragma unroll 4
    for (int o = lane; o < span; o += DENS_BLOCK) scalar(o);
    return;
  }
  const int n4 = span >> 2;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const float4* m4 = reinterpret_cast<const float4*>(m);
  const float4* v4 = reinterpret_cast<const float4*>(v);
  // no array of staged vectors here: the emit below is too large to unroll four times, and an array indexed by a loop
  // counter would live in scratch; the waves of a SIMD overlap each other's loads instead
#pragma unroll 1
  for (int k = 0; k < DENS_VECS; ++k) {
    const int i = lane + k * DENS_BLOCK;
    if (i >= n4) break;
    const float4 xv = x4[i];
    float4 mv = make_float4(0.f, 0.f, 0.f, 0.f), vv = mv;
    if (STATE) { mv = m4[i]; vv = v4[i]; }
    int q = (rem0 + 4 * i) / cols;                 // one division per float4; the row advances as the column wraps
    int col = rem0 + 4 * i - q * cols;
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
      dens_emit<STATE>(a, t, cols, role, r0 + (unsigned)q, col, dens_pick(xv, c), dens_pick(mv, c), dens_pick(vv, c));
      if (++col == cols) { col = 0; ++q; }
    }
  }
  // the scalar tail of the tensor's last workgroup: span % 4 floats
  const int o = (n4 << 2) + lane;
  if (o < span) scalar(o);
}

__global__ void __launch_bounds__(DENS_BLOCK) k_densify_move(DensMove a) {
  if (blockIdx.x >= a.first[a.n]) { dens_row_table(a, blockIdx.x - a.first[a.n]); return; }
  const int t = dens_tensor_of_block(a.first, a.n, blockIdx.x);
  if (a.m_src[t]) dens_move_span<true>(a, t);
  else dens_move_span<false>(a, t);
}

}  // namespace gsr
