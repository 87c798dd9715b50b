// gsr_adam.hip.h -- the Adam update of up to eight raw attribute tensors [rows, <= 48 columns] of one model in ONE launch
// (gsr_adam_step_multi; reference scene/gaussian_model.py:160-214,350-367: torch.optim.Adam over seven named groups).
// The step is bandwidth-bound -- four 4-byte reads and three 4-byte writes per element, 28 B -- so it is flat over a
// tensor's elements: a workgroup is one wave and owns ADAM_SPAN consecutive floats, a lane takes ADAM_VECS float4 of
// each of the four streams (all loads issued before the first use), and nothing goes through LDS, atomics or barriers.
// A tensor whose four base pointers are not all 16-byte aligned takes 4-byte accesses; rows * cols % 4 floats at the
// end of a tensor are a scalar tail of its last workgroup.
//
// Row selection (one optional uint8 mask and one row range for all tensors of the call): a workgroup first decides from
// the range and the mask bytes of the rows its span covers whether any of them moves, and returns before it touches the
// four streams if none does; in a live workgroup the mask is looked up per element (a float4 may straddle rows), and a
// row that does not move is neither read nor written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_adam.h"   // the scalar source (shared with tests/host_math/adam_host.cpp) and the non-finite / range contract

namespace gsr {

struct AdamMulti {
  float* x[ADAM_MAX_TENSORS];
  const float* g[ADAM_MAX_TENSORS];
  float* m[ADAM_MAX_TENSORS];
  float* v[ADAM_MAX_TENSORS];
  unsigned long long rows[ADAM_MAX_TENSORS];
  unsigned first[ADAM_MAX_TENSORS + 1];       // first workgroup of tensor t; first[n] = the grid
  int cols[ADAM_MAX_TENSORS];
  float step_size[ADAM_MAX_TENSORS];
  float sqrt_bc2[ADAM_MAX_TENSORS];
  float b1[ADAM_MAX_TENSORS];
  float b2[ADAM_MAX_TENSORS];
  float eps[ADAM_MAX_TENSORS];
  const uint8_t* row_mask;                    // MASKED: null = the range alone
  unsigned long long row_begin, row_end;      // MASKED
  int n;
};

template <bool MASKED>
__global__ void __launch_bounds__(ADAM_BLOCK) k_adam_step_multi(AdamMulti a) {
  const int t = adam_tensor_of_block(a.first, a.n, blockIdx.x);
  const int cols = a.cols[t];
  const unsigned long long n = a.rows[t] * (unsigned long long)cols;
  const unsigned long long e0 = (unsigned long long)(blockIdx.x - a.first[t]) * (unsigned long long)ADAM_SPAN;
  const int span = (int)min((unsigned long long)ADAM_SPAN, n - e0);      // 1 .. ADAM_SPAN floats
  const int lane = threadIdx.x;
  unsigned long long r0 = 0;
  int rem0 = 0;
  if (MASKED) {
    // wave- (= workgroup-) uniform, before anything else: does any row of [r0, r1] move?
    r0 = adam_row_of(e0, cols);
    rem0 = (int)(e0 - r0 * (unsigned long long)cols);
    const unsigned long long r1 = r0 + (unsigned long long)((rem0 + span - 1) / cols);
    const unsigned long long lo = r0 > a.row_begin ? r0 : a.row_begin;
    const unsigned long long hi = r1 + 1 < a.row_end ? r1 + 1 : a.row_end;   // rows [lo, hi)
    if (lo >= hi) return;
    if (a.row_mask) {
      int any = 0;
      for (unsigned long long r = lo + (unsigned long long)lane; r < hi; r += ADAM_BLOCK) any |= a.row_mask[r];
      if (__ballot(any != 0) == 0ull) return;
    }
  }
  float* x = a.x[t] + e0;
  const float* g = a.g[t] + e0;
  float* m = a.m[t] + e0;
  float* v = a.v[t] + e0;
  const float ss = a.step_size[t], sb = a.sqrt_bc2[t], b1 = a.b1[t], b2 = a.b2[t], eps = a.eps[t];
  auto live = [&](int o) -> bool {            // element o of the span
    return !MASKED || adam_row_live(r0 + (unsigned long long)((rem0 + o) / cols), a.row_mask, a.row_begin, a.row_end);
  };
  auto scalar = [&](int o) {
    float xv = x[o], mv = m[o], vv = v[o];
    adam_update(xv, g[o], mv, vv, ss, sb, b1, b2, eps);
    x[o] = xv; m[o] = mv; v[o] = vv;
  };
  // (e0 is a multiple of 4 floats: the span is as aligned as the tensor)
  const bool vec = ((reinterpret_cast<uintptr_t>(a.x[t]) | reinterpret_cast<uintptr_t>(a.g[t]) | reinterpret_cast<uintptr_t>(a.m[t]) |
                     reinterpret_cast<uintptr_t>(a.v[t])) & 15u) == 0u;
  if (!vec) {
#pragma unroll 4
    for (int o = lane; o < span; o += ADAM_BLOCK)
      if (live(o)) scalar(o);
    return;
  }
  const int n4 = span >> 2;
  float4* x4 = reinterpret_cast<float4*>(x);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  float4 xv[ADAM_VECS], gv[ADAM_VECS], mv[ADAM_VECS], vv[ADAM_VECS];
  bool full[ADAM_VECS];
#pragma unroll
  for (int k = 0; k < ADAM_VECS; ++k) {
    const int i = lane + k * ADAM_BLOCK;
    full[k] = i < n4;
    if (MASKED && full[k]) {
      const bool l0 = live(4 * i), l1 = live(4 * i + 1), l2 = live(4 * i + 2), l3 = live(4 * i + 3);
      full[k] = l0 && l1 && l2 && l3;
      if (!full[k]) {                         // a float4 that straddles a live and a dead row: element by element
        if (l0) scalar(4 * i);
        if (l1) scalar(4 * i + 1);
        if (l2) scalar(4 * i + 2);
        if (l3) scalar(4 * i + 3);
      }
    }
    if (full[k]) { xv[k] = x4[i]; gv[k] = g4[i]; mv[k] = m4[i]; vv[k] = v4[i]; }
  }
#pragma unroll
  for (int k = 0; k < ADAM_VECS; ++k) {
    if (!full[k]) continue;
    const int i = lane + k * ADAM_BLOCK;
    float xs[4] = {xv[k].x, xv[k].y, xv[k].z, xv[k].w}, ms[4] = {mv[k].x, mv[k].y, mv[k].z, mv[k].w};
    float vs[4] = {vv[k].x, vv[k].y, vv[k].z, vv[k].w};
    const float gs[4] = {gv[k].x, gv[k].y, gv[k].z, gv[k].w};
#pragma unroll
    for (int c = 0; c < 4; ++c) adam_update(xs[c], gs[c], ms[c], vs[c], ss, sb, b1, b2, eps);
    x4[i] = make_float4(xs[0], xs[1], xs[2], xs[3]);
    m4[i] = make_float4(ms[0], ms[1], ms[2], ms[3]);
    v4[i] = make_float4(vs[0], vs[1], vs[2], vs[3]);
  }
  // the scalar tail of the tensor's last workgroup: span % 4 floats
  const int o = (n4 << 2) + lane;
  if (o < span && live(o)) scalar(o);
}

}  // namespace gsr
