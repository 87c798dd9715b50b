// gsr_block.hip.h -- the wave and workgroup primitives the detector stages' kernels share (gsr_detloss.hip.h,
// gsr_setdet.hip.h, gsr_rcnn.hip.h).  Device only.  No float atomics anywhere: every float sum here adds the same operands
// in the same order on every run, so the kernels built on them give the same bits for the same input.
//
// Not here: wave_min_u64 (gsr_detloss.hip.h) and the butterflies of gsr_detect.hip.h and k_setdet_match, where a value and
// its index travel together under an order of their own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_detmath.h"

namespace gsr_block {

__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float o = __shfl_xor(v, m);
    v = o > v ? o : v;
  }
  return v;
}

// a + b is the same bits as b + a, so every lane ends with the same sum
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
  return v;
}

// the softmax statistics of one row of n logits, by one wave: lanes stride the row, then the butterflies.  Every lane
// returns the same maximum and the same sum of exp(x - max).
__device__ __forceinline__ void wave_softmax_stats(const float* x, int n, int lane, float& mx, float& sum) {
  GSR_FP_STRICT
  float m = -INFINITY;
  for (int k = lane; k < n; k += 64) m = x[k] > m ? x[k] : m;
  m = wave_max_f(m);
  float s = 0.0f;
  for (int k = lane; k < n; k += 64) s = s + gsr_detmath::m_exp(x[k] - m);
  mx = m;
  sum = wave_sum_f(s);
}

// inclusive scan of one int per thread over the workgroup's nt = blockDim.x threads; s_scan holds nt ints and keeps the
// scan (s_scan[nt - 1]: the total).  nt may be a constant or a run-time width; it is the same in every lane.
__device__ __forceinline__ int block_scan(int32_t* s_scan, int mine, int nt) {
  const int t = threadIdx.x;
  s_scan[t] = mine;
  __syncthreads();
  for (int s = 1; s < nt; s <<= 1) {
    const int add = t >= s ? s_scan[t - s] : 0;
    __syncthreads();
    s_scan[t] += add;
    __syncthreads();
  }
  return s_scan[t];
}

// the fixed LDS tree over K rows of THREADS = blockDim.x values, after thread t has put its values into s_red[.][t]: a
// barrier, then stride halving, t < s, row by row.  s_red[j][0] holds row j's sum when it returns (after a barrier).
// T = float or int.
template <int K, int THREADS, class T>
__device__ __forceinline__ void block_tree_sum(T (&s_red)[K][THREADS]) {
  GSR_FP_STRICT
  const int t = threadIdx.x;
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int j = 0; j < K; ++j) s_red[j][t] += s_red[j][t + s];
    __syncthreads();
  }
}

// a slab of nblocks rows of K per-block partials -> s_red[j][0], the sum of column j: lane t adds the entries
// t, t + THREADS, ... of each column in index order, then the tree.  For the one-block *_final kernels only.
template <int K, int THREADS>
__device__ __forceinline__ void slab_sum(const float* slab, unsigned nblocks, float (&s_red)[K][THREADS]) {
  GSR_FP_STRICT
  float acc[K];
  for (int j = 0; j < K; ++j) acc[j] = 0.0f;
  for (unsigned i = threadIdx.x; i < nblocks; i += THREADS)
    for (int j = 0; j < K; ++j) acc[j] += slab[(size_t)i * K + (size_t)j];
  for (int j = 0; j < K; ++j) s_red[j][threadIdx.x] = acc[j];
  block_tree_sum(s_red);
}

}  // namespace gsr_block
