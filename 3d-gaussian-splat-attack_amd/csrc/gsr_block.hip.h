// gsr_block.hip.h -- the wave and workgroup primitives the detector stages' kernels share.  Device only.  No float atomics
// anywhere: every float sum here adds the same operands in the same order on every run, so the kernels built on them give
// the same bits for the same input.
//
//   wave_max_f, wave_sum_f, wave_softmax_stats   gsr_setdet, gsr_rcnn
//   block_scan                                   gsr_setdet, gsr_rcnn
//   block_tree_sum, slab_sum                     gsr_detloss, gsr_setdet, gsr_rcnn, gsr_rpnloss, gsr_objmap
//   block_select_u64                             k_det_select_sort, k_rpn_select, k_rpnloss_select
//   block_gather_sort_u64                        k_det_select_sort, k_rpn_select
//   block_sort_u64, pow2_at_least                the gather, k_rpn_order
//
// The select, the gather and the sort rest on ONE invariant, stated here and nowhere else: a workgroup's 64-bit keys are
// unique (their low word is the element's index), so exactly k of them lie at or below the k-th smallest.
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

// ---- top-k of unique 64-bit keys by one workgroup of THREADS = blockDim.x threads: select, gather, sort ----------------
// key_at(i, key) gives element i's key for i < n and returns false for an element without one.  The keys are UNIQUE and
// their low 32 bits are an index below n, so "key <= the k-th smallest" names exactly k elements, ties of the high word
// decided by the index; whatever order atomics land in, the sorted list is the same.

__device__ __forceinline__ int pow2_at_least(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// ascending bitonic sort of s[0 .. n_pow2), the workgroup striding over the n_pow2 / 2 pairs of a step; begins and ends
// with a barrier
template <int THREADS>
__device__ __forceinline__ void block_sort_u64(uint64_t* s, int n_pow2) {
  const int t = threadIdx.x, half = n_pow2 >> 1;
  __syncthreads();
  for (int k = 2; k <= n_pow2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int q = t; q < half; q += THREADS) {
        const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
        const uint64_t a = s[i], b = s[l];
        if ((a > b) == ((i & k) == 0)) { s[i] = b; s[l] = a; }
      }
      __syncthreads();
    }
  }
}

// -> thr with exactly taken = min(cap, number of keys) keys <= thr (taken == 0: thr means nothing).  have: the number
// of keys where the caller knows it (then taken >= 1 is the caller's to see to, and the known count costs no work);
// otherwise the first pass's histogram gives it.  A radix select, 8 bits a pass from bit 56 down over s_hist (256 words):
// prefix / mask grow digit by digit, an index digit that is zero for every index below n is skipped, and a pass whose
// digit group is exactly what is still wanted ends the select with the whole group in; otherwise thr is the taken-th key
// itself.  Every thread walks the histogram, so every value that steers the loop, and with it every barrier, is uniform
// across the workgroup (as n, cap and have must be).  The pass loop keeps its `done` flag: with a return inside it the
// compiler unrolls the eight passes.
template <int THREADS, class KeyAt>
__device__ __forceinline__ uint64_t block_select_u64(uint32_t* s_hist, int n, int cap, KeyAt key_at, int& taken, int have = -1) {
  const int t = threadIdx.x;
  uint64_t prefix = 0ull, mask = 0ull, thr = 0ull;
  int want = have < 0 ? 0 : have < cap ? have : cap;                        // how many of the current group are still wanted
  taken = want;
  bool done = false;
  for (int shift = 56; shift >= 0 && !done; shift -= 8) {
    if (shift < 32 && ((uint64_t)(uint32_t)(n - 1) >> shift) == 0ull) {     // every index has a zero digit here
      mask |= 0xffull << shift;
      continue;
    }
    if (t < 256) s_hist[t] = 0u;
    __syncthreads();
    for (int i = t; i < n; i += THREADS) {
      uint64_t key;
      if (key_at(i, key) && (key & mask) == prefix) atomicAdd(&s_hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (have < 0 && shift == 56) {
      unsigned total = 0u;
      for (int d = 0; d < 256; ++d) total += s_hist[d];
      taken = want = (unsigned)cap < total ? cap : (int)total;
      if (want == 0) break;
    }
    unsigned below = 0u;
    int d = 0;
    for (; d < 255; ++d) {
      const unsigned h = s_hist[d];
      if (below + h >= (unsigned)want) break;
      below += h;
    }
    want -= (int)below;
    prefix |= (uint64_t)d << shift;
    mask |= 0xffull << shift;
    if (s_hist[d] == (unsigned)want) {                                      // the whole group is in
      thr = prefix | ~mask;
      done = true;
    }
    __syncthreads();                                                        // the histogram has been read
  }
  return done ? thr : prefix;                                               // (all 64 bits fixed: the taken-th key itself)
}

// the taken keys <= thr into s_key[0 .. taken) through the slot counter *s_cnt (a key beyond taken is refused), ~0ull up
// to the next power of two (at least 2; s_key holds that many), sorted ascending -> how many arrived.  Ends with a barrier.
template <int THREADS, class KeyAt>
__device__ __forceinline__ int block_gather_sort_u64(uint64_t* s_key, uint32_t* s_cnt, int n, int taken, uint64_t thr, KeyAt key_at) {
  const int t = threadIdx.x;
  if (t == 0) *s_cnt = 0u;
  __syncthreads();
  if (taken > 0) {
    for (int i = t; i < n; i += THREADS) {
      uint64_t key;
      if (key_at(i, key) && key <= thr) {
        const uint32_t slot = atomicAdd(s_cnt, 1u);
        if (slot < (uint32_t)taken) s_key[slot] = key;
      }
    }
  }
  __syncthreads();
  const uint32_t c = *s_cnt;
  const int K = c < (uint32_t)taken ? (int)c : taken;                       // (= taken: the select names exactly that many)
  const int P = pow2_at_least(K > 1 ? K : 2);
  for (int i = K + t; i < P; i += THREADS) s_key[i] = ~0ull;
  block_sort_u64<THREADS>(s_key, P);
  return K;
}

}  // namespace gsr_block
