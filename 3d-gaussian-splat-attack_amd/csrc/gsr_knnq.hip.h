// gsr_knnq.hip.h -- exact k-nearest-neighbour query with indices between two point sets (k <= 8) and the fused
// gather-mean over up to 8 attribute tensors, on gfx950.
//
// Counterpart of the host-side neighbour step of the reference's inpaint_setup (scene/gaussian_model.py:264-307: a
// scipy KDTree query with k = 5 and a numpy mean over the gathered rows of all seven attribute tensors).  Own algorithm,
// on the uniform grid of gsr_knn.hip.h: the REFERENCES are binned and sorted by cell with k_knn_bbox / k_knn_cells / the
// library's radix sort / k_knn_ranges exactly as gsr_knn_dist2 does, then copied once into cell-sorted order (x, y, z,
// index: 16 bytes per candidate, one load instead of the double indirection through sorted_idx).  The QUERIES get a cell
// key in the same grid and are sorted by it too, so that neighbouring lanes scan the same cells.  One lane per query
// walks cubic shells of cells (knnq_search_point, gsr_knnq.h) and keeps k sorted (d2, index) slots in registers; the
// kernel is a template on k, so the slots are never indexed dynamically.
//
// Distances are double (gsr_knnq.h says why: exactness and a decided order, not a timing -- fp64 throughput in this
// search has not been measured).  No float atomics anywhere: the only atomics are the bounding box's min and max, so the
// same bits result on every run and on any stream.  The contract, the proof of exactness and the known limit of a uniform
// grid are in gsr_knnq.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_knn.hip.h"   // k_knn_bbox, k_knn_cells, k_knn_ranges
#include "gsr_knnq.h"      // the scalar source, also built for the host

namespace gsr {

__global__ void __launch_bounds__(256) k_knnq_iota(uint32_t n, uint32_t* __restrict__ v) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = i;
}

// every slot missing: R == 0
__global__ void __launch_bounds__(256) k_knnq_fill(size_t n, int32_t* __restrict__ out_idx, float* __restrict__ out_d2) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out_idx[i] = -1;
  if (out_d2) out_d2[i] = INFINITY;
}

// the cell-sorted copy of the references
__global__ void __launch_bounds__(256) k_knnq_stage(const float* __restrict__ ref, uint32_t R,
                                                    const uint32_t* __restrict__ sorted_idx, KnnqRef* __restrict__ staged) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= R) return;
  const uint32_t o = sorted_idx[s];
  KnnqRef v;
  v.x = ref[3 * (size_t)o]; v.y = ref[3 * (size_t)o + 1]; v.z = ref[3 * (size_t)o + 2]; v.idx = (int32_t)o;
  staged[s] = v;
}

// one lane per query, in the order of the queries' cell keys in the reference grid
template <int K>
__global__ void __launch_bounds__(256) k_knnq_query(const KnnqRef* __restrict__ staged, int R, KnnGrid g,
                                                    const uint2* __restrict__ cell_range, const float* __restrict__ qry,
                                                    int Q, const uint32_t* __restrict__ q_sorted, int exclude_same,
                                                    int32_t* __restrict__ out_idx, float* __restrict__ out_d2) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= Q) return;
  const uint32_t q = q_sorted[s];
  const float px = qry[3 * (size_t)q], py = qry[3 * (size_t)q + 1], pz = qry[3 * (size_t)q + 2];
  KnnqBest<K> best;
  knnq_search_point<K>(px, py, pz, exclude_same ? (int32_t)q : -1, staged, R, g, cell_range, best);
  int32_t* oi = out_idx + (size_t)q * K;
#pragma unroll
  for (int j = 0; j < K; ++j) oi[j] = best.i[j];
  if (out_d2) {
    float* od = out_d2 + (size_t)q * K;
#pragma unroll
    for (int j = 0; j < K; ++j) od[j] = (float)best.d[j];      // the double value, rounded once
  }
}

// One instance of k_knnq_query per value of k: the slots live in registers, so k is a template argument.
template <int K>
inline void launch_knnq_query(uint32_t blocks, hipStream_t st, const KnnqRef* staged, int R, const KnnGrid& g,
                              const uint2* cell_range, const float* qry, int Q, const uint32_t* q_sorted, int exclude,
                              int32_t* out_idx, float* out_d2) {
  hipLaunchKernelGGL((k_knnq_query<K>), dim3(blocks), dim3(256), 0, st, staged, R, g, cell_range, qry, Q, q_sorted, exclude,
                     out_idx, out_d2);
}

// gsr_knn_gather_mean's tensors; first[t] = the first of tensor t's columns among the sum of all columns
struct KnnqGather {
  const float* src[KNNQ_MAX_TENSORS];
  float* dst[KNNQ_MAX_TENSORS];
  int cols[KNNQ_MAX_TENSORS];
  int first[KNNQ_MAX_TENSORS + 1];
  int total;                            // first[n]
};

// One lane per output element, lanes along the columns of one query's tensors: a neighbour's row is read contiguously
// (f_rest: 45 floats = 180 B) and the query's k indices are the same address in all of its lanes.
__global__ void __launch_bounds__(256) k_knnq_gather_mean(const int32_t* __restrict__ idx, size_t Q, int k, int R,
                                                          KnnqGather a) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= Q * (size_t)a.total) return;
  const size_t q = e / (size_t)a.total;
  const int c = (int)(e - q * (size_t)a.total);
  const float* src = nullptr;
  float* dst = nullptr;
  int cols = 0, first = 0;
#pragma unroll
  for (int t = 0; t < KNNQ_MAX_TENSORS; ++t)           // constant subscripts: the argument arrays stay in SGPRs
    if (c >= a.first[t] && c < a.first[t + 1]) { src = a.src[t]; dst = a.dst[t]; cols = a.cols[t]; first = a.first[t]; }
  if (!dst) return;
  dst[q * (size_t)cols + (size_t)(c - first)] = knnq_mean(idx + q * (size_t)k, k, R, src, cols, c - first);
}

}  // namespace gsr
