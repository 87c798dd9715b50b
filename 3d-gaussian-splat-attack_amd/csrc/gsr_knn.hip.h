// gsr_knn.hip.h -- mean squared distance of every point to its 3 nearest neighbours, exact, on gfx950.
//
// Replaces the reference's second native import, `simple_knn._C.distCUDA2` (reference scene/gaussian_model.py:17,
// used at :144 in create_from_pcd to seed the initial scales).  Own algorithm: points are binned into a uniform
// grid (about 3 points per cell), sorted by cell with the library's radix sort, and every point scans cubic shells
// of cells around its own until the third-best distance found so far is no larger than the distance to anything
// outside the scanned block -- which makes the result exact.  A point that has not terminated after MAX_SHELL
// shells (an isolated outlier) finishes with a brute-force sweep.  The scalar side -- grid, cell, search of one point, the
// contract for fewer than 4 points and non-finite points, and the known limit of a uniform grid -- is gsr_knn.h.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "gsr_knn.h"   // KnnGrid, knn_cell_key, knn_search_point: the scalar source, also built for the host

namespace gsr {

__device__ __forceinline__ float atomic_min_f(float* addr, float v) {
  // monotone int mapping of IEEE floats
  int* ia = reinterpret_cast<int*>(addr);
  int old = *ia, assumed;
  do {
    assumed = old;
    if (__int_as_float(assumed) <= v) break;
    old = atomicCAS(ia, assumed, __float_as_int(v));
  } while (assumed != old);
  return __int_as_float(old);
}
__device__ __forceinline__ float atomic_max_f(float* addr, float v) {
  int* ia = reinterpret_cast<int*>(addr);
  int old = *ia, assumed;
  do {
    assumed = old;
    if (__int_as_float(assumed) >= v) break;
    old = atomicCAS(ia, assumed, __float_as_int(v));
  } while (assumed != old);
  return __int_as_float(old);
}

// bbox[0..2] = min, bbox[3..5] = max (initialised to +/-FLT_MAX by the host)
__global__ void __launch_bounds__(256) k_knn_bbox(const float* __restrict__ pts, int P, float* __restrict__ bbox) {
  __shared__ float smin[3][4], smax[3][4];
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < P; i += gridDim.x * blockDim.x) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { const float v = pts[3 * i + a]; mn[a] = fminf(mn[a], v); mx[a] = fmaxf(mx[a], v); }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], d, 64));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], d, 64));
    }
    if (lane == 0) { smin[a][w] = mn[a]; smax[a][w] = mx[a]; }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    atomic_min_f(&bbox[a], fminf(fminf(smin[a][0], smin[a][1]), fminf(smin[a][2], smin[a][3])));
    atomic_max_f(&bbox[3 + a], fmaxf(fmaxf(smax[a][0], smax[a][1]), fmaxf(smax[a][2], smax[a][3])));
  }
}

__global__ void __launch_bounds__(256) k_knn_cells(const float* __restrict__ pts, int P, KnnGrid g,
                                                   uint32_t* __restrict__ keys) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  keys[i] = knn_cell_key(pts, i, g);
}

// ranges of equal keys in the sorted key array -> cell_range[cell] = (start, end)
__global__ void __launch_bounds__(256) k_knn_ranges(uint32_t P, const uint32_t* __restrict__ keys,
                                                    uint2* __restrict__ cell_range) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const uint32_t c = keys[i];
  if (i == 0 || keys[i - 1] != c) cell_range[c].x = i;
  if (i == P - 1 || keys[i + 1] != c) cell_range[c].y = i + 1;
}

// one thread per point, in cell-sorted order (neighbouring threads scan the same cells)
__global__ void __launch_bounds__(256) k_knn_search(const float* __restrict__ pts, int P, KnnGrid g,
                                                    const uint32_t* __restrict__ sorted_idx,
                                                    const uint2* __restrict__ cell_range, float* __restrict__ out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= P) return;
  knn_search_point(s, pts, P, g, sorted_idx, cell_range, out);
}

}  // namespace gsr
