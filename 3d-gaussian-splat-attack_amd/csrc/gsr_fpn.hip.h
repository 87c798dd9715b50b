// gsr_fpn.hip.h -- kernels of the FPN RoI pooler (gsr_fpn_pool, gsr_fpn_pool_backward).  The level arithmetic is
// gsr_fpn.h's, the pooling arithmetic gsr_rcnn.hip.h's device functions: a RoI pooled from level l gives the bits
// gsr_roi_align gives on that map, and a level's gradient the bits of gsr_roi_align_backward over that level's RoIs.  No
// float atomics: the same input gives the same bits on every run.
//
//   k_fpn_assign     one workgroup per image, one lane per RoI: its level, then for every level the rank of the lane among
//                    the level's RoIs (a wave ballot, the waves' totals scanned through LDS) places its index in the
//                    level's list: ascending.  roi_level [B,S], level_list [B,nl,S], level_count [B,nl].
//   k_fpn_pool       k_roi_align's grid: one lane per output element, a workgroup within one RoI; the RoI's level -- the
//                    same in all lanes -- picks the map.  Zeros for level -1.
//   k_fpn_pool_bwd   one launch for all levels: blockIdx.x runs over the 8 x 8 tiles of level 0, then level 1, ... (the level
//                    from a prefix table in the arguments), blockIdx.y the 32-channel chunk, blockIdx.z the image.  The
//                    workgroup walks its level's list alone, with k_roi_align_bwd's step.  The count is clamped to 0..S and
//                    an entry outside 0..S-1 is skipped: neither is trusted for an address.
#pragma once
#include <hip/hip_runtime.h>

#include "gsr_fpn.h"
#include "gsr_rcnn.hip.h"

namespace gsr_fpn {

using gsr_rcnn::RA_THREADS;
using gsr_rcnn::RB_CHUNK;
using gsr_rcnn::RB_PER;
using gsr_rcnn::RB_THREADS;
using gsr_rcnn::RB_TILE;
using gsr_rcnn::RoiBwdLds;
using gsr_rcnn::RoiMap;

constexpr int ASSIGN_WAVES = MAX_SAMPLE / 64;           // 16

struct PoolArgs {
  Spec sp;
  const float* features[MAX_LEVELS];   // forward: level l is [B, Cf, Hf[l], Wf[l]]
  const float* rois;                   // [B, S, 4]
  const int32_t* n_roi;                // element b * n_roi_stride, or NULL: S
  int32_t n_roi_stride;
  float* pooled;                       // forward: [B, S, Cf, PH, PW]
  int32_t* roi_level;                  // [B, S]
  int32_t* level_list;                 // [B, nl, S]
  int32_t* level_count;                // [B, nl]
  const float* grad_pooled;            // backward
  float* grad_features[MAX_LEVELS];    // backward
  int32_t accumulate;
  uint32_t tile_start[MAX_LEVELS + 1]; // backward: the first tile of level l; entries from nl on hold the total
};

// element l of a by-value table, l the same in all lanes: selects, so that the table stays in the argument registers
template <class T, int N>
__device__ __forceinline__ T pick(const T (&a)[N], int l) {
  T v = a[0];
#pragma unroll
  for (int k = 1; k < N; ++k) v = l == k ? a[k] : v;
  return v;
}

__device__ __forceinline__ RoiMap level_map(const Spec& sp, int l) {
  return RoiMap{sp.Cf, pick(sp.Hf, l), pick(sp.Wf, l), sp.PH, sp.PW, sp.sampling_ratio, pick(sp.scale, l)};
}

__global__ void __launch_bounds__(MAX_SAMPLE) k_fpn_assign(PoolArgs ar) {
  __shared__ int s_tot[MAX_LEVELS][ASSIGN_WAVES];
  const Spec& sp = ar.sp;
  const int b = blockIdx.x, s = threadIdx.x, lane = s & 63, wave = s >> 6;
  const int S = sp.S, nl = sp.nl;
  int n = ar.n_roi ? ar.n_roi[(size_t)b * (size_t)ar.n_roi_stride] : S;
  n = n < 0 ? 0 : (n > S ? S : n);
  int level = -1;
  if (s < S) {
    float r[4];
    for (int k = 0; k < 4; ++k) r[k] = ar.rois[((size_t)b * (size_t)S + (size_t)s) * 4 + (size_t)k];
    level = roi_level<float>(r, s, n, sp.thr, nl, sp.canonical_size);
    ar.roi_level[(size_t)b * (size_t)S + (size_t)s] = level;
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  int before[MAX_LEVELS];                                                 // the RoIs of level l in this wave's lower lanes
#pragma unroll
  for (int l = 0; l < MAX_LEVELS; ++l) {
    const unsigned long long m = __ballot(level == l);
    before[l] = __popcll(m & below);
    if (lane == 0) s_tot[l][wave] = __popcll(m);
  }
  __syncthreads();
  const int waves = ((int)blockDim.x + 63) >> 6;
#pragma unroll
  for (int l = 0; l < MAX_LEVELS; ++l) {
    if (l >= nl) break;
    int base = 0, total = 0;
    for (int w = 0; w < waves; ++w) {
      const int c = s_tot[l][w];
      base += w < wave ? c : 0;
      total += c;
    }
    const size_t row = (size_t)b * (size_t)nl + (size_t)l;
    if (level == l) ar.level_list[row * (size_t)S + (size_t)(base + before[l])] = s;     // base + before[l] < total <= S
    if (s == 0) ar.level_count[row] = total;
  }
}

__global__ void __launch_bounds__(RA_THREADS) k_fpn_pool(PoolArgs ar) {
  const Spec& sp = ar.sp;
  const unsigned bs = blockIdx.x;                                         // (image, RoI): the same in all lanes
  const unsigned bins = (unsigned)(sp.PH * sp.PW), per_roi = (unsigned)sp.Cf * bins;
  const unsigned i = blockIdx.y * RA_THREADS + threadIdx.x;               // (channel, ph, pw) of that RoI
  if (i >= per_roi) return;
  const int b = (int)(bs / (unsigned)sp.S);
  const int c = (int)(i / bins);
  const unsigned rem = i - (unsigned)c * bins;
  const int ph = (int)(rem / (unsigned)sp.PW), pw = (int)(rem - (unsigned)ph * (unsigned)sp.PW);
  const size_t e = (size_t)bs * (size_t)per_roi + (size_t)i;
  const int l = ar.roi_level[bs];
  float out = 0.0f;
  float r[4];
  for (int k = 0; k < 4; ++k) r[k] = ar.rois[(size_t)bs * 4 + (size_t)k];
  if (l >= 0 && l < sp.nl && gsr_rcnn::roi_finite<float>(r)) {            // (a level >= 0 was given to a finite row)
    const RoiMap mp = level_map(sp, l);
    out = gsr_rcnn::roi_pool_element(mp, pick(ar.features, l) + ((size_t)b * (size_t)sp.Cf + (size_t)c) * (size_t)mp.Hf * (size_t)mp.Wf, r, ph, pw);
  }
  ar.pooled[e] = out;
}

__global__ void __launch_bounds__(RB_THREADS) k_fpn_pool_bwd(PoolArgs ar) {
  __shared__ RoiBwdLds lds;
  const Spec& sp = ar.sp;
  const unsigned tile = blockIdx.x;
  int l = 0;
#pragma unroll
  for (int k = 1; k < MAX_LEVELS; ++k) l += tile >= ar.tile_start[k] ? 1 : 0;     // tile < tile_start[nl]: l < nl
  const RoiMap mp = level_map(sp, l);
  const unsigned local = tile - pick(ar.tile_start, l);
  const int tiles_x = (mp.Wf + RB_TILE - 1) / RB_TILE;
  const int x0 = (int)(local % (unsigned)tiles_x) * RB_TILE, y0 = (int)(local / (unsigned)tiles_x) * RB_TILE;
  const int c0 = (int)blockIdx.y * RB_CHUNK, b = (int)blockIdx.z;
  const int S = sp.S;
  const size_t row = (size_t)b * (size_t)sp.nl + (size_t)l;
  int n = ar.level_count[row];
  n = n < 0 ? 0 : (n > S ? S : n);
  const int32_t* list = ar.level_list + row * (size_t)S;
  const size_t per_roi = (size_t)sp.Cf * (size_t)sp.PH * (size_t)sp.PW;

  float acc[RB_PER];
#pragma unroll
  for (int k = 0; k < RB_PER; ++k) acc[k] = 0.0f;

  for (int i = 0; i < n; ++i) {                                           // n and s: the same in all lanes
    const int s = list[i];
    if (s < 0 || s >= S) continue;
    const size_t q = (size_t)b * (size_t)S + (size_t)s;
    gsr_rcnn::roi_bwd_step(mp, ar.rois + q * 4, ar.grad_pooled + q * per_roi, x0, y0, c0, lds, acc);
  }
  gsr_rcnn::roi_bwd_store(mp, pick(ar.grad_features, l) + (size_t)b * (size_t)sp.Cf * (size_t)mp.Hf * (size_t)mp.Wf, x0, y0, c0, ar.accumulate, acc);
}

}  // namespace gsr_fpn
