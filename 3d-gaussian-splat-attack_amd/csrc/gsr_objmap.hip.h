// gsr_objmap.hip.h -- kernels of the object-map classifier (gsr_objmap).  The per-pixel arithmetic is gsr_objmap.h's, shared
// with the host harness.  The torch expression torch.argmax(Conv2d(16, K, 1)(map), 0) writes a [K,H,W] logit tensor and
// reads it back (2.1 GB each way at K = 256, 1080p); here a lane keeps its pixel's 16 features in registers and walks the
// classes, and no logit is ever stored.  No float atomics, no MFMA (its accumulation order is not the host twin's), no
// inline assembly; wave64.
//
//   k_objmap_init       (INIT_BLOCKS, B) x 256.  Stats rows -> (0, INT_MAX, INT_MAX, 0, 0).  With a loss: each workgroup
//                       counts, over a strided run of its image's pixels and an integer LDS tree, the pixels the loss will
//                       count (target in 0..K-1 and some logit > -inf; the class walk stops at the first such logit, the
//                       first class as a rule) -> vpart[b][block].  The slab needs no clearing: every classify workgroup
//                       writes its own entry.
//   k_objmap_classify   (ceil(H W / 256), B) x 256, one lane per pixel: 16 coalesced plane reads into registers; pass 1 the
//                       maximum and the id; pass 2 (confidence or loss wanted) sum exp and the target's logit; pass 3 (LOSS
//                       with a gradient) the logits again in class order into 16 accumulators.  The class index is
//                       wave-uniform, so W's rows and b are read with uniform addresses, as k_group_classify reads them
//                       (through the scalar cache; 16 + 1 SGPRs per class, no LDS, no barrier in the class loop).  Staging
//                       W in LDS instead would take 68 KiB at K = 1024 and turn every operand into an LDS read.
//                       Per-class statistics go through an LDS table (5 K ints, dynamic) and are flushed with one integer
//                       atomicAdd / atomicMin / atomicMax set per (workgroup, class present): commutative integer updates,
//                       the same bits in any order of arrival.  The workgroup's CE terms: an LDS tree -> slab[b][block].
//   k_objmap_final      B x 256: empty classes' rows -> five zeros; the image's slab in index order -> terms[b] = (mean CE,
//                       valid as float).
//
// weight [K,16] and bias [K] are kernel parameters of their own, declared __restrict__: the kernels store to other tensors
// before and between the class walks, and only a pointer known not to alias those stores keeps its uniform loads scalar.
//
// Every loop that holds a barrier has a workgroup-uniform trip count (the trees, the strided table loops around barriers).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>

#include "gsr_block.hip.h"
#include "gsr_objmap.h"

namespace gsr_om {

struct Args {
  int32_t B, H, W, K;
  int32_t hw, nblk;         // pixels and classify workgroups per image
  const float* objmap;      // [B,16,H,W]
  const int32_t* target;    // [B,H,W] or null
  const uint8_t* palette;   // [K,3] or null
  float* slab;              // workspace: [B][nblk] CE partials
  int32_t* vpart;           // workspace: [B][INIT_BLOCKS] counted pixels
  int32_t* ids;             // [B,H,W]
  float* conf;              // [B,H,W] or null
  int32_t* stats;           // [B,K,5] or null: count, x0, y0, x1, y1
  uint8_t* paint;           // [B,H,W,3] or null
  float* terms;             // [B,2] or null
  float* grad;              // [B,16,H,W] or null
};

__device__ __forceinline__ void load_features(const Args& ar, int b, int p, bool live, float f[CH]) {
  const float* base = ar.objmap + (size_t)b * CH * (size_t)ar.hw + (size_t)p;
#pragma unroll
  for (int k = 0; k < CH; ++k) f[k] = live ? base[(size_t)k * (size_t)ar.hw] : 0.0f;
}

// the image's counted pixels from k_objmap_init's partials: integers, any order gives the same sum
__device__ __forceinline__ int32_t valid_of(const Args& ar, int b, int32_t (&s_cnt)[1][OM_THREADS]) {
  const int t = threadIdx.x;
  s_cnt[0][t] = t < INIT_BLOCKS ? ar.vpart[(size_t)b * INIT_BLOCKS + t] : 0;
  gsr_block::block_tree_sum(s_cnt);
  return s_cnt[0][0];
}

__global__ void __launch_bounds__(OM_THREADS) k_objmap_init(Args ar, const float* __restrict__ weight, const float* __restrict__ bias, int with_loss) {
  __shared__ int32_t s_cnt[1][OM_THREADS];
  const int t = threadIdx.x, b = blockIdx.y;
  if (ar.stats) {
    int32_t* rows = ar.stats + (size_t)b * (size_t)ar.K * 5;
    for (int c = (int)blockIdx.x * OM_THREADS + t; c < ar.K; c += INIT_BLOCKS * OM_THREADS) {
      rows[5 * c] = 0; rows[5 * c + 1] = INT_MAX; rows[5 * c + 2] = INT_MAX; rows[5 * c + 3] = 0; rows[5 * c + 4] = 0;
    }
  }
  if (!with_loss) return;                                  // (uniform: no barrier is skipped by part of a workgroup)
  int32_t n = 0;
  for (long long q = (long long)blockIdx.x * OM_THREADS + t; q < ar.hw; q += INIT_BLOCKS * OM_THREADS) {   // (hw may be 2^31 - 1)
    const int p = (int)q;
    const int tg = ar.target[(size_t)b * (size_t)ar.hw + (size_t)p];
    if (tg < 0 || tg >= ar.K) continue;
    float f[CH];
    load_features(ar, b, p, true, f);
    n += alive(weight, bias, ar.K, f) ? 1 : 0;
  }
  s_cnt[0][t] = n;
  gsr_block::block_tree_sum(s_cnt);
  if (t == 0) ar.vpart[(size_t)b * INIT_BLOCKS + blockIdx.x] = s_cnt[0][0];
}

template <bool LOSS>
__global__ void __launch_bounds__(OM_THREADS) k_objmap_classify(Args ar, const float* __restrict__ weight, const float* __restrict__ bias) {
  extern __shared__ int32_t s_stat[];                      // [5][K] with stats, else nothing
  __shared__ float s_red[1][OM_THREADS];
  __shared__ int32_t s_cnt[1][OM_THREADS];
  const int t = threadIdx.x, b = blockIdx.y, K = ar.K;
  const long long q = (long long)blockIdx.x * OM_THREADS + t;   // (hw may be 2^31 - 1: past it only as a long long)
  const bool live = q < ar.hw;
  const int p = live ? (int)q : 0;
  const size_t px = (size_t)b * (size_t)ar.hw + (size_t)p;

  if (ar.stats) {
    for (int c = t; c < K; c += OM_THREADS) {
      s_stat[c] = 0; s_stat[K + c] = INT_MAX; s_stat[2 * K + c] = INT_MAX; s_stat[3 * K + c] = 0; s_stat[4 * K + c] = 0;
    }
  }
  float scale = 0.0f;
  if (LOSS) scale = inv_valid(valid_of(ar, b, s_cnt));    // (holds barriers: the table above is set before anyone adds to it)
  else if (ar.stats) __syncthreads();

  float f[CH];
  load_features(ar, b, p, live, f);
  float m;
  int id;
  pass_max(weight, bias, K, f, m, id);
  if (live) {
    ar.ids[px] = id;
    if (ar.paint) {
      uint8_t r = 0, g = 0, bl = 0;
      if (id >= 0) { r = ar.palette[3 * id]; g = ar.palette[3 * id + 1]; bl = ar.palette[3 * id + 2]; }
      ar.paint[3 * px] = r; ar.paint[3 * px + 1] = g; ar.paint[3 * px + 2] = bl;
    }
    if (ar.stats && id >= 0) {
      const int y = p / ar.W, x = p - y * ar.W;
      atomicAdd(&s_stat[id], 1);
      atomicMin(&s_stat[K + id], x);
      atomicMin(&s_stat[2 * K + id], y);
      atomicMax(&s_stat[3 * K + id], x + 1);
      atomicMax(&s_stat[4 * K + id], y + 1);
    }
  }

  if (LOSS || ar.conf) {
    const int tg = (LOSS && live) ? ar.target[px] : -1;
    float l_t = 0.0f;
    const float sum = pass_sum(weight, bias, K, f, m, tg, l_t);
    const float cf = confidence(id, sum);
    if (live && ar.conf) ar.conf[px] = cf;
    if (LOSS) {
      const bool cnt = live && counted(id, tg, K);
      if (ar.terms) {
        s_red[0][t] = cnt ? ce_term(m, l_t, sum) : 0.0f;
        gsr_block::block_tree_sum(s_red);
        if (t == 0) ar.slab[(size_t)b * (size_t)ar.nblk + blockIdx.x] = s_red[0][0];
      }
      if (ar.grad) {
        float g[CH];
        pass_grad(weight, bias, K, f, m, cf, tg, scale, g);
        if (live) {
          float* go = ar.grad + (size_t)b * CH * (size_t)ar.hw + (size_t)p;
#pragma unroll
          for (int k = 0; k < CH; ++k) go[(size_t)k * (size_t)ar.hw] = cnt ? g[k] : 0.0f;
        }
      }
    }
  }

  if (ar.stats) {
    __syncthreads();
    int32_t* rows = ar.stats + (size_t)b * (size_t)K * 5;
    for (int c = t; c < K; c += OM_THREADS) {
      const int32_t n = s_stat[c];
      if (n == 0) continue;
      atomicAdd(&rows[5 * c], n);
      atomicMin(&rows[5 * c + 1], s_stat[K + c]);
      atomicMin(&rows[5 * c + 2], s_stat[2 * K + c]);
      atomicMax(&rows[5 * c + 3], s_stat[3 * K + c]);
      atomicMax(&rows[5 * c + 4], s_stat[4 * K + c]);
    }
  }
}

__global__ void __launch_bounds__(OM_THREADS) k_objmap_final(Args ar) {
  __shared__ float s_red[1][OM_THREADS];
  __shared__ int32_t s_cnt[1][OM_THREADS];
  const int t = threadIdx.x, b = blockIdx.x;
  if (ar.stats) {
    int32_t* rows = ar.stats + (size_t)b * (size_t)ar.K * 5;
    for (int c = t; c < ar.K; c += OM_THREADS)
      if (rows[5 * c] == 0) { rows[5 * c + 1] = 0; rows[5 * c + 2] = 0; rows[5 * c + 3] = 0; rows[5 * c + 4] = 0; }
  }
  if (!ar.terms) return;                                   // (uniform)
  const int32_t valid = valid_of(ar, b, s_cnt);
  gsr_block::slab_sum(ar.slab + (size_t)b * (size_t)ar.nblk, (unsigned)ar.nblk, s_red);
  if (t == 0) {
    ar.terms[2 * b] = mean_ce(s_red[0][0], valid);
    ar.terms[2 * b + 1] = (float)valid;
  }
}

}  // namespace gsr_om
