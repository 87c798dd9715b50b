// gsr_detloss.hip.h -- kernels of the detector's loss stage (gsr_detloss).  The arithmetic is gsr_detloss.h's, the same
// source the host harness compiles.  No float atomics: every sum is a per-thread run, a fixed LDS tree and a slab of
// per-block partials that one block adds up in index order, so the same input gives the same bits on every run.
//
//   k_detloss_metrics   one lane per (image, anchor), rows of A coalesced: the candidate test against every present gt row;
//                       only an anchor that is a candidate of some row decodes its box (64 bins) and writes ov / metric,
//                       the others write zeros.
//   k_detloss_assign    one workgroup per image.  Top-k: one wave per gt row, k passes over the row's candidates, each
//                       taking the smallest composite above the previous one (a wave min over two 32-bit halves; no
//                       barrier inside, the trip counts are wave-uniform).  Then one thread per taken (row, anchor) entry:
//                       an anchor in more than one row's list goes to the row with the largest ov over all present rows;
//                       one thread per row takes the maxima over its final positives; the entries write tgt / ts; the
//                       image's sum of ts is a strided run per thread and an LDS tree.
//   k_detloss_terms<V>  grid (anchor tiles, 1 + class chunks, images); V anchors per lane (4 with 16-byte loads and
//                       stores when A % 4 == 0 and the tensors start on 16-byte boundaries, else 1).  Chunk 0: the 64 box
//                       channels -- zeros on background, CIoU + DFL forward and gradient on foreground.  Chunks 1..:
//                       16 classes each, BCE forward and gradient, one read of the logit and one write of the gradient.
//                       1 / tss comes from the per-image sums (added in image order by every thread alike).
//   k_detloss_final     one block adds the slab in index order and writes loss[4].
#pragma once
#include <hip/hip_runtime.h>

#include "gsr_block.hip.h"
#include "gsr_detloss.h"

namespace gsr_dloss {

using gsr_block::block_tree_sum;
using gsr_block::slab_sum;

constexpr int MET_THREADS = 128;
constexpr int ASG_THREADS = 1024;
constexpr int ASG_WAVES = ASG_THREADS / 64;
constexpr int TERM_THREADS = 256;
constexpr int CLS_CHUNK = 16;
constexpr int FIN_THREADS = 256;

struct Args {
  Spec sp;
  const float* pred;          // [B, 64 + C, A]
  const float* gt_boxes;      // [B, M, 4]
  const int32_t* gt_cls;      // [B, M]
  float* ov;                  // workspace [B, M, A]
  float* metric;              // workspace [B, M, A]
  int32_t* tgt;               // workspace [B, A]
  float* ts;                  // workspace [B, A]
  float* ts_sum;              // workspace [B]
  float* slab;                // workspace [blocks of k_detloss_terms, 3]
  float* loss;                // [4]
  float* grad_pred;           // [B, 64 + C, A] or NULL
  int32_t* tgt_out;           // [B, A] or NULL
  float* ts_out;              // [B, A] or NULL
};

// ---- (a) ov and metric of every (row, anchor) ---------------------------------------------------------------------------
__global__ void __launch_bounds__(MET_THREADS) k_detloss_metrics(Args ar) {
  const Spec& sp = ar.sp;
  const long long g = (long long)blockIdx.x * MET_THREADS + threadIdx.x;
  if (g >= (long long)sp.B * (long long)sp.A) return;
  const int b = (int)(g / sp.A), a = (int)(g % sp.A);
  const size_t A = (size_t)sp.A;
  float gx, gy, st;
  anchor_point(sp, a, gx, gy, st);
  const float px = gx * st, py = gy * st;
  const float* gtb = ar.gt_boxes + (size_t)b * (size_t)sp.M * 4;
  const int32_t* gtc = ar.gt_cls + (size_t)b * (size_t)sp.M;
  uint32_t mask = 0u;
  for (int m = 0; m < sp.M; ++m)
    if (present(gtc[m], sp.C) && is_candidate<float>(px, py, gtb + (size_t)m * 4)) mask |= 1u << m;
  const float* p = ar.pred + (size_t)b * (size_t)channels(sp) * A + (size_t)a;
  Box<float> pp;
  pp.x1 = pp.y1 = pp.x2 = pp.y2 = 0.0f;
  if (mask) {
    const Box<float> q = decode_grid<float>(p, A, gx, gy);
    pp.x1 = q.x1 * st; pp.y1 = q.y1 * st; pp.x2 = q.x2 * st; pp.y2 = q.y2 * st;
  }
  for (int m = 0; m < sp.M; ++m) {
    float ov = 0.0f, met = 0.0f;
    if ((mask >> m) & 1u)
      candidate_metric<float>(gtb + (size_t)m * 4, pp, p[(size_t)(BOX_CH + gtc[m]) * A], sp.alpha, sp.beta, ov, met);
    const size_t o = ((size_t)b * (size_t)sp.M + (size_t)m) * A + (size_t)a;
    ar.ov[o] = ov;
    ar.metric[o] = met;
  }
}

// ---- (b) the assignment of one image --------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
    const uint64_t o = ((uint64_t)hi << 32) | (uint64_t)lo;
    v = o < v ? o : v;
  }
  return v;
}

__global__ void __launch_bounds__(ASG_THREADS) k_detloss_assign(Args ar) {
  __shared__ int32_t s_sel[MAX_ROWS * MAX_TOPK];     // entry (row, j): the anchor taken, or -1
  __shared__ int32_t s_fin[MAX_ROWS * MAX_TOPK];     // the row the entry's anchor finally goes to
  __shared__ float s_eov[MAX_ROWS * MAX_TOPK], s_emet[MAX_ROWS * MAX_TOPK];
  __shared__ float s_rov[MAX_ROWS], s_rmet[MAX_ROWS];
  __shared__ int32_t s_cls[MAX_ROWS];                // -1: absent
  __shared__ float s_gt[MAX_ROWS * 4];
  __shared__ float s_red[1][ASG_THREADS];
  const Spec& sp = ar.sp;
  const int b = blockIdx.x, t = threadIdx.x, A = sp.A, M = sp.M, K = sp.topk;
  const int E = M * K;                               // <= 512
  const float* ovb = ar.ov + (size_t)b * (size_t)M * (size_t)A;
  const float* metb = ar.metric + (size_t)b * (size_t)M * (size_t)A;
  int32_t* tgt = ar.tgt + (size_t)b * (size_t)A;
  float* ts = ar.ts + (size_t)b * (size_t)A;
  int32_t* tgt_o = ar.tgt_out ? ar.tgt_out + (size_t)b * (size_t)A : nullptr;
  float* ts_o = ar.ts_out ? ar.ts_out + (size_t)b * (size_t)A : nullptr;

  if (t < M) {
    const int c = ar.gt_cls[(size_t)b * (size_t)M + (size_t)t];
    s_cls[t] = present(c, sp.C) ? c : -1;
    for (int i = 0; i < 4; ++i) s_gt[t * 4 + i] = ar.gt_boxes[((size_t)b * (size_t)M + (size_t)t) * 4 + (size_t)i];
  }
  if (t < E) s_sel[t] = -1;
  for (int a = t; a < A; a += ASG_THREADS) {
    tgt[a] = -1;
    ts[a] = 0.0f;
    if (tgt_o) tgt_o[a] = -1;
    if (ts_o) ts_o[a] = 0.0f;
  }
  __syncthreads();

  // top-k: wave w takes the rows w, w + 16; every quantity that steers the loops is the same in all 64 lanes
  const int wave = t >> 6, lane = t & 63;
  for (int m = wave; m < M; m += ASG_WAVES) {
    if (s_cls[m] < 0) continue;
    const float* met = metb + (size_t)m * (size_t)A;
    const float* gt = s_gt + m * 4;
    uint64_t prev = 0ull;
    for (int j = 0; j < K; ++j) {
      uint64_t best = ~0ull;                         // no composite has all bits set (an anchor index is below 2^31)
      for (int a = lane; a < A; a += 64) {
        if (!anchor_is_candidate<float>(sp, a, gt)) continue;
        const uint64_t c = order_composite<float>(met[a], a);
        if ((j == 0 || c > prev) && c < best) best = c;
      }
      best = wave_min_u64(best);
      if (best == ~0ull) break;
      if (lane == 0) s_sel[m * K + j] = (int32_t)(uint32_t)best;
      prev = best;
    }
  }
  __syncthreads();

  // conflicts: an anchor in more than one list goes to the row with the largest ov over all present rows (lowest on ties)
  if (t < E) {
    const int a = s_sel[t];
    int fin = -1;
    float eo = 0.0f, em = 0.0f;
    if (a >= 0) {
      int n = 0;
      for (int e = 0; e < E; ++e) n += s_sel[e] == a ? 1 : 0;
      fin = t / K;
      if (n > 1) {
        bool first = true;
        float bo = 0.0f;
        for (int m = 0; m < M; ++m) {
          if (s_cls[m] < 0) continue;
          const float o = ovb[(size_t)m * (size_t)A + (size_t)a];
          if (first || o > bo) { bo = o; fin = m; first = false; }
        }
      }
      eo = ovb[(size_t)fin * (size_t)A + (size_t)a];
      em = metb[(size_t)fin * (size_t)A + (size_t)a];
    }
    s_fin[t] = fin;
    s_eov[t] = eo;
    s_emet[t] = em;
  }
  __syncthreads();
  if (t < M) {
    float mo = 0.0f, mm = 0.0f;
    for (int e = 0; e < E; ++e)
      if (s_fin[e] == t) {
        mo = s_eov[e] > mo ? s_eov[e] : mo;
        mm = s_emet[e] > mm ? s_emet[e] : mm;
      }
    s_rov[t] = mo;
    s_rmet[t] = mm;
  }
  __syncthreads();
  if (t < E && s_sel[t] >= 0) {                      // entries of one anchor all write the same values
    const int a = s_sel[t], fin = s_fin[t];
    const float v = target_score<float>(s_emet[t], s_rov[fin], s_rmet[fin]);
    tgt[a] = fin;
    ts[a] = v;
    if (tgt_o) tgt_o[a] = fin;
    if (ts_o) ts_o[a] = v;
  }
  __syncthreads();

  float acc = 0.0f;
  for (int a = t; a < A; a += ASG_THREADS) acc += ts[a];
  s_red[0][t] = acc;
  block_tree_sum(s_red);
  if (t == 0) ar.ts_sum[b] = s_red[0][0];
}

// ---- (c) the loss terms and the gradient ------------------------------------------------------------------------------------
__device__ __forceinline__ float detloss_tss(const float* ts_sum, int B) {
  float s = 0.0f;
  for (int i = 0; i < B; ++i) s += ts_sum[i];
  return clamp_tss<float>(s);
}

template <int V>
__device__ __forceinline__ void load_v(const float* p, float* v) {
  if (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = p[0];
  }
}

template <int V>
__device__ __forceinline__ void store_v(float* p, const float* v) {
  if (V == 4)
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else
    p[0] = v[0];
}

template <int V>
__global__ void __launch_bounds__(TERM_THREADS) k_detloss_terms(Args ar) {
  __shared__ float s_red[3][TERM_THREADS];
  const Spec& sp = ar.sp;
  const int t = threadIdx.x, b = blockIdx.z, chunk = blockIdx.y;
  const size_t A = (size_t)sp.A;
  const long long a0 = ((long long)blockIdx.x * TERM_THREADS + t) * V;
  const bool live = a0 < (long long)sp.A;            // V == 4: A % 4 == 0, so a group lies inside or outside as a whole
  const float tss = detloss_tss(ar.ts_sum, sp.B);
  const float fB = (float)sp.B;
  float acc_box = 0.0f, acc_cls = 0.0f, acc_dfl = 0.0f;
  if (live) {
    const size_t a = (size_t)a0;
    const float* pb = ar.pred + (size_t)b * (size_t)channels(sp) * A + a;
    float* gb = ar.grad_pred ? ar.grad_pred + (size_t)b * (size_t)channels(sp) * A + a : nullptr;
    int tg[V];
    float tv[V];
    bool any = false;
    for (int v = 0; v < V; ++v) {
      tg[v] = ar.tgt[(size_t)b * A + a + (size_t)v];
      tg[v] = tg[v] < sp.M ? tg[v] : -1;             // never past the rows, whatever the floats were
      tv[v] = ar.ts[(size_t)b * A + a + (size_t)v];
      any = any || tg[v] >= 0;
    }
    if (chunk == 0) {
      if (!any) {
        if (gb) {
          float z[V];
          for (int v = 0; v < V; ++v) z[v] = 0.0f;
          for (int k = 0; k < BOX_CH; ++k) store_v<V>(gb + (size_t)k * A, z);
        }
      } else {
        for (int v = 0; v < V; ++v) {
          if (tg[v] < 0) {
            if (gb)
              for (int k = 0; k < BOX_CH; ++k) gb[(size_t)k * A + (size_t)v] = 0.0f;
            continue;
          }
          float gx, gy, st;
          anchor_point(sp, (int)a + v, gx, gy, st);
          const float w = tv[v] / tss;
          float bt, dt;
          box_dfl_anchor<float>(pb + v, A, gx, gy, st, ar.gt_boxes + ((size_t)b * (size_t)sp.M + (size_t)tg[v]) * 4,
                                fB * sp.w_box * w, fB * sp.w_dfl * w, gb ? gb + v : nullptr, A, bt, dt);
          acc_box += bt * tv[v];
          acc_dfl += dt * tv[v];
        }
      }
    } else {
      int tc[V];
      for (int v = 0; v < V; ++v) tc[v] = tg[v] >= 0 ? ar.gt_cls[(size_t)b * (size_t)sp.M + (size_t)tg[v]] : -1;
      const float kc = fB * sp.w_cls / tss;
      const int c0 = (chunk - 1) * CLS_CHUNK, c1 = c0 + CLS_CHUNK < sp.C ? c0 + CLS_CHUNK : sp.C;
      for (int c = c0; c < c1; ++c) {
        float x[V], g[V];
        load_v<V>(pb + (size_t)(BOX_CH + c) * A, x);
        for (int v = 0; v < V; ++v) {
          float d;
          acc_cls += bce<float>(x[v], tc[v] == c ? tv[v] : 0.0f, &d);
          g[v] = kc * d;
        }
        if (gb) store_v<V>(gb + (size_t)(BOX_CH + c) * A, g);
      }
    }
  }
  s_red[0][t] = acc_box;
  s_red[1][t] = acc_cls;
  s_red[2][t] = acc_dfl;
  block_tree_sum(s_red);
  if (t < 3) {
    const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    ar.slab[blk * 3 + (size_t)t] = s_red[t][0];
  }
}

// ---- (d) the slab -> loss[4] ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FIN_THREADS) k_detloss_final(Args ar, unsigned nblocks) {
  __shared__ float s_red[3][FIN_THREADS];
  const Spec& sp = ar.sp;
  const int t = threadIdx.x;
  slab_sum<3, FIN_THREADS>(ar.slab, nblocks, s_red);
  if (t == 0) {
    const float tss = detloss_tss(ar.ts_sum, sp.B);
    const float box = s_red[0][0] / tss, cls = s_red[1][0] / tss, dfl = s_red[2][0] / tss;
    ar.loss[0] = box;
    ar.loss[1] = cls;
    ar.loss[2] = dfl;
    ar.loss[3] = (float)sp.B * (sp.w_box * box + sp.w_cls * cls + sp.w_dfl * dfl);
  }
}

}  // namespace gsr_dloss
