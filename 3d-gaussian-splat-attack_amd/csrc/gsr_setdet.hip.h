// gsr_setdet.hip.h -- kernels of the set-prediction detector stage (gsr_setdet_loss, gsr_setdet_postprocess).  The
// arithmetic is gsr_setdet.h's, the same source the host harness compiles.  No float atomics: every sum is a per-thread
// run, a wave butterfly or a fixed LDS tree and a slab of per-block partials that one block adds up in index order, so the
// same input gives the same bits on every run.
//
//   k_setdet_cost    one wave per (image, query): the maximum and the sum of exponentials of its C + 1 logits (lanes stride
//                    the row, wave butterflies), kept as stats [B,Q,2]; then lane m < M writes cost[b,m,q] of a present row.
//   k_setdet_match   one workgroup per image: gsr_setdet.h's match_rows with the columns dealt over the lanes.  Per pass:
//                    every lane scans its columns (reduced cost, minv / way update, its closest column), a wave butterfly
//                    and one LDS slot per wave give (delta, j1) by closer() -- the smallest value, the lowest column among
//                    equals -- and the lanes shift u / v / minv.  Everything that steers the loops is the same in all
//                    lanes, so the barriers are uniform.  Writes tgt, the optional outputs and the image's matched count.
//   k_setdet_terms   flat over the B * Q * (C + 1) logits, 4 per lane a workgroup-width apart: the cross-entropy gradient of
//                    each, the CE term where c is the query's target class, and at c == 0 the query's box terms and box
//                    gradient (zeros for an unmatched query).  The normalisers come from the per-image counts (integers).
//   k_setdet_final   one block adds the slab in index order and writes loss[4].
//   k_setdet_post    one workgroup per image, one lane per query: its statistics, class and score in index order, then a
//                    scan of the kept flags gives every kept query its row: query order.
#pragma once
#include <hip/hip_runtime.h>

#include "gsr_block.hip.h"
#include "gsr_setdet.h"

namespace gsr_setdet {

using gsr_block::block_scan;
using gsr_block::block_tree_sum;
using gsr_block::slab_sum;
using gsr_block::wave_softmax_stats;

constexpr int COST_THREADS = 256;
constexpr int COST_WAVES = COST_THREADS / 64;
constexpr int MATCH_THREADS = 256;
constexpr int MATCH_WAVES = MATCH_THREADS / 64;
constexpr int TERM_THREADS = 256;
constexpr int TERM_PER = 4;
constexpr int TERM_TILE = TERM_THREADS * TERM_PER;
constexpr int FIN_THREADS = 256;
constexpr int POST_THREADS = MAX_QUERIES;

struct Args {
  Spec sp;
  const float* logits;        // [B, Q, C + 1]
  const float* boxes;         // [B, Q, 4]
  const float* gt_boxes;      // [B, M, 4]
  const int32_t* gt_cls;      // [B, M]
  float* stats;               // workspace [B, Q, 2]
  float* cost;                // workspace [B, M, Q]
  int32_t* tgt;               // workspace [B, Q]
  int32_t* nmatch;            // workspace [B]
  float* slab;                // workspace [blocks of k_setdet_terms, 3]
  float* loss;                // [4]
  float* grad_logits;         // [B, Q, C + 1] or NULL
  float* grad_boxes;          // [B, Q, 4] or NULL
  int32_t* match_out;         // [B, M] or NULL
  int32_t* tgt_out;           // [B, Q] or NULL
};

// ---- (a) statistics and the cost matrix -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(COST_THREADS) k_setdet_cost(Args ar) {
  const Spec& sp = ar.sp;
  const int lane = threadIdx.x & 63;
  const long long gq = (long long)blockIdx.x * COST_WAVES + (threadIdx.x >> 6);
  if (gq >= (long long)sp.B * (long long)sp.Q) return;                  // the same in all lanes of a wave
  const int b = (int)(gq / sp.Q), q = (int)(gq % sp.Q);
  const int n = sp.C + 1;
  const float* x = ar.logits + (size_t)gq * (size_t)n;
  float mx, sum;
  wave_softmax_stats(x, n, lane, mx, sum);
  if (lane == 0) {
    ar.stats[(size_t)gq * 2] = mx;
    ar.stats[(size_t)gq * 2 + 1] = sum;
  }
  if (lane < sp.M) {
    const int cls = ar.gt_cls[(size_t)b * (size_t)sp.M + (size_t)lane];
    float c = 0.0f;
    if (present(cls, sp.C)) {
      float gt[4], bx[4];
      gt_normalise<float>(ar.gt_boxes + ((size_t)b * (size_t)sp.M + (size_t)lane) * 4, sp.img_w, sp.img_h, gt);
      for (int i = 0; i < 4; ++i) bx[i] = ar.boxes[(size_t)gq * 4 + (size_t)i];
      c = pair_cost<float>(softmax_prob<float>(x[cls], mx, sum), bx, gt, sp.c_class, sp.c_l1, sp.c_giou);
    }
    ar.cost[((size_t)b * (size_t)sp.M + (size_t)lane) * (size_t)sp.Q + (size_t)q] = c;
  }
}

// ---- (b) the match of one image ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MATCH_THREADS) k_setdet_match(Args ar) {
  __shared__ float s_u[MAX_ROWS + 1], s_v[MAX_QUERIES + 1], s_minv[MAX_QUERIES + 1];
  __shared__ int32_t s_p[MAX_QUERIES + 1], s_way[MAX_QUERIES + 1], s_used[MAX_QUERIES + 1];
  __shared__ int32_t s_cls[MAX_ROWS], s_match[MAX_ROWS];
  __shared__ float s_bv[MATCH_WAVES];
  __shared__ int32_t s_bj[MATCH_WAVES];
  const Spec& sp = ar.sp;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int M = sp.M, Q = sp.Q;
  const float* cost = ar.cost + (size_t)b * (size_t)M * (size_t)Q;
  const float inf = m_inf<float>();

  if (t <= M) s_u[t] = 0.0f;
  if (t < M) {
    s_cls[t] = ar.gt_cls[(size_t)b * (size_t)M + (size_t)t];
    s_match[t] = -1;
  }
  for (int j = t; j <= Q; j += MATCH_THREADS) { s_v[j] = 0.0f; s_p[j] = 0; }
  __syncthreads();

  for (int i = 1; i <= M; ++i) {
    if (!present(s_cls[i - 1], sp.C)) continue;                         // the same in every lane
    for (int j = t; j <= Q; j += MATCH_THREADS) { s_minv[j] = inf; s_used[j] = 0; s_way[j] = 0; }
    if (t == 0) s_p[0] = i;
    int j0 = 0;
    __syncthreads();
    for (int it = 0; it <= M; ++it) {
      if (t == 0) s_used[j0] = 1;
      __syncthreads();
      const int i0 = s_p[j0];
      const float ui = s_u[i0];
      const float* row = cost + (size_t)(i0 - 1) * (size_t)Q;
      float bv = inf;
      int bj = -1;
      for (int j = 1 + t; j <= Q; j += MATCH_THREADS) {
        if (s_used[j]) continue;
        const float cur = reduced<float>(row[j - 1], ui, s_v[j]);
        float mv = s_minv[j];
        if (cur < mv) { mv = cur; s_minv[j] = cur; s_way[j] = j0; }
        if (closer<float>(mv, j, bv, bj)) { bv = mv; bj = j; }
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(bv, m);
        const int oj = __shfl_xor(bj, m);
        if (closer<float>(ov, oj, bv, bj)) { bv = ov; bj = oj; }
      }
      if (lane == 0) { s_bv[wave] = bv; s_bj[wave] = bj; }
      __syncthreads();
      float delta = inf;
      int j1 = -1;
      for (int w = 0; w < MATCH_WAVES; ++w)
        if (closer<float>(s_bv[w], s_bj[w], delta, j1)) { delta = s_bv[w]; j1 = s_bj[w]; }
      if (!(delta < inf)) {                                             // nothing below +inf: the lowest unmarked column
        __syncthreads();                                                // every lane has read s_bj
        int lo = 0x7fffffff;
        for (int j = 1 + t; j <= Q; j += MATCH_THREADS)
          if (!s_used[j] && j < lo) lo = j;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
          const int o = __shfl_xor(lo, m);
          lo = o < lo ? o : lo;
        }
        if (lane == 0) s_bj[wave] = lo;
        __syncthreads();
        lo = 0x7fffffff;
        for (int w = 0; w < MATCH_WAVES; ++w) lo = s_bj[w] < lo ? s_bj[w] : lo;
        j1 = lo <= Q ? lo : -1;
        delta = 0.0f;
      }
      if (j1 < 0) break;                                                // cannot happen while Q >= M; the same in every lane
      for (int j = t; j <= Q; j += MATCH_THREADS) {
        if (s_used[j]) {                                                // marked columns hold distinct rows
          const int r = s_p[j];
          s_u[r] = s_u[r] + delta;
          s_v[j] = s_v[j] - delta;
        } else {
          s_minv[j] = s_minv[j] - delta;
        }
      }
      __syncthreads();
      j0 = j1;
      if (s_p[j0] == 0) break;
    }
    __syncthreads();
    if (t == 0) {
      for (int it = 0; it <= M && j0 != 0; ++it) {
        const int j1 = s_way[j0];
        s_p[j0] = s_p[j1];
        j0 = j1;
      }
    }
    __syncthreads();
  }

  int32_t* tgt = ar.tgt + (size_t)b * (size_t)Q;
  int32_t* tgt_o = ar.tgt_out ? ar.tgt_out + (size_t)b * (size_t)Q : nullptr;
  for (int j = 1 + t; j <= Q; j += MATCH_THREADS) {
    int i = s_p[j];
    i = i <= M ? i : 0;
    tgt[j - 1] = i - 1;
    if (tgt_o) tgt_o[j - 1] = i - 1;
    if (i > 0) s_match[i - 1] = j - 1;                                  // one column per row
  }
  __syncthreads();
  if (t < M && ar.match_out) ar.match_out[(size_t)b * (size_t)M + (size_t)t] = s_match[t];
  if (t == 0) {
    int n = 0;
    for (int m = 0; m < M; ++m) n += s_match[m] >= 0 ? 1 : 0;
    ar.nmatch[b] = n;
  }
}

// ---- (c) the loss terms and the gradients -------------------------------------------------------------------------------------
// the batch's matched rows: integers, so any order gives the same number
template <int THREADS>
__device__ __forceinline__ long long block_matched(const int32_t* nmatch, int B, int (&s_cnt)[1][THREADS]) {
  const int t = threadIdx.x;
  int n = 0;
  for (int i = t; i < B; i += THREADS) n += nmatch[i];
  s_cnt[0][t] = n;
  block_tree_sum(s_cnt);
  return (long long)s_cnt[0][0];
}

__global__ void __launch_bounds__(TERM_THREADS) k_setdet_terms(Args ar) {
  __shared__ float s_red[3][TERM_THREADS];
  __shared__ int s_cnt[1][TERM_THREADS];
  const Spec& sp = ar.sp;
  const int t = threadIdx.x;
  const unsigned n1 = (unsigned)sp.C + 1u;
  const unsigned long long total = (unsigned long long)sp.B * (unsigned long long)sp.Q * n1;
  const long long matched = block_matched<TERM_THREADS>(ar.nmatch, sp.B, s_cnt);
  const float nb = norm_boxes<float>(matched);
  const float wsum = norm_ce<float>(matched, (long long)sp.B * (long long)sp.Q, sp.eos_coef);
  const float kce = sp.w_ce / wsum, kl1 = sp.w_l1 / nb, kg = sp.w_giou / nb;
  float acc_ce = 0.0f, acc_l1 = 0.0f, acc_g = 0.0f;
  for (int r = 0; r < TERM_PER; ++r) {
    const unsigned long long e = (unsigned long long)blockIdx.x * TERM_TILE + (unsigned long long)(r * TERM_THREADS + t);
    if (e >= total) break;
    const unsigned qi = (unsigned)(e / n1);
    const int c = (int)(e - (unsigned long long)qi * n1);
    const int b = (int)(qi / (unsigned)sp.Q);
    int tg = ar.tgt[qi];
    tg = tg < sp.M ? tg : -1;                                           // never past the rows, whatever the floats were
    int tc = tg >= 0 ? ar.gt_cls[(size_t)b * (size_t)sp.M + (size_t)tg] : sp.C;
    tc = present(tc, sp.C) ? tc : sp.C;
    const float wt = tc == sp.C ? sp.eos_coef : 1.0f;
    const float mx = ar.stats[(size_t)qi * 2], sum = ar.stats[(size_t)qi * 2 + 1];
    const float x = ar.logits[e];
    if (ar.grad_logits) ar.grad_logits[e] = (kce * wt) * (softmax_prob<float>(x, mx, sum) - (c == tc ? 1.0f : 0.0f));
    if (c == tc) acc_ce += wt * -log_softmax<float>(x, mx, sum);
    if (c == 0) {
      float* gb = ar.grad_boxes ? ar.grad_boxes + (size_t)qi * 4 : nullptr;
      if (tg >= 0) {
        float gt[4], bx[4], g[4], l1, gterm;
        gt_normalise<float>(ar.gt_boxes + ((size_t)b * (size_t)sp.M + (size_t)tg) * 4, sp.img_w, sp.img_h, gt);
        for (int i = 0; i < 4; ++i) bx[i] = ar.boxes[(size_t)qi * 4 + (size_t)i];
        pair_terms<float>(bx, gt, kl1, kg, gb ? g : nullptr, l1, gterm);
        acc_l1 += l1;
        acc_g += gterm;
        if (gb)
          for (int i = 0; i < 4; ++i) gb[i] = g[i];
      } else if (gb) {
        for (int i = 0; i < 4; ++i) gb[i] = 0.0f;
      }
    }
  }
  s_red[0][t] = acc_ce;
  s_red[1][t] = acc_l1;
  s_red[2][t] = acc_g;
  block_tree_sum(s_red);
  if (t < 3) ar.slab[(size_t)blockIdx.x * 3 + (size_t)t] = s_red[t][0];
}

// ---- (d) the slab -> loss[4] ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FIN_THREADS) k_setdet_final(Args ar, unsigned nblocks) {
  __shared__ float s_red[3][FIN_THREADS];
  __shared__ int s_cnt[1][FIN_THREADS];
  const Spec& sp = ar.sp;
  const int t = threadIdx.x;
  const long long matched = block_matched<FIN_THREADS>(ar.nmatch, sp.B, s_cnt);
  slab_sum<3, FIN_THREADS>(ar.slab, nblocks, s_red);
  if (t == 0) {
    const float nb = norm_boxes<float>(matched);
    const float wsum = norm_ce<float>(matched, (long long)sp.B * (long long)sp.Q, sp.eos_coef);
    const float ce = s_red[0][0] / wsum, l1 = s_red[1][0] / nb, gi = s_red[2][0] / nb;
    ar.loss[0] = ce;
    ar.loss[1] = l1;
    ar.loss[2] = gi;
    ar.loss[3] = sp.w_ce * ce + sp.w_l1 * l1 + sp.w_giou * gi;
  }
}

// ---- the output stage -----------------------------------------------------------------------------------------------------------
// blockDim.x = Q rounded up to a whole wave; lane t is query t
__global__ void __launch_bounds__(POST_THREADS) k_setdet_post(Spec sp, const float* logits, const float* boxes, float* dets,
                                                              int32_t* counts) {
  __shared__ int32_t s_scan[POST_THREADS];
  const int b = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
  const int Q = sp.Q, n = sp.C + 1;
  float bp = -INFINITY;
  int bc = 0x7fffffff;
  if (t < Q) {
    const float* x = logits + ((size_t)b * (size_t)Q + (size_t)t) * (size_t)n;
    float mx, sum;
    softmax_stats<float>(x, n, mx, sum);
    for (int c = 0; c < sp.C; ++c) {
      const float p = softmax_prob<float>(x[c], mx, sum);
      if (score_better<float>(p, c, bp, bc)) { bp = p; bc = c; }
    }
  }
  const int mine = bp > sp.conf_thr ? 1 : 0;                            // false for a NaN score and for t >= Q
  const int incl = block_scan(s_scan, mine, nt);
  const int above = s_scan[nt - 1];
  const int kept = above < sp.max_det ? above : sp.max_det;
  float* out = dets + (size_t)b * (size_t)sp.max_det * 6;
  const int pos = incl - mine;
  if (mine && pos < sp.max_det) {
    float bx[4], o[4];
    for (int k = 0; k < 4; ++k) bx[k] = boxes[((size_t)b * (size_t)Q + (size_t)t) * 4 + (size_t)k];
    out_box<float>(bx, sp.img_w, sp.img_h, o);
    float* row = out + (size_t)pos * 6;
    row[0] = o[0]; row[1] = o[1]; row[2] = o[2]; row[3] = o[3];
    row[4] = bp;
    row[5] = (float)(bc < sp.C ? bc : 0);
  }
  for (int i = kept * 6 + t; i < sp.max_det * 6; i += nt) out[i] = 0.0f;
  if (t == 0) {
    counts[(size_t)b * 2] = kept;
    counts[(size_t)b * 2 + 1] = above;
  }
}

}  // namespace gsr_setdet
