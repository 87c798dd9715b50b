// gsr_rpnloss.hip.h -- kernels of the RPN loss stage (gsr_rpnloss_label, gsr_rpnloss).  The arithmetic is gsr_rpnloss.h's,
// the same source the host harness compiles.  No float atomics: the rows' maxima travel as the bit images of non-negative
// floats through integer atomicMax (a maximum does not depend on the order of arrival, and it is read by the next launch
// only), the counts and histograms are integers, and every float sum adds the same operands in the same order on every
// run: the same input gives the same bits.
//
//   k_rpnloss_init      zeroes the rows' maxima [B,M] and the kinds' counts [B,2] (workspace)
//   k_rpnloss_rowmax    (ceil(R/256), B), one lane per anchor, the image's gt rows in LDS: the IoU of the anchor with every
//                       present row; a lane whose value exceeds the block's maximum so far raises it (LDS atomicMax), and
//                       lane m of the block raises row m's global maximum
//   k_rpnloss_prelabel  the same grid: the IoUs again by the same function (equality with a row's maximum is bit equality),
//                       the first-maximum row, the promotion, the pre-label; the kinds' counts by ballots, one integer
//                       atomicAdd per block and kind
//   k_rpnloss_select    (2, B), one workgroup per image and kind: the quota-th smallest composite key << 32 | r of the kind
//                       by gsr_block's block_select_u64, reads in index order; returns before it when the quota takes
//                       nothing or the whole kind, which every thread sees alike
//   k_rpnloss_labels    (ceil(R/256), B): label = the pre-label where the composite is at or below its kind's threshold,
//                       else -1; counts [B,4]
//   k_rpnloss_terms     (tiles of all levels, B), lanes along the logits' memory order (anchor a slowest, then y, x): r is
//                       computed from the lane's place, the logit and, for a positive, the four deltas are read coalesced and
//                       each gradient element stored once, coalesced; the block's two partial sums (LDS tree) -> the slab
//   k_rpnloss_final     one block: the slab in index order (strided runs, LDS tree) -> loss[3]
#pragma once
#include <hip/hip_runtime.h>

#include "gsr_block.hip.h"
#include "gsr_rpnloss.h"

namespace gsr_rpnl {

constexpr int RL_THREADS = 256;
constexpr int RL_SEL_THREADS = 1024;

struct LabelArgs {
  Spec sp;
  int32_t off[MAX_LEVELS + 1];
  int32_t R;
  const float* cells[MAX_LEVELS];    // level l: [A_l, 4]
  const float* gt_boxes;             // [B, M, 4]
  const int32_t* gt_cls;             // [B, M]
  uint32_t* rowmax;                  // workspace [B, M]: bit images of floats >= 0
  int32_t* kind_count;               // workspace [B, 2]: pre-labels 1, pre-labels 0
  unsigned long long* thr;           // workspace [B, 2]
  int32_t* pre;                      // workspace [B, R]
  int32_t* prelabels;                // [B, R] or NULL
  int32_t* labels;                   // [B, R]
  int32_t* matched;                  // [B, R]
  int32_t* counts;                   // [B, 4]
};

struct LossArgs {
  Spec sp;
  int32_t off[MAX_LEVELS + 1];
  int32_t R;
  uint32_t tile_start[MAX_LEVELS + 1];   // the first tile of level l; entries from nl on hold the total
  const float* cells[MAX_LEVELS];
  const float* logits[MAX_LEVELS];       // level l: [B, A_l, Hf_l, Wf_l]
  const float* deltas[MAX_LEVELS];       // level l: [B, 4 A_l, Hf_l, Wf_l]
  float* grad_logits[MAX_LEVELS];        // all NULL: not wanted
  float* grad_deltas[MAX_LEVELS];
  const float* gt_boxes;
  const int32_t* labels;
  const int32_t* matched;
  float* slab;                           // workspace [B * tiles, 2]
  float* loss;                           // [3]
  float norm;
};

__global__ void __launch_bounds__(RL_THREADS) k_rpnloss_init(LabelArgs ar) {
  const unsigned i = blockIdx.x * RL_THREADS + threadIdx.x;
  const unsigned n_max = (unsigned)ar.sp.B * (unsigned)ar.sp.M, n_cnt = (unsigned)ar.sp.B * 2u;
  if (i < n_max) ar.rowmax[i] = 0u;
  if (i < n_cnt) ar.kind_count[i] = 0;
}

// the image's gt rows into LDS; the caller's barrier follows
__device__ __forceinline__ void stage_rows(const LabelArgs& ar, int b, float* s_gt, int32_t* s_cls) {
  const int M = ar.sp.M;
  for (int m = threadIdx.x; m < M; m += RL_THREADS) {
    const size_t q = (size_t)b * (size_t)M + (size_t)m;
#pragma unroll
    for (int k = 0; k < 4; ++k) s_gt[m * 4 + k] = ar.gt_boxes[q * 4 + (size_t)k];
    s_cls[m] = ar.gt_cls[q];
  }
}

__global__ void __launch_bounds__(RL_THREADS) k_rpnloss_rowmax(LabelArgs ar) {
  __shared__ float s_gt[MAX_ROWS * 4];
  __shared__ int32_t s_cls[MAX_ROWS];
  __shared__ uint32_t s_max[MAX_ROWS];
  const Spec& sp = ar.sp;
  const int b = blockIdx.y, t = threadIdx.x, M = sp.M;
  stage_rows(ar, b, s_gt, s_cls);
  for (int m = t; m < M; m += RL_THREADS) s_max[m] = 0u;
  __syncthreads();
  const unsigned r = blockIdx.x * RL_THREADS + (unsigned)t;
  if (r < (unsigned)ar.R) {
    float anc[4];
    anchor_of<float>(sp, ar.off, ar.cells, (int)r, anc);
    for (int m = 0; m < M; ++m) {
      if (!row_present(s_cls[m])) continue;
      const float v = gsr_rcnn::pair_iou<float>(s_gt + m * 4, anc);
      if (v > 0.0f) {                                                       // false for a NaN
        const uint32_t u = __float_as_uint(v);                              // positive floats order as their bit images
        if (u > s_max[m]) atomicMax(&s_max[m], u);                          // (the read only spares atomics: the maximum rises)
      }
    }
  }
  __syncthreads();
  for (int m = t; m < M; m += RL_THREADS) {
    const uint32_t u = s_max[m];
    if (u != 0u) atomicMax(&ar.rowmax[(size_t)b * (size_t)M + (size_t)m], u);
  }
}

__global__ void __launch_bounds__(RL_THREADS) k_rpnloss_prelabel(LabelArgs ar) {
  __shared__ float s_gt[MAX_ROWS * 4];
  __shared__ int32_t s_cls[MAX_ROWS];
  __shared__ float s_rowmax[MAX_ROWS];
  __shared__ int s_kind[2];
  const Spec& sp = ar.sp;
  const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, M = sp.M;
  stage_rows(ar, b, s_gt, s_cls);
  for (int m = t; m < M; m += RL_THREADS) s_rowmax[m] = __uint_as_float(ar.rowmax[(size_t)b * (size_t)M + (size_t)m]);
  if (t < 2) s_kind[t] = 0;
  __syncthreads();
  const unsigned r = blockIdx.x * RL_THREADS + (unsigned)t;
  int pre = -1;
  if (r < (unsigned)ar.R) {
    float anc[4], best;
    int row;
    anchor_of<float>(sp, ar.off, ar.cells, (int)r, anc);
    const bool promoted = match_anchor<float>(anc, s_gt, s_cls, M, s_rowmax, best, row);
    pre = pre_label<float>(best, sp.iou_lo, sp.iou_hi, promoted);
    const size_t o = (size_t)b * (size_t)ar.R + (size_t)r;
    ar.pre[o] = pre;
    ar.matched[o] = row;
    if (ar.prelabels) ar.prelabels[o] = pre;
  }
  const bool live = r < (unsigned)ar.R;
  const int n1 = __popcll(__ballot(live && pre == 1)), n0 = __popcll(__ballot(live && pre == 0));
  if (lane == 0) {
    if (n1) atomicAdd(&s_kind[0], n1);
    if (n0) atomicAdd(&s_kind[1], n0);
  }
  __syncthreads();
  if (t < 2 && s_kind[t] != 0) atomicAdd(&ar.kind_count[(size_t)b * 2 + (size_t)t], s_kind[t]);   // integers: any order, one number
}

__global__ void __launch_bounds__(RL_SEL_THREADS) k_rpnloss_select(LabelArgs ar) {
  __shared__ uint32_t s_hist[256];
  const Spec& sp = ar.sp;
  const int kind = blockIdx.x, b = blockIdx.y, t = threadIdx.x, R = ar.R;
  const int all_pos = ar.kind_count[(size_t)b * 2], all_neg = ar.kind_count[(size_t)b * 2 + 1];
  int n_pos, n_neg;
  quotas(all_pos, all_neg, sp.batch_per_image, sp.pos_quota, n_pos, n_neg);
  const int have = kind == 0 ? all_pos : all_neg;
  const int want = kind == 0 ? n_pos : n_neg;                               // the same in all threads
  const int wanted_pre = kind == 0 ? 1 : 0;
  unsigned long long* out = ar.thr + (size_t)b * 2 + (size_t)kind;
  if (want <= 0 || want >= have) {                                          // nothing, or the whole kind: no select, and
    if (t == 0) *out = TAKE_ALL;                                            // no barrier has been met yet
    return;
  }
  const int32_t* pre = ar.pre + (size_t)b * (size_t)R;
  const auto key_at = [&](int r, uint64_t& key) {
    key = composite(sp.seed, b, r);                                         // needs no load: it runs while pre[r] is on its way
    return pre[r] == wanted_pre;
  };
  int taken;
  const uint64_t thr = gsr_block::block_select_u64<RL_SEL_THREADS>(s_hist, R, want, key_at, taken, have);
  if (t == 0) *out = thr;
}

__global__ void __launch_bounds__(RL_THREADS) k_rpnloss_labels(LabelArgs ar) {
  const Spec& sp = ar.sp;
  const int b = blockIdx.y;
  const unsigned r = blockIdx.x * RL_THREADS + threadIdx.x;
  const int all_pos = ar.kind_count[(size_t)b * 2], all_neg = ar.kind_count[(size_t)b * 2 + 1];
  int n_pos, n_neg;
  quotas(all_pos, all_neg, sp.batch_per_image, sp.pos_quota, n_pos, n_neg);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int32_t* c = ar.counts + (size_t)b * 4;
    c[0] = all_pos; c[1] = all_neg; c[2] = n_pos; c[3] = n_neg;
  }
  if (r >= (unsigned)ar.R) return;
  const uint64_t thr_pos = ar.thr[(size_t)b * 2], thr_neg = ar.thr[(size_t)b * 2 + 1];
  const size_t o = (size_t)b * (size_t)ar.R + (size_t)r;
  ar.labels[o] = final_label(ar.pre[o], composite(sp.seed, b, (int)r), n_pos, thr_pos, n_neg, thr_neg);
}

__global__ void __launch_bounds__(RL_THREADS) k_rpnloss_terms(LossArgs ar) {
  __shared__ float s_red[2][RL_THREADS];
  const Spec& sp = ar.sp;
  const unsigned tile = blockIdx.x;
  const int b = blockIdx.y, t = threadIdx.x;
  int l = 0;
#pragma unroll
  for (int k = 1; k < MAX_LEVELS; ++k) l += tile >= ar.tile_start[k] ? 1 : 0;       // tile < tile_start[nl]: l < nl
  const int A = pick(sp.A, l), Wf = pick(sp.Wf, l), HW = pick(sp.Hf, l) * Wf;
  const unsigned n_l = (unsigned)A * (unsigned)HW;
  const unsigned e = (tile - pick(ar.tile_start, l)) * RL_THREADS + (unsigned)t;    // (a, y, x) in the logits' memory order
  float cls = 0.0f, loc = 0.0f;
  if (e < n_l) {
    const int a = (int)(e / (unsigned)HW), p = (int)(e - (unsigned)a * (unsigned)HW);
    const int r = pick(ar.off, l) + p * A + a;
    const size_t o = (size_t)b * (size_t)ar.R + (size_t)r;
    const int label = ar.labels[o];
    const size_t le = (size_t)b * (size_t)n_l + (size_t)e;
    const size_t de = ((size_t)b * (size_t)(4 * A) + (size_t)(4 * a)) * (size_t)HW + (size_t)p;
    float logit = 0.0f, d[4] = {0.0f, 0.0f, 0.0f, 0.0f}, anc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool located = false;
    if (label == 0 || label == 1) logit = pick(ar.logits, l)[le];          // an unsampled anchor's values are never read
    if (label == 1) {
      const int m = ar.matched[o];
      if (m >= 0 && m < sp.M) {
        const float* dl = pick(ar.deltas, l);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          d[k] = dl[de + (size_t)k * (size_t)HW];
          gt[k] = ar.gt_boxes[((size_t)b * (size_t)sp.M + (size_t)m) * 4 + (size_t)k];
        }
        const int y = p / Wf, x = p - y * Wf;
        const float* c = pick(ar.cells, l) + (size_t)a * 4;
        const float cell[4] = {c[0], c[1], c[2], c[3]};
        gsr_rpn::anchor_at<float>(cell, x, y, pick(sp.stride, l), pick(sp.shift0, l), anc);
        located = true;
      }
    }
    float g_logit, g_d[4];
    anchor_terms<float>(label, located, logit, d, anc, gt, sp.beta, cls, loc, g_logit, g_d);
    float* gl = pick(ar.grad_logits, l);
    float* gd = pick(ar.grad_deltas, l);
    const float k_cls = sp.w_cls / ar.norm, k_loc = sp.w_loc / ar.norm;
    if (gl) gl[le] = (label == 0 || label == 1) ? k_cls * g_logit : 0.0f;
    if (gd) {
#pragma unroll
      for (int k = 0; k < 4; ++k) gd[de + (size_t)k * (size_t)HW] = located ? k_loc * g_d[k] : 0.0f;
    }
  }
  s_red[0][t] = cls;
  s_red[1][t] = loc;
  gsr_block::block_tree_sum(s_red);
  if (t == 0) {
    const size_t row = (size_t)b * (size_t)gridDim.x + (size_t)tile;
    ar.slab[row * 2] = s_red[0][0];
    ar.slab[row * 2 + 1] = s_red[1][0];
  }
}

__global__ void __launch_bounds__(RL_THREADS) k_rpnloss_final(LossArgs ar, unsigned nblocks) {
  __shared__ float s_red[2][RL_THREADS];
  gsr_block::slab_sum(ar.slab, nblocks, s_red);
  if (threadIdx.x == 0) finish<float>(s_red[0][0], s_red[1][0], ar.sp.w_cls, ar.sp.w_loc, ar.norm, ar.loss);
}

}  // namespace gsr_rpnl
