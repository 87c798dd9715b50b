// gsr_rpnloss.h -- the RPN loss stage: an anchor's place among the levels, its match and low-quality promotion, the
// pre-label, the keyed sample's composite and the final label, and the two loss terms of one anchor with a hand-written
// backward (include/gsraster.h, GsrRpnLossSpec).
//
// Pure scalar functions, usable from the HIP kernels (gsr_rpnloss.hip.h, T = float) and from a host C++ harness (g++;
// tests/host_math/rpnloss_host.cpp, T = float and T = double).  Every function that rounds starts with GSR_FP_STRICT (the
// host build adds -ffp-contract=off): each product, sum and quotient is rounded once, in source order, on both sides.
//
// Nothing is written a second time: the IoU, the key, the target deltas and smooth L1 are gsr_rcnn.h's, the anchor and its
// index gsr_rpn.h's, the binary cross-entropy gsr_detloss.h's.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gsr_detloss.h"  // bce
#include "gsr_math.h"     // GSR_HD, GSR_FP_STRICT
#include "gsr_rcnn.h"     // pair_iou, sample_key, target_deltas, smooth_l1
#include "gsr_rpn.h"      // anchor_at, split_index

namespace gsr_rpnl {

constexpr int MAX_LEVELS = 5;
constexpr int MAX_ROWS = 256;              // gt rows per image
constexpr int MAX_ANCHORS = 1 << 24;       // R: anchors per image, all levels
constexpr int MAX_BATCH = 1 << 16;         // batch_per_image
constexpr uint64_t TAKE_ALL = ~0ull;       // the threshold of a kind whose quota takes all of it

// What the kernels take by value (GsrRpnLossSpec, field for field).
struct Spec {
  int32_t B, M, nl;
  int32_t A[MAX_LEVELS], Hf[MAX_LEVELS], Wf[MAX_LEVELS], stride[MAX_LEVELS];
  float shift0[MAX_LEVELS];
  int32_t batch_per_image, pos_quota;
  uint32_t seed;
  float iou_lo, iou_hi;
  float beta, w_cls, w_loc;
  uint32_t flags;
};

// element l of a table of MAX_LEVELS entries by selects: no indexed read, so a by-value table stays in registers
template <class V>
GSR_HD V pick(const V* a, int l) {
  V v = a[0];
#pragma unroll
  for (int k = 1; k < MAX_LEVELS; ++k) v = l == k ? a[k] : v;
  return v;
}

// off[l]: the flat index of level l's first anchor; entries from nl on, off[MAX_LEVELS] included, hold R.  -> R
GSR_HD long long level_offsets(const Spec& sp, int32_t* off) {
  long long r = 0;
  for (int l = 0; l <= MAX_LEVELS; ++l) {
    off[l] = (int32_t)(r > 0x7fffffffll ? 0x7fffffffll : r);
    if (l < sp.nl && l < MAX_LEVELS) r += (long long)sp.A[l] * (long long)sp.Hf[l] * (long long)sp.Wf[l];
  }
  return r;
}

GSR_HD int level_of(int r, const int32_t* off) {
  int l = 0;
#pragma unroll
  for (int k = 1; k < MAX_LEVELS; ++k) l += r >= off[k] ? 1 : 0;           // r < R = off[k] for k >= nl
  return l;
}

// anchor r = off[l] + (y * Wf + x) * A + a of the image: DefaultAnchorGenerator's box
template <class T>
GSR_HD void anchor_of(const Spec& sp, const int32_t* off, const float* const* cells, int r, T* anc) {
  const int l = level_of(r, off);
  int a, x, y;
  gsr_rpn::split_index(r - pick(off, l), pick(sp.A, l), pick(sp.Wf, l), a, x, y);
  const float* c = pick(cells, l) + (size_t)a * 4;
  const T cell[4] = {(T)c[0], (T)c[1], (T)c[2], (T)c[3]};
  gsr_rpn::anchor_at<T>(cell, x, y, pick(sp.stride, l), (T)pick(sp.shift0, l), anc);
}

// a gt row is present iff its class is not negative: the RPN is class-agnostic
GSR_HD bool row_present(int cls) { return cls >= 0; }

// Matcher on one anchor.  best / row: the first maximum of the IoU over the present rows in ascending m (a NaN is never the
// maximum); -1 / -1 without a present row.  rowmax (NULL: no promotion): the rows' maxima over all anchors; -> the anchor
// reaches the maximum of some present row whose maximum is above 0 (Matcher's low-quality match, with the stated rule that
// a row nothing overlaps promotes nothing).
template <class T>
GSR_HD bool match_anchor(const T* anc, const T* gt_boxes, const int32_t* gt_cls, int M, const T* rowmax, T& best, int& row) {
  T bv = (T)-1;
  int bm = -1;
  bool promoted = false;
  for (int m = 0; m < M; ++m) {
    if (!row_present(gt_cls[m])) continue;
    const T v = gsr_rcnn::pair_iou<T>(gt_boxes + (size_t)m * 4, anc);
    if (v > bv) { bv = v; bm = m; }
    if (rowmax && rowmax[m] > (T)0 && v == rowmax[m]) promoted = true;
  }
  best = bv;
  row = bm;
  return promoted;
}

// 0 below iou_lo, -1 in [iou_lo, iou_hi), 1 from iou_hi on; a promoted anchor 1
template <class T>
GSR_HD int pre_label(T best, T iou_lo, T iou_hi, bool promoted) {
  if (promoted) return 1;
  return best < iou_lo ? 0 : (best < iou_hi ? -1 : 1);
}

// the sample orders a kind by (key, r) ascending: one 64-bit word, unique within an image
GSR_HD uint64_t composite(uint32_t seed, int b, int r) {
  return ((uint64_t)gsr_rcnn::sample_key(seed, b, r) << 32) | (uint64_t)(uint32_t)r;
}

GSR_HD void quotas(int n_pos_all, int n_neg_all, int batch_per_image, int pos_quota, int& n_pos, int& n_neg) {
  n_pos = n_pos_all < pos_quota ? n_pos_all : pos_quota;
  const int rest = batch_per_image - n_pos;
  n_neg = n_neg_all < rest ? n_neg_all : rest;
}

// thr_*: the n-th smallest composite of the kind (TAKE_ALL when the quota takes the whole kind)
GSR_HD int final_label(int pre, uint64_t comp, int n_pos, uint64_t thr_pos, int n_neg, uint64_t thr_neg) {
  if (pre == 1) return (n_pos > 0 && comp <= thr_pos) ? 1 : -1;
  if (pre == 0) return (n_neg > 0 && comp <= thr_neg) ? 0 : -1;
  return -1;
}

// The unweighted terms of one anchor and their derivatives.  label: 1, 0, anything else takes no part (zeros, and neither
// the logit nor the deltas are looked at).  gt: the matched row's box, read only when `located` (label 1 and the matched row
// in range); otherwise the anchor stays out of the localisation term.
template <class T>
GSR_HD void anchor_terms(int label, bool located, T logit, const T* d, const T* anc, const T* gt, T beta, T& cls, T& loc, T& g_logit, T* g_d) {
  GSR_FP_STRICT
  cls = (T)0; loc = (T)0; g_logit = (T)0;
  g_d[0] = g_d[1] = g_d[2] = g_d[3] = (T)0;
  if (label != 0 && label != 1) return;
  cls = gsr_dloss::bce<T>(logit, (T)label, &g_logit);
  if (label != 1 || !located) return;
  const T w[4] = {(T)1, (T)1, (T)1, (T)1};
  T t[4];
  gsr_rcnn::target_deltas<T>(anc, gt, w, t);
#pragma unroll
  for (int k = 0; k < 4; ++k) loc = loc + gsr_rcnn::smooth_l1<T>(d[k] - t[k], beta, g_d[k]);
}

// loss[3] = total, cls, loc from the two sums; norm = batch_per_image * B
template <class T>
GSR_HD void finish(T s_cls, T s_loc, T w_cls, T w_loc, T norm, T* loss) {
  GSR_FP_STRICT
  loss[1] = (w_cls * s_cls) / norm;
  loss[2] = (w_loc * s_loc) / norm;
  loss[0] = loss[1] + loss[2];
}

}  // namespace gsr_rpnl
