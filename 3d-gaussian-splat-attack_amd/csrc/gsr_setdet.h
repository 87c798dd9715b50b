// gsr_setdet.h -- the set-prediction (DETR-style) detector stage: the matching cost, the one-to-one match of ground-truth
// rows to queries (shortest augmenting paths with dual potentials), DETR's set criterion (weighted cross-entropy, L1, GIoU)
// with a hand-written backward, and the output stage's per-query class / score / box (include/gsraster.h, GsrSetDetSpec).
//
// Pure scalar functions, usable from the HIP kernels (gsr_setdet.hip.h, T = float) and from a host C++ harness (g++;
// tests/host_math/setdet_host.cpp, T = float and T = double: the double build is what the hand-written backward is
// checked against by finite differences of its own forward).  Every function that rounds starts with GSR_FP_STRICT (the
// host build adds -ffp-contract=off).
//
// The match is written twice: match_rows() below walks the columns one by one, the kernel deals them over the lanes of a
// workgroup.  Both take the same steps in the same order -- reduced(), the strict `<` of the column scan and closer() are
// shared -- so for finite costs they return the same pairs, ties included.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gsr_detmath.h"   // m_exp, m_log, dmax_da, dmin_da, present, the softmax pieces
#include "gsr_math.h"      // GSR_HD, GSR_FP_STRICT

namespace gsr_setdet {

using gsr_detmath::dmax_da;
using gsr_detmath::dmin_da;
using gsr_detmath::log_softmax;
using gsr_detmath::m_exp;
using gsr_detmath::m_log;
using gsr_detmath::present;
using gsr_detmath::softmax_prob;
using gsr_detmath::softmax_stats;   // of one query's n = C + 1 logits

constexpr int MAX_ROWS = 32;       // gt rows per image
constexpr int MAX_QUERIES = 1024;
constexpr int MAX_CLASSES = 1024;

// What the kernels take by value.
struct Spec {
  int32_t B, Q, C, M;
  float img_w, img_h;
  float c_class, c_l1, c_giou;
  float w_ce, w_l1, w_giou, eos_coef;
  float conf_thr;
  int32_t max_det;
};

template <class T>
GSR_HD T m_inf() { return (T)INFINITY; }

// gt x1 y1 x2 y2 in pixels of the (img_w, img_h) frame -> normalised (cx, cy, w, h)
template <class T>
GSR_HD void gt_normalise(const T* gt, T img_w, T img_h, T* out) {
  GSR_FP_STRICT
  out[0] = (gt[0] + gt[2]) * (T)0.5 / img_w;
  out[1] = (gt[1] + gt[3]) * (T)0.5 / img_h;
  out[2] = (gt[2] - gt[0]) / img_w;
  out[3] = (gt[3] - gt[1]) / img_h;
}

template <class T>
GSR_HD void to_xyxy(const T* b, T* o) {
  GSR_FP_STRICT
  o[0] = b[0] - (T)0.5 * b[2];
  o[1] = b[1] - (T)0.5 * b[3];
  o[2] = b[0] + (T)0.5 * b[2];
  o[3] = b[1] + (T)0.5 * b[3];
}

// ---- GIoU(a, b) on x1 y1 x2 y2, no epsilon; g (may be NULL): d giou / d (a.x1, a.y1, a.x2, a.y2)
template <class T>
GSR_HD T giou(const T* a, const T* b, T* g) {
  GSR_FP_STRICT
  const T aw = a[2] - a[0], ah = a[3] - a[1];
  const T area_a = aw * ah, area_b = (b[2] - b[0]) * (b[3] - b[1]);
  const T ix1 = a[0] > b[0] ? a[0] : b[0], ix2 = a[2] < b[2] ? a[2] : b[2];
  const T iy1 = a[1] > b[1] ? a[1] : b[1], iy2 = a[3] < b[3] ? a[3] : b[3];
  const T rw = ix2 - ix1, rh = iy2 - iy1;
  const T iw = rw > (T)0 ? rw : (T)0, ih = rh > (T)0 ? rh : (T)0;
  const T inter = iw * ih;
  const T uni = area_a + area_b - inter;
  const T iou = inter / uni;
  const T ex1 = a[0] < b[0] ? a[0] : b[0], ex2 = a[2] > b[2] ? a[2] : b[2];
  const T ey1 = a[1] < b[1] ? a[1] : b[1], ey2 = a[3] > b[3] ? a[3] : b[3];
  const T qw = ex2 - ex1, qh = ey2 - ey1;
  const T ew = qw > (T)0 ? qw : (T)0, eh = qh > (T)0 ? qh : (T)0;
  const T encl = ew * eh;
  const T gap = (encl - uni) / encl;
  if (g) {
    // a clamp passes its gradient where its argument is >= 0 (torch.clamp); a tie of max / min is shared in halves
    const T pw = rw >= (T)0 ? ih : (T)0, ph = rh >= (T)0 ? iw : (T)0;    // d inter / d rw, d inter / d rh
    const T di[4] = {-pw * dmax_da(a[0], b[0]), -ph * dmax_da(a[1], b[1]), pw * dmin_da(a[2], b[2]), ph * dmin_da(a[3], b[3])};
    const T da[4] = {-ah, -aw, ah, aw};                                   // d area_a
    const T cw = qw >= (T)0 ? eh : (T)0, ch = qh >= (T)0 ? ew : (T)0;    // d encl / d qw, d encl / d qh
    const T de[4] = {-cw * dmin_da(a[0], b[0]), -ch * dmin_da(a[1], b[1]), cw * dmax_da(a[2], b[2]), ch * dmax_da(a[3], b[3])};
    for (int i = 0; i < 4; ++i) {
      const T duni = da[i] - di[i];
      const T diou = (di[i] - iou * duni) / uni;
      const T dgap = ((de[i] - duni) - gap * de[i]) / encl;
      g[i] = diou - dgap;
    }
  }
  return iou - gap;
}

// ---- the matching cost of one (row, query): p_cls = softmax(logits_q)[cls_m]; box and gt normalised (cx, cy, w, h)
template <class T>
GSR_HD T pair_cost(T p_cls, const T* box, const T* gt, T c_class, T c_l1, T c_giou) {
  GSR_FP_STRICT
  T l1 = (T)0;
  for (int i = 0; i < 4; ++i) {
    const T d = box[i] - gt[i];
    l1 = l1 + (d < (T)0 ? -d : d);
  }
  T a[4], b[4];
  to_xyxy(box, a);
  to_xyxy(gt, b);
  return -c_class * p_cls + c_l1 * l1 + -c_giou * giou<T>(a, b, nullptr);
}

// ---- one matched pair of the loss: l1 = sum |box - gt|, gterm = 1 - GIoU; gb (may be NULL): where
// k_l1 * d l1 / d box + k_giou * d gterm / d box goes (4 values, box = cx cy w h)
template <class T>
GSR_HD void pair_terms(const T* box, const T* gt, T k_l1, T k_giou, T* gb, T& l1, T& gterm) {
  GSR_FP_STRICT
  T s = (T)0, sg[4];
  for (int i = 0; i < 4; ++i) {
    const T d = box[i] - gt[i];
    s = s + (d < (T)0 ? -d : d);
    sg[i] = d > (T)0 ? (T)1 : (d < (T)0 ? (T)-1 : (T)0);               // sign(0) = 0; a NaN gives 0
  }
  T a[4], b[4], g[4] = {(T)0, (T)0, (T)0, (T)0};
  to_xyxy(box, a);
  to_xyxy(gt, b);
  const T gi = giou<T>(a, b, gb ? g : nullptr);
  l1 = s;
  gterm = (T)1 - gi;
  if (gb) {
    // x1 = cx - w/2, x2 = cx + w/2: d / d cx = g_x1 + g_x2, d / d w = (g_x2 - g_x1) / 2; gterm falls as giou rises
    const T dg[4] = {g[0] + g[2], g[1] + g[3], (T)0.5 * (g[2] - g[0]), (T)0.5 * (g[3] - g[1])};
    for (int i = 0; i < 4; ++i) gb[i] = k_l1 * sg[i] - k_giou * dg[i];
  }
}

// ---- the normalisers: n = max(#matched, 1); wsum = the sum of wt[t] over all B * Q queries
template <class T>
GSR_HD T norm_boxes(long long matched) { return matched > 0 ? (T)matched : (T)1; }
template <class T>
GSR_HD T norm_ce(long long matched, long long queries, T eos_coef) {
  GSR_FP_STRICT
  return (T)matched + eos_coef * (T)(queries - matched);
}

// ---- the match.  Columns are 1 .. Q (column j is query j - 1), column 0 is the virtual start; rows are 1 .. M.
// The reduced cost of (row i0, column j), rounded in this order:
template <class T>
GSR_HD T reduced(T cost, T u_i0, T v_j) {
  GSR_FP_STRICT
  return (cost - u_i0) - v_j;
}

// (value, column) a is closer than b: the smaller value, the lower column among equals.  j < 0: no candidate.
template <class T>
GSR_HD bool closer(T va, int ja, T vb, int jb) {
  if (ja < 0) return false;
  if (jb < 0) return true;
  return va < vb || (va == vb && ja < jb);
}

// One image.  cost [M, Q] (row m at cost + m * Q; rows that are not present are not read), cls [M].
// u [M + 1], v / minv [Q + 1] of T and p / way / used [Q + 1] of int32 are scratch.  match [M] and tgt [Q] are written.
// Returns the number of matched rows.  Every loop is bounded by M and Q alone, whatever the floats are.
template <class T>
GSR_HD int match_rows(const T* cost, const int32_t* cls, int M, int Q, int C, T* u, T* v, T* minv, int32_t* p, int32_t* way,
                      int32_t* used, int32_t* match, int32_t* tgt) {
  GSR_FP_STRICT
  for (int i = 0; i <= M; ++i) u[i] = (T)0;
  for (int j = 0; j <= Q; ++j) { v[j] = (T)0; p[j] = 0; }
  for (int i = 1; i <= M; ++i) {
    if (!present(cls[i - 1], C)) continue;
    p[0] = i;
    int j0 = 0;
    for (int j = 0; j <= Q; ++j) { minv[j] = m_inf<T>(); used[j] = 0; way[j] = 0; }
    for (int it = 0; it <= M; ++it) {                   // every pass marks one more column; at most (rows so far) + 1
      used[j0] = 1;
      const int i0 = p[j0];
      const T* row = cost + (size_t)(i0 - 1) * (size_t)Q;
      T delta = m_inf<T>();
      int j1 = -1;
      for (int j = 1; j <= Q; ++j) {
        if (used[j]) continue;
        const T cur = reduced<T>(row[j - 1], u[i0], v[j]);
        if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
        if (closer<T>(minv[j], j, delta, j1)) { delta = minv[j]; j1 = j; }
      }
      if (!(delta < m_inf<T>())) {                      // nothing compares below +inf: the lowest unmarked column, no shift
        j1 = -1;
        for (int j = Q; j >= 1; --j)
          if (!used[j]) j1 = j;
        delta = (T)0;
      }
      if (j1 < 0) break;                                // cannot happen while Q >= M
      for (int j = 0; j <= Q; ++j) {
        if (used[j]) { u[p[j]] = u[p[j]] + delta; v[j] = v[j] - delta; }
        else minv[j] = minv[j] - delta;
      }
      j0 = j1;
      if (p[j0] == 0) break;
    }
    for (int it = 0; it <= M && j0 != 0; ++it) {        // flip the path back to column 0
      const int j1 = way[j0];
      p[j0] = p[j1];
      j0 = j1;
    }
  }
  for (int m = 0; m < M; ++m) match[m] = -1;
  int n = 0;
  for (int j = 1; j <= Q; ++j) {
    const int i = p[j];
    tgt[j - 1] = i > 0 ? i - 1 : -1;
    if (i > 0) { match[i - 1] = j - 1; ++n; }
  }
  return n;
}

// ---- the output stage: the class and score of one query from its statistics.  The first maximum of p[c] over c < C (a NaN
// is never the maximum); no class above -inf: class 0, score -inf.
template <class T>
GSR_HD bool score_better(T pa, int ca, T pb, int cb) { return pa > pb || (pa == pb && ca < cb); }

template <class T>
GSR_HD void out_box(const T* box, T img_w, T img_h, T* o) {
  GSR_FP_STRICT
  o[0] = (box[0] - (T)0.5 * box[2]) * img_w;
  o[1] = (box[1] - (T)0.5 * box[3]) * img_h;
  o[2] = (box[0] + (T)0.5 * box[2]) * img_w;
  o[3] = (box[1] + (T)0.5 * box[3]) * img_h;
}

}  // namespace gsr_setdet
