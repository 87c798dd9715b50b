// gsr_rcnn.h -- the two-stage (R-CNN-style) detector stage: the proposal sampler's IoU, match and key, RoIAlign's axis
// set-up and bilinear read, the box head's loss terms with a hand-written backward, and the output stage's class / score /
// box (include/gsraster.h, GsrRcnnSpec).
//
// Pure scalar functions, usable from the HIP kernels (gsr_rcnn.hip.h, T = float) and from a host C++ harness (g++;
// tests/host_math/rcnn_host.cpp, T = float and T = double).  Every function that rounds starts with GSR_FP_STRICT (the
// host build adds -ffp-contract=off): each product, sum and quotient is rounded once, in source order, on both sides.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gsr_detmath.h"   // m_exp, m_log, present, is_finite, the softmax pieces
#include "gsr_math.h"      // GSR_HD, GSR_FP_STRICT

namespace gsr_rcnn {

using gsr_detmath::is_finite;
using gsr_detmath::log_softmax;
using gsr_detmath::m_exp;
using gsr_detmath::m_log;
using gsr_detmath::present;
using gsr_detmath::softmax_prob;
using gsr_detmath::softmax_stats;

constexpr int MAX_ROWS = 32;         // gt rows per image
constexpr int MAX_SAMPLE = 1024;     // RoIs per image
constexpr int MAX_CAND = 4096;       // R + M of the sampler, R of the output stage
constexpr int MAX_CLASSES = 1024;
constexpr int MAX_POOL = 14;         // PH, PW
constexpr int MAX_GRID = 16;         // samples per bin and axis
constexpr uint32_t CLASS_AGNOSTIC = 1u;   // = GSR_RCNN_CLASS_AGNOSTIC

// What the kernels take by value (GsrRcnnSpec, field for field).
struct Spec {
  int32_t B, R, M, S, C;
  int32_t max_pos, append_gt;
  uint32_t seed;
  float fg_iou;
  int32_t Cf, Hf, Wf, PH, PW;
  float spatial_scale;
  int32_t sampling_ratio;
  float bw_x, bw_y, bw_w, bw_h;
  float beta, w_cls, w_box;
  float conf_thr, iou_thr;
  int32_t max_det;
  float img_w, img_h;
  uint32_t flags;
};

// ---- the sampler ------------------------------------------------------------------------------------------------------
GSR_HD uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

GSR_HD uint32_t sample_key(uint32_t seed, int b, int i) { return mix32(mix32(seed ^ ((uint32_t)b * 0x9E3779B9u)) + (uint32_t)i); }

// (key, index) a comes before b
GSR_HD bool key_before(uint32_t ka, int ia, uint32_t kb, int ib) { return ka < kb || (ka == kb && ia < ib); }

// Detectron2's pairwise_iou of two x1 y1 x2 y2 boxes: 0 where they do not intersect
template <class T>
GSR_HD T pair_iou(const T* a, const T* b) {
  GSR_FP_STRICT
  const T area_a = (a[2] - a[0]) * (a[3] - a[1]), area_b = (b[2] - b[0]) * (b[3] - b[1]);
  const T lx = a[0] > b[0] ? a[0] : b[0], ly = a[1] > b[1] ? a[1] : b[1];
  const T rx = a[2] < b[2] ? a[2] : b[2], ry = a[3] < b[3] ? a[3] : b[3];
  T iw = rx - lx, ih = ry - ly;
  iw = iw > (T)0 ? iw : (T)0;
  ih = ih > (T)0 ? ih : (T)0;
  const T inter = iw * ih;
  const T sum = area_a + area_b;
  return inter > (T)0 ? inter / (sum - inter) : (T)0;
}

// The match of one candidate: the first maximum of its IoU over the present rows in ascending m (a NaN is never the
// maximum).  -> the row, or -1 for background (no present row, or the maximum below fg_iou); best: that maximum, -1 if none.
template <class T>
GSR_HD int match_candidate(const T* box, const T* gt_boxes, const int32_t* gt_cls, int M, int C, T fg_iou, T& best) {
  T bv = (T)-1;
  int bm = -1;
  for (int m = 0; m < M; ++m) {
    if (!present(gt_cls[m], C)) continue;
    const T v = pair_iou<T>(box, gt_boxes + (size_t)m * 4);
    if (v > bv) { bv = v; bm = m; }
  }
  best = bv;
  return (bm >= 0 && bv >= fg_iou) ? bm : -1;
}

// ---- RoIAlign -----------------------------------------------------------------------------------------------------------
// one axis of a RoI: lo, hi in image pixels -> start, the bin length and the samples per bin (0..MAX_GRID)
template <class T>
GSR_HD void roi_axis(T lo, T hi, T scale, int P, int sampling_ratio, T& start, T& bin, int& grid) {
  GSR_FP_STRICT
  start = lo * scale - (T)0.5;
  const T end = hi * scale - (T)0.5;
  const T len = end - start;
  bin = len / (T)P;
  int g;
  if (sampling_ratio > 0) {
    g = sampling_ratio;
  } else {
    const T c = ceil(bin);
    g = c >= (T)MAX_GRID ? MAX_GRID : (c >= (T)1 ? (int)c : 0);           // a NaN gives 0
  }
  grid = g > MAX_GRID ? MAX_GRID : g;
}

template <class T>
GSR_HD bool roi_finite(const T* r) { return is_finite(r[0]) && is_finite(r[1]) && is_finite(r[2]) && is_finite(r[3]); }

// sample i of bin p
template <class T>
GSR_HD T sample_pos(T start, T bin, int grid, int p, int i) {
  GSR_FP_STRICT
  return start + (T)p * bin + ((T)i + (T)0.5) * bin / (T)grid;
}

// one axis of the bilinear read at y on a map of n cells: false where the read is 0; otherwise the two cells and weights
template <class T>
GSR_HD bool lerp_axis(T y, int n, int& lo, int& hi, T& wl, T& wh) {
  GSR_FP_STRICT
  if (!(y >= (T)-1 && y <= (T)n)) return false;
  y = y > (T)0 ? y : (T)0;
  int yl = (int)y;
  int yh;
  if (yl >= n - 1) {
    yl = yh = n - 1;
    y = (T)yl;
  } else {
    yh = yl + 1;
  }
  const T l = y - (T)yl;
  lo = yl; hi = yh;
  wl = (T)1 - l;          // the weight of cell lo
  wh = l;                 // the weight of cell hi
  return true;
}

// ---- the box head's loss --------------------------------------------------------------------------------------------------
// Box2BoxTransform.get_deltas: src = the RoI, dst = the gt box, weights w[4] = wx wy ww wh
template <class T>
GSR_HD void target_deltas(const T* src, const T* dst, const T* w, T* t) {
  GSR_FP_STRICT
  const T sw = src[2] - src[0], sh = src[3] - src[1];
  const T scx = src[0] + (T)0.5 * sw, scy = src[1] + (T)0.5 * sh;
  const T dw = dst[2] - dst[0], dh = dst[3] - dst[1];
  const T dcx = dst[0] + (T)0.5 * dw, dcy = dst[1] + (T)0.5 * dh;
  t[0] = w[0] * (dcx - scx) / sw;
  t[1] = w[1] * (dcy - scy) / sh;
  t[2] = w[2] * m_log(dw / sw);
  t[3] = w[3] * m_log(dh / sh);
}

// smooth L1 of x and its derivative; beta = 0: |x|, sign(0) = 0
template <class T>
GSR_HD T smooth_l1(T x, T beta, T& g) {
  GSR_FP_STRICT
  const T ax = x < (T)0 ? -x : x;
  const T sg = x > (T)0 ? (T)1 : (x < (T)0 ? (T)-1 : (T)0);
  if (ax < beta) {
    g = x / beta;
    return (T)0.5 * x * x / beta;
  }
  g = sg;
  return ax - (T)0.5 * beta;
}

// ---- the output stage -------------------------------------------------------------------------------------------------------
template <class T>
GSR_HD bool score_better(T pa, int ca, T pb, int cb) { return pa > pb || (pa == pb && ca < cb); }

template <class T>
GSR_HD T clip(T v, T lo, T hi) { return v < lo ? lo : (v > hi ? hi : v); }   // a NaN stays a NaN

// Box2BoxTransform.apply_deltas, before any clip (the proposal stage, gsr_rpn.h, tests this box for finiteness)
template <class T>
GSR_HD void apply_deltas_raw(const T* roi, const T* d, const T* w, T* o) {
  GSR_FP_STRICT
  const T bw = roi[2] - roi[0], bh = roi[3] - roi[1];
  const T cx = roi[0] + (T)0.5 * bw, cy = roi[1] + (T)0.5 * bh;
  const T lim = m_log((T)1000 / (T)16);
  const T dx = d[0] / w[0], dy = d[1] / w[1];
  T dw = d[2] / w[2], dh = d[3] / w[3];
  dw = dw < lim ? dw : (dw == dw ? lim : dw);
  dh = dh < lim ? dh : (dh == dh ? lim : dh);
  const T pcx = dx * bw + cx, pcy = dy * bh + cy;
  const T pw = m_exp(dw) * bw, ph = m_exp(dh) * bh;
  o[0] = pcx - (T)0.5 * pw;
  o[1] = pcy - (T)0.5 * ph;
  o[2] = pcx + (T)0.5 * pw;
  o[3] = pcy + (T)0.5 * ph;
}

template <class T>
GSR_HD void clip_box(T* o, T img_w, T img_h) {
  o[0] = clip<T>(o[0], (T)0, img_w);
  o[1] = clip<T>(o[1], (T)0, img_h);
  o[2] = clip<T>(o[2], (T)0, img_w);
  o[3] = clip<T>(o[3], (T)0, img_h);
}

// ... and a clip to the image
template <class T>
GSR_HD void apply_deltas(const T* roi, const T* d, const T* w, T img_w, T img_h, T* o) {
  apply_deltas_raw<T>(roi, d, w, o);
  clip_box<T>(o, img_w, img_h);
}

}  // namespace gsr_rcnn
