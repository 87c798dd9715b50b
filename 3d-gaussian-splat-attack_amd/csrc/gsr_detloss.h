// gsr_detloss.h -- the detector's loss stage: the anchor-free YOLO detection loss (task-aligned assigner, BCE on the class
// logits, CIoU on the decoded boxes, distribution focal loss on the 4 x 16 distance bins) and its gradient with respect
// to the head's raw training output (include/gsraster.h, GsrDetLossSpec).
//
// Pure scalar functions with a hand-written backward, usable from the HIP kernels (gsr_detloss.hip.h, T = float) and from
// a host C++ harness (g++; tests/host_math/detloss_host.cpp, T = float and T = double: the double build is what the
// hand-written backward is checked against by finite differences of its own forward).  Every function that rounds starts
// with GSR_FP_STRICT (the host build adds -ffp-contract=off).
//
// The order of a row's candidates (metric descending, then anchor index ascending) is gsr_detect.h's composite of
// (score, anchor): no two candidates share one, so the first k are the same whatever walks the list.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gsr_detect.h"   // score_key, composite
#include "gsr_detmath.h"  // m_exp, m_log, dmax_da, dmin_da, present
#include "gsr_math.h"     // GSR_HD, GSR_FP_STRICT

namespace gsr_dloss {

using gsr_detmath::dmax_da;
using gsr_detmath::dmin_da;
using gsr_detmath::m_exp;
using gsr_detmath::m_log;
using gsr_detmath::present;

constexpr int MAX_LEVELS = 5;
constexpr int MAX_ROWS = 32;     // gt rows per image
constexpr int MAX_TOPK = 16;
constexpr int REG_MAX = 16;      // bins per side
constexpr int BOX_CH = 4 * REG_MAX;

// What the kernels take by value.  start[i]: the first anchor of level i.
struct Spec {
  int32_t B, A, C, M, nl;
  int32_t h[MAX_LEVELS], w[MAX_LEVELS], start[MAX_LEVELS];
  float stride[MAX_LEVELS];
  int32_t topk;
  float alpha, beta, w_box, w_cls, w_dfl;
};

template <class T>
struct Box {
  T x1, y1, x2, y2;
};

GSR_HD float m_log1p(float x) { return log1pf(x); }
GSR_HD double m_log1p(double x) { return log1p(x); }
GSR_HD float m_atan(float x) { return atanf(x); }
GSR_HD double m_atan(double x) { return atan(x); }
GSR_HD float m_pow(float x, float y) { return powf(x, y); }
GSR_HD double m_pow(double x, double y) { return pow(x, y); }
GSR_HD float m_floor(float x) { return floorf(x); }
GSR_HD double m_floor(double x) { return floor(x); }

GSR_HD int channels(const Spec& sp) { return BOX_CH + sp.C; }

// anchor a -> its grid point (x + 0.5, y + 0.5) and the stride of its level (a in 0 .. A-1)
GSR_HD void anchor_point(const Spec& sp, int a, float& gx, float& gy, float& stride) {
  int i = 0;
  for (int l = 1; l < sp.nl; ++l)
    if (a >= sp.start[l]) i = l;
  const int local = a - sp.start[i];
  const int y = local / sp.w[i], x = local - y * sp.w[i];
  gx = (float)x + 0.5f;
  gy = (float)y + 0.5f;
  stride = sp.stride[i];
}

// ---- decode: the expectation of a max-subtracted softmax over the 16 bins of one side, `step` elements apart.
// p (may be NULL): the 16 probabilities; lse (may be NULL): log sum exp of the bins.  d d / d bin_k = p_k * (k - d).
template <class T>
GSR_HD T softmax_expect(const T* bins, size_t step, T* p, T* lse) {
  GSR_FP_STRICT
  T m = bins[0];
  for (int k = 1; k < REG_MAX; ++k) {
    const T v = bins[(size_t)k * step];
    m = v > m ? v : m;
  }
  T e[REG_MAX];
  T s = (T)0;
  for (int k = 0; k < REG_MAX; ++k) {
    e[k] = m_exp(bins[(size_t)k * step] - m);
    s = s + e[k];
  }
  T d = (T)0;
  for (int k = 0; k < REG_MAX; ++k) {
    const T pk = e[k] / s;
    if (p) p[k] = pk;
    d = d + (T)k * pk;
  }
  if (lse) *lse = m + m_log(s);
  return d;
}

// ---- CIoU(b1, b2) of the contract; g (may be NULL): d ciou / d (b1.x1, b1.y1, b1.x2, b1.y2) with `a` held constant.
// a_in (may be NULL): the value of `a` to use instead of this point's -- the function of b1 whose derivative g is, for
// the finite-difference test; a_out (may be NULL): where the `a` used goes.
template <class T>
GSR_HD T ciou(const Box<T>& b1, const Box<T>& b2, T* g, const T* a_in = nullptr, T* a_out = nullptr) {
  GSR_FP_STRICT
  const T eps = (T)1e-7;
  const T w1 = b1.x2 - b1.x1, h1 = b1.y2 - b1.y1 + eps;
  const T w2 = b2.x2 - b2.x1, h2 = b2.y2 - b2.y1 + eps;
  const T ix1 = b1.x1 > b2.x1 ? b1.x1 : b2.x1, ix2 = b1.x2 < b2.x2 ? b1.x2 : b2.x2;
  const T iy1 = b1.y1 > b2.y1 ? b1.y1 : b2.y1, iy2 = b1.y2 < b2.y2 ? b1.y2 : b2.y2;
  const T rw = ix2 - ix1, rh = iy2 - iy1;
  const T iw = rw > (T)0 ? rw : (T)0, ih = rh > (T)0 ? rh : (T)0;
  const T inter = iw * ih;
  const T uni = w1 * h1 + w2 * h2 - inter + eps;
  const T iou = inter / uni;
  const T ex1 = b1.x1 < b2.x1 ? b1.x1 : b2.x1, ex2 = b1.x2 > b2.x2 ? b1.x2 : b2.x2;
  const T ey1 = b1.y1 < b2.y1 ? b1.y1 : b2.y1, ey2 = b1.y2 > b2.y2 ? b1.y2 : b2.y2;
  const T cw = ex2 - ex1, ch = ey2 - ey1;
  const T c2 = cw * cw + ch * ch + eps;
  const T dx = b2.x1 + b2.x2 - b1.x1 - b1.x2, dy = b2.y1 + b2.y2 - b1.y1 - b1.y2;
  const T rho2 = (dx * dx + dy * dy) / (T)4;
  const T k = (T)0.40528473456935108577551785283891;   // 4 / pi^2
  const T da = m_atan(w2 / h2) - m_atan(w1 / h1);
  const T v = k * (da * da);
  const T al = a_in ? *a_in : v / (v - iou + ((T)1 + eps));
  if (a_out) *a_out = al;
  const T pen = rho2 / c2;
  if (g) {
    // the clamp passes its gradient where its argument is >= 0 (torch.clamp)
    const T pw = rw >= (T)0 ? ih : (T)0, ph = rh >= (T)0 ? iw : (T)0;   // d inter / d rw, d inter / d rh
    const T di[4] = {-pw * dmax_da(b1.x1, b2.x1), -ph * dmax_da(b1.y1, b2.y1), pw * dmin_da(b1.x2, b2.x2),
                     ph * dmin_da(b1.y2, b2.y2)};
    const T da1[4] = {-h1, -w1, h1, w1};                                 // d (w1 * h1)
    const T dcw[4] = {-dmin_da(b1.x1, b2.x1), (T)0, dmax_da(b1.x2, b2.x2), (T)0};
    const T dch[4] = {(T)0, -dmin_da(b1.y1, b2.y1), (T)0, dmax_da(b1.y2, b2.y2)};
    const T drho[4] = {-dx / (T)2, -dy / (T)2, -dx / (T)2, -dy / (T)2};
    const T q = w1 * w1 + h1 * h1;
    const T dv_dw = -(T)2 * k * da * (h1 / q), dv_dh = (T)2 * k * da * (w1 / q);
    const T dv[4] = {-dv_dw, -dv_dh, dv_dw, dv_dh};
    for (int i = 0; i < 4; ++i) {
      const T duni = da1[i] - di[i];
      const T diou = (di[i] - iou * duni) / uni;
      const T dc2 = (T)2 * cw * dcw[i] + (T)2 * ch * dch[i];
      const T dpen = (drho[i] - pen * dc2) / c2;
      g[i] = diou - dpen - al * dv[i];
    }
  }
  return iou - (pen + v * al);
}

// ---- DFL: the clamped target distance -> left bin and the two weights
template <class T>
GSR_HD void dfl_target(T dist, int& tl, T& wl, T& wr) {
  GSR_FP_STRICT
  T t = dist > (T)0 ? dist : (T)0;                   // a NaN distance counts as 0: the bins stay in range
  t = t < (T)14.99 ? t : (T)14.99;
  tl = (int)m_floor(t);
  wl = (T)(tl + 1) - t;
  wr = (T)1 - wl;
}

// ---- stable BCE with logits; g: d / d x = sigmoid(x) - t
template <class T>
GSR_HD T bce(T x, T t, T* g) {
  GSR_FP_STRICT
  const T ax = x < (T)0 ? -x : x;
  const T e = m_exp(-ax);
  const T pos = x > (T)0 ? x : (T)0;
  if (g) *g = (x >= (T)0 ? (T)1 / ((T)1 + e) : e / ((T)1 + e)) - t;
  return pos - x * t + m_log1p(e);
}

template <class T>
GSR_HD T sigmoid(T x) {
  GSR_FP_STRICT
  const T ax = x < (T)0 ? -x : x;
  const T e = m_exp(-ax);
  return x >= (T)0 ? (T)1 / ((T)1 + e) : e / ((T)1 + e);
}

// ---- assignment
// gt: x1 y1 x2 y2 in pixels; (px, py): the anchor's pixel point
template <class T>
GSR_HD bool is_candidate(T px, T py, const T* gt) {
  GSR_FP_STRICT
  T m = px - gt[0];
  const T b = py - gt[1], c = gt[2] - px, d = gt[3] - py;
  m = b < m ? b : m;
  m = c < m ? c : m;
  m = d < m ? d : m;
  return m > (T)1e-9;                                // false for NaN
}

template <class T>
GSR_HD bool anchor_is_candidate(const Spec& sp, int a, const T* gt) {
  GSR_FP_STRICT
  float gx, gy, st;
  anchor_point(sp, a, gx, gy, st);
  return is_candidate((T)gx * (T)st, (T)gy * (T)st, gt);
}

// the anchor's predicted box in grid units
template <class T>
GSR_HD Box<T> decode_grid(const T* bins, size_t step, T gx, T gy) {
  GSR_FP_STRICT
  Box<T> r;
  r.x1 = gx - softmax_expect<T>(bins, step, nullptr, nullptr);
  r.y1 = gy - softmax_expect<T>(bins + (size_t)REG_MAX * step, step, nullptr, nullptr);
  r.x2 = gx + softmax_expect<T>(bins + (size_t)(2 * REG_MAX) * step, step, nullptr, nullptr);
  r.y2 = gy + softmax_expect<T>(bins + (size_t)(3 * REG_MAX) * step, step, nullptr, nullptr);
  return r;
}

// ov and metric of one candidate: gt and the predicted box in pixels, the logit of the row's class
template <class T>
GSR_HD void candidate_metric(const T* gt, const Box<T>& pred_px, T logit, T alpha, T beta, T& ov, T& metric) {
  GSR_FP_STRICT
  Box<T> g;
  g.x1 = gt[0]; g.y1 = gt[1]; g.x2 = gt[2]; g.y2 = gt[3];
  const T c = ciou<T>(g, pred_px, nullptr);
  ov = c > (T)0 ? c : (T)0;                          // a NaN counts as 0
  metric = m_pow(sigmoid(logit), alpha) * m_pow(ov, beta);
}

template <class T>
GSR_HD uint64_t order_composite(T metric, int anchor) { return gsr_detect::composite((float)metric, anchor); }

template <class T>
GSR_HD T target_score(T metric, T row_max_ov, T row_max_metric) {
  GSR_FP_STRICT
  return metric * row_max_ov / (row_max_metric + (T)1e-9);
}

template <class T>
GSR_HD T clamp_tss(T s) { return s > (T)1 ? s : (T)1; }

// ---- one foreground anchor: box_term = 1 - CIoU(pred_grid, gt_grid), dfl_term = 1/4 sum over the sides of the DFL pair.
// bins: the anchor's 64 box channels, `step` apart.  gb (may be NULL): where d total / d bins goes, `gstep` apart, with
// cb = d total / d box_term and cd = d total / d dfl_term.  a_in / a_out: ciou's.
template <class T>
GSR_HD void box_dfl_anchor(const T* bins, size_t step, T gx, T gy, T stride, const T* gt, T cb, T cd, T* gb, size_t gstep,
                           T& box_term, T& dfl_term, const T* a_in = nullptr, T* a_out = nullptr) {
  GSR_FP_STRICT
  T d[4], lse[4];
  for (int s = 0; s < 4; ++s) d[s] = softmax_expect<T>(bins + (size_t)(s * REG_MAX) * step, step, nullptr, &lse[s]);
  Box<T> pb, gg;
  pb.x1 = gx - d[0]; pb.y1 = gy - d[1]; pb.x2 = gx + d[2]; pb.y2 = gy + d[3];
  gg.x1 = gt[0] / stride; gg.y1 = gt[1] / stride; gg.x2 = gt[2] / stride; gg.y2 = gt[3] / stride;
  T g[4] = {(T)0, (T)0, (T)0, (T)0};
  const T c = ciou<T>(pb, gg, gb ? g : nullptr, a_in, a_out);
  box_term = (T)1 - c;
  const T dist[4] = {gx - gg.x1, gy - gg.y1, gg.x2 - gx, gg.y2 - gy};
  // d total / d d_s: box_term falls as ciou rises; x1 = gx - d_l, y1 = gy - d_t, x2 = gx + d_r, y2 = gy + d_b
  const T dd[4] = {cb * g[0], cb * g[1], -(cb * g[2]), -(cb * g[3])};
  const T cq = cd * (T)0.25;
  T acc = (T)0;
  for (int s = 0; s < 4; ++s) {
    int tl;
    T wl, wr;
    dfl_target(dist[s], tl, wl, wr);
    const T* bs = bins + (size_t)(s * REG_MAX) * step;
    acc = acc + ((lse[s] - bs[(size_t)tl * step]) * wl + (lse[s] - bs[(size_t)(tl + 1) * step]) * wr);
    if (gb) {
      T p[REG_MAX];
      softmax_expect<T>(bs, step, p, nullptr);
      for (int k = 0; k < REG_MAX; ++k) {
        const T hot = k == tl ? wl : (k == tl + 1 ? wr : (T)0);
        gb[(size_t)(s * REG_MAX + k) * gstep] = dd[s] * (p[k] * ((T)k - d[s])) + cq * (p[k] - hot);
      }
    }
  }
  dfl_term = acc * (T)0.25;
}

}  // namespace gsr_dloss
