// gsr_detect.h -- the detector's output stage: per-anchor score and class, the candidate order, box decode, box IoU,
// the affine back to the render frame and the success verdict (include/gsraster.h, GsrDetSpec).
//
// Pure scalar functions, usable from the HIP kernels (gsr_detect.hip.h) and from a host C++ harness (g++;
// tests/host_math/detect_host.cpp): the host build is checked against a numpy oracle written from the contract, the
// kernels against the host build bit for bit.  Every function that rounds starts with GSR_FP_STRICT (the host build
// adds -ffp-contract=off): each product, sum and quotient is rounded once, in source order, on both sides.
//
// Order of the candidates of one image: score descending, then anchor index ascending.  It is carried by one 64-bit
// composite per candidate, composite(score, anchor) = (~key(score)) << 32 | anchor, sorted ASCENDING; key() is the
// monotone uint32 image of a float (-0 counted as +0), so that the composite compares as the pair does and no two
// candidates share one: whatever produced the list (atomics, any launch geometry), the sorted list is the same.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gsr_math.h"   // GSR_HD, GSR_FP_STRICT

namespace gsr_detect {

constexpr int MAX_CAND = 4096;             // candidates that enter the NMS walk, per image
constexpr uint32_t CLASS_AGNOSTIC = 1u;    // = GSR_DET_CLASS_AGNOSTIC

// What the kernels take by value.
struct Spec {
  int32_t B, A, C;
  int32_t layout, has_obj, box_format;
  float conf_thr, iou_thr;
  int32_t max_candidates, max_det;
  uint32_t flags;
  float ox, oy, sx, sy;
};

struct Box {
  float x1, y1, x2, y2;
};

GSR_HD int channels(const Spec& sp) { return 4 + sp.has_obj + sp.C; }

// element (b, a, channel k) of pred
GSR_HD size_t pred_index(const Spec& sp, int b, int a, int k) {
  const size_t K = (size_t)channels(sp), A = (size_t)sp.A;
  return sp.layout == 0 ? ((size_t)b * A + (size_t)a) * K + (size_t)k : ((size_t)b * K + (size_t)k) * A + (size_t)a;
}

GSR_HD uint32_t float_bits(float f) {
  union { float f; uint32_t u; } v;
  v.f = f;
  return v.u;
}

GSR_HD float neg_inf() {
  union { float f; uint32_t u; } v;
  v.u = 0xff800000u;
  return v.f;
}

// larger float -> larger key; -0 and +0 share one key (they compare equal)
GSR_HD uint32_t score_key(float s) {
  uint32_t u = float_bits(s);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

GSR_HD uint64_t composite(float score, int anchor) {
  return ((uint64_t)(~score_key(score)) << 32) | (uint64_t)(uint32_t)anchor;
}

GSR_HD float class_score(float obj, float cls, int has_obj) {
  GSR_FP_STRICT
  return has_obj ? obj * cls : cls;
}

// The running best of an anchor over its classes: start at (-inf, class 0); better() is a strict total preference
// (score, then the lower class), so the result does not depend on the order the classes are visited in, and a NaN class
// score is never preferred.
GSR_HD bool better(float s, int c, float best_s, int best_c) { return s > best_s || (s == best_s && c < best_c); }

// One anchor, sequentially: its best class and that class's score.  cls: the first class channel, `stride` floats apart.
GSR_HD void anchor_best(const float* cls, size_t stride, int C, float obj, int has_obj, float& score, int& best) {
  float bs = neg_inf();
  int bc = 0;
  for (int c = 0; c < C; ++c) {
    const float s = class_score(obj, cls[(size_t)c * stride], has_obj);
    if (better(s, c, bs, bc)) { bs = s; bc = c; }
  }
  score = bs;
  best = bc;
}

GSR_HD bool is_candidate(float score, float conf_thr) { return score > conf_thr; }   // false for NaN

GSR_HD Box decode_box(float a, float b, float c, float d, int box_format) {
  GSR_FP_STRICT
  Box r;
  if (box_format == 0) {
    const float hw = c * 0.5f, hh = d * 0.5f;
    r.x1 = a - hw; r.y1 = b - hh; r.x2 = a + hw; r.y2 = b + hh;
  } else {
    r.x1 = a; r.y1 = b; r.x2 = c; r.y2 = d;
  }
  return r;
}

GSR_HD Box load_box(const Spec& sp, const float* pred, int b, int a) {
  return decode_box(pred[pred_index(sp, b, a, 0)], pred[pred_index(sp, b, a, 1)], pred[pred_index(sp, b, a, 2)],
                    pred[pred_index(sp, b, a, 3)], sp.box_format);
}

GSR_HD float box_area(const Box& a) {
  GSR_FP_STRICT
  const float w = a.x2 - a.x1, h = a.y2 - a.y1;
  return w * h;
}

// torchvision's box_iou, operation by operation.  0 / 0 (two empty boxes) is NaN.
GSR_HD float iou(const Box& a, float area_a, const Box& b, float area_b) {
  GSR_FP_STRICT
  const float lx = a.x1 > b.x1 ? a.x1 : b.x1, ly = a.y1 > b.y1 ? a.y1 : b.y1;
  const float rx = a.x2 < b.x2 ? a.x2 : b.x2, ry = a.y2 < b.y2 ? a.y2 : b.y2;
  float iw = rx - lx, ih = ry - ly;
  iw = iw > 0.0f ? iw : 0.0f;
  ih = ih > 0.0f ? ih : 0.0f;
  const float inter = iw * ih;
  const float sum = area_a + area_b;
  const float uni = sum - inter;
  return inter / uni;
}

// `later` is suppressed by the kept box `kept` (false for a NaN IoU)
GSR_HD bool suppresses(const Box& kept, float area_kept, int cls_kept, const Box& later, float area_later, int cls_later,
                       float iou_thr, bool agnostic) {
  if (!agnostic && cls_kept != cls_later) return false;
  return iou(kept, area_kept, later, area_later) > iou_thr;
}

// back to the render frame, after NMS
GSR_HD Box to_render_frame(const Box& a, float ox, float oy, float sx, float sy) {
  GSR_FP_STRICT
  Box r;
  r.x1 = (a.x1 - ox) * sx; r.y1 = (a.y1 - oy) * sy; r.x2 = (a.x2 - ox) * sx; r.y2 = (a.y2 - oy) * sy;
  return r;
}

GSR_HD bool gt_present(const float* gt) {
  return gt && gt[0] == gt[0] && gt[1] == gt[1] && gt[2] == gt[2] && gt[3] == gt[3];
}

// IoU(det row, gt) for the verdict: a NaN counts as 0
GSR_HD float verdict_iou(const float* det, const Box& g, float area_g) {
  Box d;
  d.x1 = det[0]; d.y1 = det[1]; d.x2 = det[2]; d.y2 = det[3];
  const float v = iou(d, box_area(d), g, area_g);
  return v == v ? v : 0.0f;
}

// The verdict's bits from what the rows gave.  has_best: a gt box and at least one row (best_iou / best_cls are the
// first maximum's); otherwise any_target / any_untarget over the kept classes (both false with no rows).
GSR_HD int32_t verdict_bits(bool has_best, float best_iou, int best_cls, bool any_target, bool any_untarget, int n,
                            int target, int untarget, int is_targeted, float iou_match) {
  bool target_exists, untarget_absent;
  if (n <= 0) {
    target_exists = false;
    untarget_absent = true;
  } else if (has_best) {
    const bool match = best_iou > iou_match;
    target_exists = match && best_cls == target;
    untarget_absent = !(match && best_cls == untarget);
  } else {
    target_exists = any_target;
    untarget_absent = !any_untarget;
  }
  const bool ok = is_targeted ? (target_exists && (untarget < 0 || untarget_absent)) : untarget_absent;
  return (ok ? 1 : 0) | (target_exists ? 2 : 0) | (untarget_absent ? 4 : 0);
}

}  // namespace gsr_detect
