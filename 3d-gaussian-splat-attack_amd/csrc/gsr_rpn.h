// gsr_rpn.h -- the RPN proposal stage: the order of the objectness logits, the anchor of a candidate, its decode and
// validity, and the suppression test of the NMS walk (include/gsraster.h, GsrRpnSpec).
//
// Pure scalar functions, usable from the HIP kernels (gsr_rpn.hip.h, T = float) and from a host C++ harness (g++;
// tests/host_math/rpn_host.cpp, T = float and T = double).  Every function that rounds starts with GSR_FP_STRICT (the host
// build adds -ffp-contract=off): each product, sum and quotient is rounded once, in source order, on both sides.
//
// Nothing is written a second time: the order is gsr_detect.h's composite (score descending, then index ascending, -0
// counted as +0), the decode is gsr_rcnn.h's apply_deltas_raw and clip_box, the IoU is gsr_detect.h's (the one gsr_det_nms
// documents) and the suppression test gsr_detect::suppresses with the level in the place of the class.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gsr_detect.h"   // composite, Box, box_area, iou, suppresses
#include "gsr_math.h"     // GSR_HD, GSR_FP_STRICT
#include "gsr_rcnn.h"     // apply_deltas_raw, clip_box, roi_finite

namespace gsr_rpn {

using gsr_detect::Box;
using gsr_detect::box_area;

constexpr int MAX_SLOTS = 16384;   // N: candidate slots per image
constexpr int MAX_POST = 4096;     // post_topk: what the sampler's R + M <= 4096 can take
constexpr uint64_t NO_KEY = ~0ull; // sorts behind every candidate

// What the kernels take by value (GsrRpnSpec, field for field).
struct Spec {
  int32_t B, A, Hf, Wf;
  int32_t stride;
  float shift0;
  float img_w, img_h, min_size;
  int32_t pre_topk, level, cand_offset;
  int32_t N, post_topk;
  float iou_thr;
  uint32_t flags;
};

// the slots a level fills: min(pre_topk, A * Hf * Wf)
GSR_HD long long level_slots(const Spec& sp) {
  const long long n_in = (long long)sp.A * (long long)sp.Hf * (long long)sp.Wf;
  return n_in < (long long)sp.pre_topk ? n_in : (long long)sp.pre_topk;
}

GSR_HD bool is_nan(float v) { return v != v; }

// The order of two candidates is the order of their keys, ascending: logit descending (by float comparison, -0 = +0), then
// index ascending.  No two indices share a key.  A NaN has no key: the caller leaves it out.
GSR_HD uint64_t order_key(float logit, int index) { return gsr_detect::composite(logit, index); }

// candidate index i = (y * Wf + x) * A + a
GSR_HD void split_index(int i, int A, int Wf, int& a, int& x, int& y) {
  a = i % A;
  const int p = i / A;
  y = p / Wf;
  x = p - y * Wf;
}

// DefaultAnchorGenerator: the cell anchor moved to its cell's shift
template <class T>
GSR_HD void anchor_at(const T* cell, int x, int y, int stride, T shift0, T* a) {
  GSR_FP_STRICT
  const T sx = (T)(x * stride) + shift0, sy = (T)(y * stride) + shift0;
  a[0] = cell[0] + sx;
  a[1] = cell[1] + sy;
  a[2] = cell[2] + sx;
  a[3] = cell[3] + sy;
}

// Box2BoxTransform(weights 1, 1, 1, 1).apply_deltas, dropped where an unclipped coordinate is not finite, clipped to the
// frame, dropped unless both sides exceed min_size.  -> the candidate stays; box: the clipped box (defined only then)
template <class T>
GSR_HD bool decode_candidate(const T* anchor, const T* d, T img_w, T img_h, T min_size, T* box) {
  GSR_FP_STRICT
  const T w[4] = {(T)1, (T)1, (T)1, (T)1};
  gsr_rcnn::apply_deltas_raw<T>(anchor, d, w, box);
  if (!gsr_rcnn::roi_finite<T>(box)) return false;
  gsr_rcnn::clip_box<T>(box, img_w, img_h);
  const T bw = box[2] - box[0], bh = box[3] - box[1];
  return bw > min_size && bh > min_size;
}

// `later` is suppressed by the kept box `kept`: the same level and iou > iou_thr (false for a NaN IoU)
GSR_HD bool suppresses(const Box& kept, float area_kept, int level_kept, const Box& later, float area_later, int level_later,
                       float iou_thr) {
  return gsr_detect::suppresses(kept, area_kept, level_kept, later, area_later, level_later, iou_thr, false);
}

}  // namespace gsr_rpn
