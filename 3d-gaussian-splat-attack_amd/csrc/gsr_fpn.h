// gsr_fpn.h -- the FPN RoI pooler's level assignment: the canonical-size quotient of a RoI and the level it is pooled
// from (include/gsraster.h, GsrFpnSpec).  The pooling itself is gsr_rcnn.h's RoIAlign arithmetic, not written again.
//
// Pure scalar functions, usable from the HIP kernels (gsr_fpn.hip.h, T = float) and from a host C++ harness (g++;
// tests/host_math/fpn_host.cpp, T = float and T = double).  Every function that rounds starts with GSR_FP_STRICT (the host
// build adds -ffp-contract=off): each product, sum and quotient is rounded once, in source order, on both sides.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gsr_math.h"   // GSR_HD, GSR_FP_STRICT
#include "gsr_rcnn.h"   // roi_finite

namespace gsr_fpn {

constexpr int MAX_LEVELS = 5;
constexpr int MAX_SAMPLE = gsr_rcnn::MAX_SAMPLE;   // RoIs per image

// What the kernels take by value (GsrFpnSpec, field for field).
struct Spec {
  int32_t B, S, Cf, PH, PW;
  int32_t sampling_ratio;
  int32_t nl;
  int32_t Hf[MAX_LEVELS], Wf[MAX_LEVELS];
  float scale[MAX_LEVELS];
  float thr[MAX_LEVELS];      // entry 0 unused
  float canonical_size;
};

GSR_HD float m_sqrt(float v) { return sqrtf(v); }
GSR_HD double m_sqrt(double v) { return sqrt(v); }

// Detectron2's assign_boxes_to_levels, up to the logarithm: sqrt(area) / canonical_size + 1e-8.  A negative area gives a NaN.
template <class T>
GSR_HD T level_quotient(const T* r, T canonical_size) {
  GSR_FP_STRICT
  const T area = (r[2] - r[0]) * (r[3] - r[1]);
  return m_sqrt(area) / canonical_size + (T)1e-8;
}

// the number of l in 1 .. nl - 1 with q >= thr[l]: floor(canonical_level + log2(q)) clamped to the levels, without the
// logarithm.  A NaN passes no threshold: level 0.  thr has MAX_LEVELS entries (a loop of fixed length: the kernels keep
// the table in their argument registers); those from nl on are read and not used.
template <class T>
GSR_HD int level_of(T q, const T* thr, int nl) {
  int level = 0;
#pragma unroll
  for (int l = 1; l < MAX_LEVELS; ++l) level += (l < nl && q >= thr[l]) ? 1 : 0;
  return level;
}

// the level of row s of an image with n live rows: -1 for a row at or beyond n and for a row that is not finite
template <class T>
GSR_HD int roi_level(const T* r, int s, int n, const T* thr, int nl, T canonical_size) {
  if (s >= n || !gsr_rcnn::roi_finite<T>(r)) return -1;
  return level_of<T>(level_quotient<T>(r, canonical_size), thr, nl);
}

}  // namespace gsr_fpn
