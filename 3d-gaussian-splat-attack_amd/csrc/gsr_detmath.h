// gsr_detmath.h -- the scalar helpers the detector stages share: the loss stage (gsr_detloss.h), the set-prediction stage
// (gsr_setdet.h) and the two-stage stage (gsr_rcnn.h) pull these names into their own namespaces with `using`.
//
// Pure scalar functions, usable from the HIP kernels (T = float) and from the host C++ harnesses (g++, T = float and
// T = double).  Every function that rounds starts with GSR_FP_STRICT (the host build adds -ffp-contract=off).
//
// What is NOT here, on purpose: the four IoU-family functions -- gsr_detect::iou, gsr_rcnn::pair_iou, gsr_setdet::giou and
// gsr_dloss::ciou.  They look alike and are not: each follows its own reference and rounds as that reference does (an
// epsilon in the union or none, 0 or NaN for an empty box, the area passed in or computed, a clamp on the enclosing box or
// none).  Merging them would change results; leave them where they are.
#pragma once
#include <math.h>

#include "gsr_math.h"     // GSR_HD, GSR_FP_STRICT

namespace gsr_detmath {

GSR_HD float m_exp(float x) { return expf(x); }
GSR_HD double m_exp(double x) { return exp(x); }
GSR_HD float m_log(float x) { return logf(x); }
GSR_HD double m_log(double x) { return log(x); }

// d max(a, b) / d a and d min(a, b) / d a, a tie shared in halves (torch.maximum / torch.minimum)
template <class T>
GSR_HD T dmax_da(T a, T b) { return a > b ? (T)1 : (a == b ? (T)0.5 : (T)0); }
template <class T>
GSR_HD T dmin_da(T a, T b) { return a < b ? (T)1 : (a == b ? (T)0.5 : (T)0); }

// a gt row is present iff its class is one of the head's
GSR_HD bool present(int cls, int C) { return cls >= 0 && cls < C; }

template <class T>
GSR_HD bool is_finite(T v) { return v - v == (T)0; }

// ---- softmax statistics of one row of n logits: the maximum and sum exp(x - max), added in index order
template <class T>
GSR_HD void softmax_stats(const T* x, int n, T& mx, T& sum) {
  GSR_FP_STRICT
  T m = x[0];
  for (int k = 1; k < n; ++k) m = x[k] > m ? x[k] : m;
  T s = (T)0;
  for (int k = 0; k < n; ++k) s = s + m_exp(x[k] - m);
  mx = m;
  sum = s;
}

template <class T>
GSR_HD T softmax_prob(T x, T mx, T sum) {
  GSR_FP_STRICT
  return m_exp(x - mx) / sum;
}

template <class T>
GSR_HD T log_softmax(T x, T mx, T sum) {
  GSR_FP_STRICT
  return (x - mx) - m_log(sum);
}

}  // namespace gsr_detmath
