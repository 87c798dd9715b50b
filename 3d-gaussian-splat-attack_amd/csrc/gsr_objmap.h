// gsr_objmap.h -- per-pixel arithmetic of the object-map classifier (include/gsraster.h, GsrObjMapSpec): the 1x1 convolution
// Conv2d(16, K, 1) over render()'s 16-channel object map, fused with what consumes its logits -- the arg-max id, its softmax
// probability, the cross entropy against a target id map and that loss's gradient with respect to the map -- so that no
// logit is ever stored.
//
// Pure scalar functions, usable from the HIP kernels (gsr_objmap.hip.h) and from a host C++ harness (g++;
// tests/host_math/objmap_host.cpp).  All arithmetic is float32 but for the running sum of pass_sum.  A logit is one chain
// of fmaf in channel order, which is correctly rounded on both sides: the logits, and with them the ids, the per-class
// statistics and the painted image, are the same bits from the kernels and from plain loops over these functions.  expf
// and logf are each side's own, so the confidence, the loss and the gradient agree to a few ulp, not to the bit.
//
// Deviations from the torch expression (torch.argmax(Conv2d(16, K, 1)(map), 0), F.cross_entropy):
//   * a NaN logit is never the maximum (torch.argmax lets a NaN win); a pixel none of whose logits compares greater than
//     -inf -- all NaN or -inf -- gets id -1, confidence 0, and takes no part in the loss;
//   * a NaN logit beside a finite maximum still reaches the softmax sum: that pixel's confidence, loss term and gradient
//     are NaN, as torch's would be;
//   * the classifier is frozen: the gradient is taken with respect to the map alone.  Gradients to W and b are out of scope.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gsr_detmath.h"   // m_exp, m_log; the softmax_stats order: the maximum first, then sum exp(x - max) in index order
#include "gsr_math.h"      // GSR_HD, GSR_FP_STRICT

namespace gsr_om {   // (gsr_objmap is the C entry point's name)

using gsr_detmath::m_exp;
using gsr_detmath::m_log;

constexpr int CH = 16;                 // object channels: fixed (NUM_OBJECTS)
constexpr int MAX_CLASSES = 1024;      // = GROUP_MAX_CLASSES
constexpr int OM_THREADS = 256;        // one workgroup's pixels, a lane each
constexpr int INIT_BLOCKS = 64;        // workgroups per image of the valid-pixel count
constexpr uint32_t FLAG_LOSS = 1u;     // GSR_OBJMAP_LOSS

// GsrObjMapSpec, field for field
struct Spec {
  int32_t B, H, W, K;
  uint32_t flags;
};

// l_c = b[c] + sum_k W[c,k] f[k], k ascending, one fmaf per term
GSR_HD float logit(const float* w_row, float bias, const float f[CH]) {
  float l = bias;
#pragma unroll
  for (int k = 0; k < CH; ++k) l = fmaf(w_row[k], f[k], l);
  return l;
}

// pass 1: the first maximum over c = 0..K-1 under l > best, from -inf.  id = -1 when nothing compares greater.
GSR_HD void pass_max(const float* W, const float* b, int K, const float f[CH], float& m, int& id) {
  float best = -INFINITY;
  int arg = -1;
  for (int c = 0; c < K; ++c) {
    const float l = logit(W + (size_t)c * CH, b[c], f);
    if (l > best) { best = l; arg = c; }
  }
  m = best;
  id = arg;
}

// some logit compares greater than -inf: the pixel will get an id (what pass_max decides, without the maximum)
GSR_HD bool alive(const float* W, const float* b, int K, const float f[CH]) {
  for (int c = 0; c < K; ++c)
    if (logit(W + (size_t)c * CH, b[c], f) > -INFINITY) return true;
  return false;
}

// pass 2: sum_c exp(l_c - m) in class order, and the target's logit picked up on the way (untouched for t outside 0..K-1).
// Every term is a float32 exp; the running sum is carried in double and rounded to float32 once at the end: a float32
// running sum of 1024 terms of one size is off by up to 1e-6 of itself, several times the float32 oracle's distance.
GSR_HD float pass_sum(const float* W, const float* b, int K, const float f[CH], float m, int t, float& l_t) {
  GSR_FP_STRICT
  double s = 0.0;
  for (int c = 0; c < K; ++c) {
    const float l = logit(W + (size_t)c * CH, b[c], f);
    if (c == t) l_t = l;
    s = s + (double)m_exp(l - m);
  }
  return (float)s;
}

// the arg-max's softmax probability: exp(m - m) / sum
GSR_HD float confidence(int id, float sum) {
  GSR_FP_STRICT
  return id >= 0 ? 1.0f / sum : 0.0f;
}

// a pixel counts towards the loss iff it has an id and its target names a class
GSR_HD bool counted(int id, int t, int K) { return id >= 0 && t >= 0 && t < K; }

// -log softmax(l)[t]
GSR_HD float ce_term(float m, float l_t, float sum) {
  GSR_FP_STRICT
  return (m - l_t) + m_log(sum);
}

// pass 3: g_k = scale * sum_c W[c,k] (p_c - [c == t]), c ascending, one fmaf per term; p_c = exp(l_c - m) * inv_sum.
// scale = 1 / valid_b: the gradient of the image's mean.
GSR_HD void pass_grad(const float* W, const float* b, int K, const float f[CH], float m, float inv_sum, int t, float scale, float g[CH]) {
  GSR_FP_STRICT
#pragma unroll
  for (int k = 0; k < CH; ++k) g[k] = 0.0f;
  for (int c = 0; c < K; ++c) {
    const float* w = W + (size_t)c * CH;
    const float p = m_exp(logit(w, b[c], f) - m) * inv_sum;
    const float d = p - (c == t ? 1.0f : 0.0f);
#pragma unroll
    for (int k = 0; k < CH; ++k) g[k] = fmaf(w[k], d, g[k]);
  }
#pragma unroll
  for (int k = 0; k < CH; ++k) g[k] = g[k] * scale;
}

GSR_HD float inv_valid(int32_t valid) {
  GSR_FP_STRICT
  return valid > 0 ? 1.0f / (float)valid : 0.0f;
}

// the image's mean from the sum of its terms; 0 without a counted pixel
GSR_HD float mean_ce(float sum, int32_t valid) {
  GSR_FP_STRICT
  return valid > 0 ? sum / (float)valid : 0.0f;
}

GSR_HD int blocks_of(int H, int W) { return (int)(((long long)H * W + OM_THREADS - 1) / OM_THREADS); }

}  // namespace gsr_om
