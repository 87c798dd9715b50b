// gsr_imgloss.h -- per-pixel arithmetic of the fused image losses (include/gsraster.h, GsrImgLossSpec): L1, L2 and SSIM
// of an image against a reference image, and the gradient with respect to the image.
//
// Pure scalar functions, usable from the HIP kernels (gsr_imgloss.hip.h, T = float) and from a host C++ harness (g++;
// tests/host_math/imgloss_host.cpp).  Every function that rounds starts with GSR_FP_STRICT (the host build adds
// -ffp-contract=off): each product, sum and quotient is rounded once, in source order, on both sides, so that the SSIM map
// and the gradient are the same bits from the kernels and from plain loops over these functions.
//
// The window is separable: rows first (row_stats / win11 along x), then columns (win11 along y), zero padding of HALO.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gsr_math.h"   // GSR_HD, GSR_FP_STRICT

namespace gsr_il {   // (gsr_imgloss is the C entry point's name)

constexpr int WIN = 11, HALO = WIN / 2;
constexpr int IMGLOSS_TH = 16, IMGLOSS_TW = 32;   // one workgroup's tile of one (image, channel) plane: a thread per pixel
constexpr int MAX_CHANNELS = 4;
constexpr uint32_t FLAG_CLAMP01 = 1u, FLAG_NO_GRAD = 2u;   // GSR_IMGLOSS_CLAMP01, GSR_IMGLOSS_NO_GRAD

// exp(-(k - 5)^2 / 4.5) as float32, divided by their float32 sum: the eleven numbers the reference's gaussian(11, 1.5) holds
#define GSR_IMGLOSS_TAPS                                                                                                 \
  { 0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f, 0x1.b43c3ep-3f,      \
    0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f }

// GsrImgLossSpec, field for field
struct Spec {
  int32_t B, C, H, W;
  float w_l1, w_l2, w_ssim;
  uint32_t flags;
};

constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

// sum_k tap[k] * v[k * stride], k ascending: the one order both passes of both kernels use
template <class T>
GSR_HD T win11(const T* v, int stride) {
  GSR_FP_STRICT
  const float w[WIN] = GSR_IMGLOSS_TAPS;
  T acc = (T)w[0] * v[0];
#pragma unroll
  for (int k = 1; k < WIN; ++k) acc = acc + (T)w[k] * v[(ptrdiff_t)k * stride];
  return acc;
}

// the row pass of the forward: from eleven neighbours x[0..10], y[0..10] of a row (zeros beyond the image) the five window
// sums of x, y, x^2, y^2, xy
template <class T>
GSR_HD void row_stats(const T* x, const T* y, T out[5]) {
  GSR_FP_STRICT
  const float w[WIN] = GSR_IMGLOSS_TAPS;
  T a = (T)w[0] * x[0], b = (T)w[0] * y[0], c = (T)w[0] * (x[0] * x[0]), d = (T)w[0] * (y[0] * y[0]), e = (T)w[0] * (x[0] * y[0]);
#pragma unroll
  for (int k = 1; k < WIN; ++k) {
    const T wk = (T)w[k], xv = x[k], yv = y[k];
    a = a + wk * xv;
    b = b + wk * yv;
    c = c + wk * (xv * xv);
    d = d + wk * (yv * yv);
    e = e + wk * (xv * yv);
  }
  out[0] = a; out[1] = b; out[2] = c; out[3] = d; out[4] = e;
}

// The reference's _ssim at one pixel from mu1 = win * x, mu2 = win * y, e11 = win * x^2, e22 = win * y^2, e12 = win * xy, and
// the map's derivatives with respect to mu1 (total: the paths through sigma1^2 = e11 - mu1^2 and sigma12 = e12 - mu1 mu2
// included), e11 and e12.
template <class T>
GSR_HD T ssim_point(T mu1, T mu2, T e11, T e22, T e12, T& d_mu1, T& d_e11, T& d_e12) {
  GSR_FP_STRICT
  const T C1 = (T)SSIM_C1, C2 = (T)SSIM_C2;
  const T mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
  const T s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
  const T a1 = (T)2 * mu12 + C1, a2 = (T)2 * s12 + C2;
  const T b1 = mu1_sq + mu2_sq + C1, b2 = s1 + s2 + C2;
  const T den = b1 * b2;
  const T map = (a1 * a2) / den;
  d_e11 = -(map / b2);
  d_e12 = ((T)2 * a1) / den;
  d_mu1 = ((T)2 * mu2) * ((a2 - a1) / den) + ((T)2 * mu1) * (map / b2 - map / b1);
  return map;
}

// torch.clamp(v, 0, 1) (a NaN stays a NaN) and its inclusive mask (gsr_image_resample's: a NaN gives 0)
template <class T>
GSR_HD T clamp01(T v) { return v < (T)0 ? (T)0 : (v > (T)1 ? (T)1 : v); }
template <class T>
GSR_HD T clamp_mask(T v) { return (v >= (T)0 && v <= (T)1) ? (T)1 : (T)0; }

// d = x - y: what L1 sums the magnitude and L2 the square of
template <class T>
GSR_HD T diff(T x, T y) {
  GSR_FP_STRICT
  return x - y;
}
template <class T>
GSR_HD T sq(T d) {
  GSR_FP_STRICT
  return d * d;
}
template <class T>
GSR_HD T sign0(T d) { return d > (T)0 ? (T)1 : (d < (T)0 ? (T)-1 : (d == (T)0 ? (T)0 : d)); }   // sign(0) = 0; a NaN stays

// d loss_b / d x(p): x, y the (clamped) pixel values; gm, g11, g12 the window sums of the three derivative maps at p; inv_n =
// 1 / (C H W); mask: 1, or the clamp's mask of the pixel as given.
template <class T>
GSR_HD T grad_point(T x, T y, T gm, T g11, T g12, T w_l1, T w_l2, T w_ssim, T inv_n, T mask) {
  GSR_FP_STRICT
  const T d = x - y;
  const T s = gm + ((T)2 * x) * g11 + y * g12;
  const T g = (w_l1 * sign0<T>(d) + w_l2 * ((T)2 * d) - w_ssim * s) * inv_n;
  return mask != (T)0 ? g : (T)0;
}

// terms of one image from its three sums (double: sums of float32 per-tile partials) -> l1, l2, ssim, loss
GSR_HD void finish_terms(double sum_abs, double sum_sq, double sum_map, int64_t n, float w_l1, float w_l2, float w_ssim, float out[4]) {
  GSR_FP_STRICT
  const float l1 = (float)(sum_abs / (double)n), l2 = (float)(sum_sq / (double)n), ss = (float)(sum_map / (double)n);
  out[0] = l1; out[1] = l2; out[2] = ss;
  out[3] = w_l1 * l1 + w_l2 * l2 + w_ssim * (1.0f - ss);
}

GSR_HD int tiles_of(int H, int W) { return ((H + IMGLOSS_TH - 1) / IMGLOSS_TH) * ((W + IMGLOSS_TW - 1) / IMGLOSS_TW); }

}  // namespace gsr_il
