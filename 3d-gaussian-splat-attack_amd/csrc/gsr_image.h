// gsr_image.h -- the image front end between the renders and a detector: bilinear resize into a padded canvas
// (letterbox), optional clamp to [0,1] and per-channel normalisation, and its backward in GATHER form.
//
// Pure scalar float32 functions, usable from the HIP kernels (gsr_image.hip.h) and from a host C++ harness (g++;
// tests/host_math/image_host.cpp), so that the source the kernels run is checked against torch.nn.functional.interpolate
// on the CPU, and the kernels against the host build bit for bit.  Every function that rounds starts with GSR_FP_STRICT
// (the host build adds -ffp-contract=off): each product and sum is rounded once, in source order, on both sides.
//
// Semantics (include/gsraster.h, GsrResample): F.interpolate(mode="bilinear", align_corners=False, size=(rh, rw)),
// per axis with input size `in`, resized size `out` and output index d:
//     scale = (float)in / (float)out
//     src   = scale * (d + 0.5f) - 0.5f;   if (src < 0) src = 0
//     i0    = min((int)src, in - 1);       i1 = i0 + (i0 < in - 1 ? 1 : 0)
//     l1    = clamp(src - (float)i0, 0, 1); l0 = 1 - l1
// value = h0*(w0*a + w1*b) + h1*(w0*c + w1*d), a b from row i0, c d from row i1, a c from column i0, b d from column i1.
//
// Backward: grad_src[y,x] = the sum of ((h*w) * g) over the output pixels that sample (y,x), output rows ascending,
// output columns ascending inside a row, and inside one output pixel the roles (row i0, col i0), (i0, i1), (i1, i0),
// (i1, i1); a role counts only if it names (y,x).  No atomics, no memset: every source pixel is written once, and the
// sum has one order wherever it runs.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gsr_math.h"   // GSR_HD, GSR_FP_STRICT

namespace gsr_image {

constexpr int MAX_C = 4;
constexpr uint32_t CLAMP01 = 1u;    // = GSR_RESAMPLE_CLAMP01

// What the kernels take by value: the sizes, the two scales (computed once, on the host, by axis_scale) and the
// per-channel affine (mean 0 / inv_std 1 with affine == 0: then it is not applied at all).
struct Spec {
  int32_t C, H, W;             // source planes
  int32_t out_h, out_w;        // destination planes
  int32_t rh, rw, top, left;   // the resized image and where it sits in the destination
  float pad_value;
  float sy, sx;                // axis_scale(H, rh), axis_scale(W, rw)
  float mean[MAX_C], inv_std[MAX_C];
  uint32_t flags;
  int32_t affine;
};

struct Tap {
  int i0, i1;
  float l0, l1;
};

inline float axis_scale(int in, int out) { return (float)in / (float)out; }

GSR_HD Tap axis_sample(float scale, int in, int d) {
  GSR_FP_STRICT
  float src = scale * ((float)d + 0.5f) - 0.5f;
  if (src < 0.0f) src = 0.0f;
  Tap t;
  const int i = (int)src;
  t.i0 = i < in - 1 ? i : in - 1;
  t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
  float l1 = src - (float)t.i0;
  l1 = l1 < 0.0f ? 0.0f : l1 > 1.0f ? 1.0f : l1;
  t.l1 = l1;
  t.l0 = 1.0f - l1;
  return t;
}

GSR_HD bool axis_names(const Tap& t, int s) { return t.i0 == s || t.i1 == s; }

// A conservative range [lo, hi] of output indices that can name source index s: the inverse of the src formula at
// s - 1 and s + 1, widened by one on either side (the float evaluation is off by far less than one index for every size
// the entry points accept), clipped to [0, out - 1].  Source indices 0 and 1 start at 0: wherever src is clamped to 0 the
// taps are i0 = 0 and i1 = 1, however far below zero the unclamped coordinate lies (an upscale's first outputs).
GSR_HD void axis_candidates(float scale, int out, int s, int& lo, int& hi) {
  GSR_FP_STRICT
  const float a = ((float)s - 0.5f) / scale - 0.5f;
  const float b = ((float)s + 1.5f) / scale - 0.5f;
  const float top = (float)(out - 1);
  const float fa = a < 0.0f ? 0.0f : a > top ? top : a;
  const float fb = b < 0.0f ? 0.0f : b > top ? top : b;
  lo = (int)fa - 1;        // (int) truncates = floor for fa >= 0
  hi = (int)fb + 2;        // >= ceil(fb) + 1
  if (lo < 0 || s <= 1) lo = 0;
  if (hi > out - 1) hi = out - 1;
}

// The exact range: src is non-decreasing in d (every rounding is monotone), so are i0 and i1, and the indices that name
// s -- i0(d) <= s <= i1(d) -- are contiguous.  The candidates are re-checked with the forward formula from both ends;
// lo > hi: nothing samples s.
GSR_HD void axis_range(float scale, int in, int out, int s, int& lo, int& hi) {
  axis_candidates(scale, out, s, lo, hi);
  while (lo <= hi && !axis_names(axis_sample(scale, in, lo), s)) ++lo;
  while (hi >= lo && !axis_names(axis_sample(scale, in, hi), s)) --hi;
}

GSR_HD float load_src(const float* p, uint32_t flags) {
  const float v = *p;
  return (flags & CLAMP01) ? (v < 0.0f ? 0.0f : v > 1.0f ? 1.0f : v) : v;
}

GSR_HD float bilerp(float h0, float h1, float w0, float w1, float a, float b, float c, float d) {
  GSR_FP_STRICT
  const float r0 = w0 * a + w1 * b;
  const float r1 = w0 * c + w1 * d;
  return h0 * r0 + h1 * r1;
}

GSR_HD float affine(float v, float mean, float inv_std) {
  GSR_FP_STRICT
  return (v - mean) * inv_std;
}

// One destination pixel (oy, ox), every channel: out[c].  src: this image's [C,H,W] planes.
GSR_HD void forward_pixel(const Spec& sp, const float* src, int oy, int ox, float out[MAX_C]) {
  const int ry = oy - sp.top, rx = ox - sp.left;
  if (ry < 0 || ry >= sp.rh || rx < 0 || rx >= sp.rw) {
    for (int c = 0; c < MAX_C; ++c) out[c] = sp.pad_value;
    return;
  }
  const Tap ty = axis_sample(sp.sy, sp.H, ry), tx = axis_sample(sp.sx, sp.W, rx);
  const size_t plane = (size_t)sp.H * (size_t)sp.W;
  const size_t r0 = (size_t)ty.i0 * (size_t)sp.W, r1 = (size_t)ty.i1 * (size_t)sp.W;
  for (int c = 0; c < MAX_C; ++c) {
    if (c >= sp.C) { out[c] = 0.0f; continue; }
    const float* p = src + (size_t)c * plane;
    const float v = bilerp(ty.l0, ty.l1, tx.l0, tx.l1, load_src(p + r0 + tx.i0, sp.flags), load_src(p + r0 + tx.i1, sp.flags),
                           load_src(p + r1 + tx.i0, sp.flags), load_src(p + r1 + tx.i1, sp.flags));
    out[c] = sp.affine ? affine(v, sp.mean[c], sp.inv_std[c]) : v;
  }
}

GSR_HD void add_term(float& acc, float h, float w, float g) {
  GSR_FP_STRICT
  const float hw = h * w;
  const float t = hw * g;
  acc = acc + t;
}

// One source pixel (y, x), every channel: acc[c] = the gradient's sum in the fixed order, BEFORE the affine's factor and
// the clamp's mask (finish_grad).  grad: this image's [C,out_h,out_w] planes.  [ylo, yhi]: axis_range of y (the same for
// a whole source row).  Returns the number of terms one channel received.
GSR_HD int backward_pixel(const Spec& sp, const float* grad, int y, int x, int ylo, int yhi, float acc[MAX_C]) {
  for (int c = 0; c < MAX_C; ++c) acc[c] = 0.0f;
  int xlo, xhi;
  axis_range(sp.sx, sp.W, sp.rw, x, xlo, xhi);
  const size_t oplane = (size_t)sp.out_h * (size_t)sp.out_w;
  int n = 0;
  for (int ry = ylo; ry <= yhi; ++ry) {
    const Tap ty = axis_sample(sp.sy, sp.H, ry);
    const float* grow = grad + (size_t)(sp.top + ry) * (size_t)sp.out_w + (size_t)sp.left;
    for (int rx = xlo; rx <= xhi; ++rx) {
      const Tap tx = axis_sample(sp.sx, sp.W, rx);
      float g[MAX_C];
      for (int c = 0; c < MAX_C; ++c) g[c] = c < sp.C ? grow[(size_t)c * oplane + (size_t)rx] : 0.0f;
      const bool y0 = ty.i0 == y, y1 = ty.i1 == y, x0 = tx.i0 == x, x1 = tx.i1 == x;
      if (y0 && x0) { for (int c = 0; c < MAX_C; ++c) add_term(acc[c], ty.l0, tx.l0, g[c]); ++n; }
      if (y0 && x1) { for (int c = 0; c < MAX_C; ++c) add_term(acc[c], ty.l0, tx.l1, g[c]); ++n; }
      if (y1 && x0) { for (int c = 0; c < MAX_C; ++c) add_term(acc[c], ty.l1, tx.l0, g[c]); ++n; }
      if (y1 && x1) { for (int c = 0; c < MAX_C; ++c) add_term(acc[c], ty.l1, tx.l1, g[c]); ++n; }
    }
  }
  return n;
}

// total -> what is written: times inv_std[c] under the affine, times torch.clamp's inclusive mask (0 <= v && v <= 1; a
// NaN source gives 0) under CLAMP01, plus what grad_src held when accumulating.
GSR_HD float finish_grad(const Spec& sp, int c, float total, const float* src_px, float old, bool accumulate) {
  GSR_FP_STRICT
  float t = total;
  if (sp.affine) t = t * sp.inv_std[c];
  if (sp.flags & CLAMP01) {
    const float v = *src_px;
    t = t * ((0.0f <= v && v <= 1.0f) ? 1.0f : 0.0f);
  }
  return accumulate ? old + t : t;
}

// (uint8)(clamp(v, 0, 1) * 255.0f), truncating; NaN -> 0.
GSR_HD uint8_t to_u8(float v) {
  GSR_FP_STRICT
  const float c = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f;
  return (uint8_t)(int)(c * 255.0f);
}

}  // namespace gsr_image
