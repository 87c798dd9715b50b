// Host build of csrc/gsr_image.h: the image front end's forward and backward over whole tensors, the same scalar
// source the HIP kernels compile.  g++ -O1 -ffp-contract=off -shared -fPIC (tests/test_image_host_cpu.py builds it);
// image_harness.cpp includes this file and adds a main for the sanitised run.
#include <cstdint>
#include <cstddef>

#include "gsr_image.h"

namespace {

gsr_image::Spec make_spec(int C, int H, int W, int out_h, int out_w, int rh, int rw, int top, int left, float pad,
                          const float* mean, const float* inv_std, uint32_t flags) {
  gsr_image::Spec sp;
  sp.C = C; sp.H = H; sp.W = W; sp.out_h = out_h; sp.out_w = out_w;
  sp.rh = rh; sp.rw = rw; sp.top = top; sp.left = left;
  sp.pad_value = pad;
  sp.sy = gsr_image::axis_scale(H, rh);
  sp.sx = gsr_image::axis_scale(W, rw);
  sp.flags = flags;
  sp.affine = (mean || inv_std) ? 1 : 0;
  for (int c = 0; c < gsr_image::MAX_C; ++c) {
    sp.mean[c] = (mean && c < C) ? mean[c] : 0.0f;
    sp.inv_std[c] = (inv_std && c < C) ? inv_std[c] : 1.0f;
  }
  return sp;
}

bool spec_ok(int B, int C, int H, int W, int out_h, int out_w, int rh, int rw, int top, int left) {
  return B >= 1 && C >= 1 && C <= gsr_image::MAX_C && H >= 1 && W >= 1 && out_h >= 1 && out_w >= 1 && rh >= 1 && rw >= 1 &&
         top >= 0 && left >= 0 && top + rh <= out_h && left + rw <= out_w;
}

}  // namespace

extern "C" {

int ih_forward(int B, int C, int H, int W, int out_h, int out_w, int rh, int rw, int top, int left, float pad,
               const float* mean, const float* inv_std, uint32_t flags, const float* src, float* dst) {
  if (!spec_ok(B, C, H, W, out_h, out_w, rh, rw, top, left) || !src || !dst) return 1;
  const gsr_image::Spec sp = make_spec(C, H, W, out_h, out_w, rh, rw, top, left, pad, mean, inv_std, flags);
  const size_t splane = (size_t)H * W, oplane = (size_t)out_h * out_w;
  for (int b = 0; b < B; ++b)
    for (int oy = 0; oy < out_h; ++oy)
      for (int ox = 0; ox < out_w; ++ox) {
        float out[gsr_image::MAX_C];
        gsr_image::forward_pixel(sp, src + (size_t)b * C * splane, oy, ox, out);
        for (int c = 0; c < C; ++c) dst[((size_t)b * C + c) * oplane + (size_t)oy * out_w + ox] = out[c];
      }
  return 0;
}

// *n_max (may be null): the largest number of terms a source pixel received
int ih_backward(int B, int C, int H, int W, int out_h, int out_w, int rh, int rw, int top, int left, const float* mean,
                const float* inv_std, uint32_t flags, const float* src, const float* grad_dst, float* grad_src,
                int accumulate, int* n_max) {
  if (!spec_ok(B, C, H, W, out_h, out_w, rh, rw, top, left) || !grad_dst || !grad_src) return 1;
  if ((flags & gsr_image::CLAMP01) && !src) return 1;
  const gsr_image::Spec sp = make_spec(C, H, W, out_h, out_w, rh, rw, top, left, 0.0f, mean, inv_std, flags);
  const size_t splane = (size_t)H * W, oplane = (size_t)out_h * out_w;
  int worst = 0;
  for (int b = 0; b < B; ++b)
    for (int y = 0; y < H; ++y) {
      int ylo, yhi;
      gsr_image::axis_range(sp.sy, H, rh, y, ylo, yhi);
      for (int x = 0; x < W; ++x) {
        float acc[gsr_image::MAX_C];
        const int n = gsr_image::backward_pixel(sp, grad_dst + (size_t)b * C * oplane, y, x, ylo, yhi, acc);
        if (n > worst) worst = n;
        for (int c = 0; c < C; ++c) {
          const size_t o = ((size_t)b * C + c) * splane + (size_t)y * W + x;
          const float v = (flags & gsr_image::CLAMP01) ? src[o] : 0.0f;
          grad_src[o] = gsr_image::finish_grad(sp, c, acc[c], &v, accumulate ? grad_src[o] : 0.0f, accumulate != 0);
        }
      }
    }
  if (n_max) *n_max = worst;
  return 0;
}

void ih_to_u8(const float* src, int B, int H, int W, uint8_t* dst) {
  const size_t plane = (size_t)H * W;
  for (int b = 0; b < B; ++b)
    for (size_t p = 0; p < plane; ++p)
      for (int c = 0; c < 3; ++c) dst[((size_t)b * plane + p) * 3 + c] = gsr_image::to_u8(src[((size_t)b * 3 + c) * plane + p]);
}

// one axis of the forward formula, and the exact inverse range of a source index: for the tests of the header itself
void ih_axis_sample(int in, int out, int d, int* i01, float* l01) {
  const gsr_image::Tap t = gsr_image::axis_sample(gsr_image::axis_scale(in, out), in, d);
  i01[0] = t.i0; i01[1] = t.i1; l01[0] = t.l0; l01[1] = t.l1;
}

void ih_axis_range(int in, int out, int s, int* lohi) {
  gsr_image::axis_range(gsr_image::axis_scale(in, out), in, out, s, lohi[0], lohi[1]);
}

}  // extern "C"
