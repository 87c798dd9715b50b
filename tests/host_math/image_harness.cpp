// Stand-alone run of the image front end's host forward and backward on the three smallest shapes, for a build with
// -fsanitize=address,undefined: every buffer is exactly as large as the shape says, so an index outside a plane is
// reported.  Also checks, against a brute-force scatter over the forward taps, that the gather's inverse ranges miss no
// term.  Prints "image_harness ok" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "image_host.cpp"

namespace {

struct Shape { int H, W, rh, rw, out_h, out_w, top, left; };

float noise(uint32_t& s) {
  s = s * 1664525u + 1013904223u;
  return (float)(s >> 8) * (1.0f / 16777216.0f);
}

int run(const Shape& q, int C, uint32_t flags, bool affine) {
  const int B = 2;
  uint32_t seed = 12345u + (uint32_t)(q.H * 131 + q.W);
  std::vector<float> src((size_t)B * C * q.H * q.W), dst((size_t)B * C * q.out_h * q.out_w), g(dst.size()), gs(src.size());
  for (float& v : src) v = noise(seed) * 1.4f - 0.2f;
  for (float& v : g) v = noise(seed) * 2.0f - 1.0f;
  const float mean[4] = {0.485f, 0.456f, 0.406f, 0.5f}, inv_std[4] = {4.37f, 4.46f, 4.44f, 2.0f};
  const float* m = affine ? mean : nullptr;
  const float* is = affine ? inv_std : nullptr;
  if (ih_forward(B, C, q.H, q.W, q.out_h, q.out_w, q.rh, q.rw, q.top, q.left, 0.447f, m, is, flags, src.data(), dst.data())) return 1;
  int n_max = 0;
  if (ih_backward(B, C, q.H, q.W, q.out_h, q.out_w, q.rh, q.rw, q.top, q.left, m, is, flags, src.data(), g.data(), gs.data(), 0, &n_max))
    return 2;
  if (ih_backward(B, C, q.H, q.W, q.out_h, q.out_w, q.rh, q.rw, q.top, q.left, m, is, flags, src.data(), g.data(), gs.data(), 1, nullptr))
    return 3;
  for (float v : dst) if (!std::isfinite(v)) return 4;
  // scatter in double over the forward taps: the gather must agree to rounding (it would be off by a whole term otherwise)
  std::vector<double> ref(src.size(), 0.0);
  const float sy = gsr_image::axis_scale(q.H, q.rh), sx = gsr_image::axis_scale(q.W, q.rw);
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < C; ++c)
      for (int ry = 0; ry < q.rh; ++ry)
        for (int rx = 0; rx < q.rw; ++rx) {
          const gsr_image::Tap ty = gsr_image::axis_sample(sy, q.H, ry), tx = gsr_image::axis_sample(sx, q.W, rx);
          const double gv = g[(((size_t)b * C + c) * q.out_h + q.top + ry) * q.out_w + q.left + rx] * (affine ? (double)inv_std[c] : 1.0);
          double* r = ref.data() + ((size_t)b * C + c) * q.H * q.W;
          r[(size_t)ty.i0 * q.W + tx.i0] += (double)ty.l0 * tx.l0 * gv;
          r[(size_t)ty.i0 * q.W + tx.i1] += (double)ty.l0 * tx.l1 * gv;
          r[(size_t)ty.i1 * q.W + tx.i0] += (double)ty.l1 * tx.l0 * gv;
          r[(size_t)ty.i1 * q.W + tx.i1] += (double)ty.l1 * tx.l1 * gv;
        }
  for (size_t i = 0; i < src.size(); ++i) {
    const bool pass = !(flags & gsr_image::CLAMP01) || (0.0f <= src[i] && src[i] <= 1.0f);
    const double want = pass ? 2.0 * ref[i] : 0.0;                     // the second call accumulated onto the first
    if (std::fabs((double)gs[i] - want) > 1e-4 * (1.0 + std::fabs(want))) {
      std::fprintf(stderr, "gather != scatter at %zu: %g vs %g (n_max %d)\n", i, (double)gs[i], want, n_max);
      return 5;
    }
  }
  return 0;
}

}  // namespace

int main() {
  const Shape shapes[] = {{1, 1, 4, 4, 4, 4, 0, 0}, {2, 3, 1, 1, 1, 1, 0, 0}, {9, 16, 23, 37, 23, 37, 0, 0},
                          {2, 3, 1, 1, 4, 5, 2, 3}, {9, 16, 23, 37, 40, 40, 8, 1}};
  for (const Shape& q : shapes)
    for (int C = 1; C <= 4; C += 3)
      for (int mode = 0; mode < 4; ++mode) {
        const int rc = run(q, C, (mode & 1) ? gsr_image::CLAMP01 : 0u, (mode & 2) != 0);
        if (rc) {
          std::fprintf(stderr, "image_harness: shape %dx%d -> %dx%d C=%d mode=%d failed with %d\n", q.H, q.W, q.rh, q.rw, C, mode, rc);
          return 1;
        }
      }
  std::uint8_t px[2 * 5 * 7 * 3];
  std::vector<float> im(2 * 3 * 5 * 7);
  uint32_t seed = 7u;
  for (float& v : im) v = noise(seed) * 1.4f - 0.2f;
  ih_to_u8(im.data(), 2, 5, 7, px);
  std::printf("image_harness ok\n");
  return 0;
}
