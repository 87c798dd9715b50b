// The fused image losses in plain loops over csrc/gsr_imgloss.h, the same scalar source the HIP kernels compile:
//   ih_tile      IMGLOSS_TH, IMGLOSS_TW and the eleven taps, as the header holds them
//   ih_imgloss   what gsr_imgloss computes: terms [B,4], ssim_map and grad_img [B,C,H,W] (either may be null).  The map and
//                the gradient take the kernels' operations in the kernels' order (rows, then columns, zeros beyond the
//                image); the three sums of an image are plain double sums in pixel order -- a different order of the same
//                sum as the kernels' tiles.
// Build: g++ -O1 -ffp-contract=off -shared -fPIC -I <csrc> imgloss_host.cpp -o libimglosshost.so
#include <cmath>
#include <cstdint>
#include <vector>

#include "gsr_imgloss.h"

using namespace gsr_il;

extern "C" void ih_tile(int32_t* th, int32_t* tw, float* taps) {
  const float w[WIN] = GSR_IMGLOSS_TAPS;
  *th = IMGLOSS_TH;
  *tw = IMGLOSS_TW;
  for (int k = 0; k < WIN; ++k) taps[k] = w[k];
}

// out[y][x] = the window sum of in[y][x - 5 .. x + 5] (rows pass) -- then of tmp[y - 5 .. y + 5][x]: zeros beyond the plane
static void window2(const std::vector<float>& in, int H, int W, std::vector<float>& tmp, std::vector<float>& out) {
  float v[WIN];
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      for (int k = 0; k < WIN; ++k) {
        const int gx = x - HALO + k;
        v[k] = (gx >= 0 && gx < W) ? in[(size_t)y * W + gx] : 0.0f;
      }
      tmp[(size_t)y * W + x] = win11<float>(v, 1);
    }
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      for (int k = 0; k < WIN; ++k) {
        const int gy = y - HALO + k;
        v[k] = (gy >= 0 && gy < H) ? tmp[(size_t)gy * W + x] : 0.0f;
      }
      out[(size_t)y * W + x] = win11<float>(v, 1);
    }
}

extern "C" int ih_imgloss(const Spec* d, const float* img, const float* ref, float* terms, float* grad, float* ssim_map) {
  if (!d || d->B < 1 || d->C < 1 || d->C > MAX_CHANNELS || d->H < 1 || d->W < 1 || !img || !ref || !terms) return 1;
  const int H = d->H, W = d->W;
  const size_t hw = (size_t)H * (size_t)W;
  const bool clamp = (d->flags & FLAG_CLAMP01) != 0u;
  const float inv_n = 1.0f / (float)((long long)d->C * H * W);
  std::vector<float> xs(hw), ys(hw), row[5], dm[3], tmp(hw), g[3];
  for (auto& r : row) r.resize(hw);
  for (auto& r : dm) r.resize(hw);
  for (auto& r : g) r.resize(hw);
  for (int b = 0; b < d->B; ++b) {
    double s_abs = 0.0, s_sq = 0.0, s_map = 0.0;
    for (int c = 0; c < d->C; ++c) {
      const size_t off = ((size_t)b * (size_t)d->C + (size_t)c) * hw;
      for (size_t e = 0; e < hw; ++e) {
        xs[e] = clamp ? clamp01<float>(img[off + e]) : img[off + e];
        ys[e] = clamp ? clamp01<float>(ref[off + e]) : ref[off + e];
      }
      float xv[WIN], yv[WIN], o[5];
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          for (int k = 0; k < WIN; ++k) {
            const int gx = x - HALO + k;
            const bool in = gx >= 0 && gx < W;
            xv[k] = in ? xs[(size_t)y * W + gx] : 0.0f;
            yv[k] = in ? ys[(size_t)y * W + gx] : 0.0f;
          }
          row_stats<float>(xv, yv, o);
          for (int q = 0; q < 5; ++q) row[q][(size_t)y * W + x] = o[q];
        }
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          float st[5], v[WIN];
          for (int q = 0; q < 5; ++q) {
            for (int k = 0; k < WIN; ++k) {
              const int gy = y - HALO + k;
              v[k] = (gy >= 0 && gy < H) ? row[q][(size_t)gy * W + x] : 0.0f;
            }
            st[q] = win11<float>(v, 1);
          }
          const size_t e = (size_t)y * W + x;
          const float m = ssim_point<float>(st[0], st[1], st[2], st[3], st[4], dm[0][e], dm[1][e], dm[2][e]);
          const float df = diff<float>(xs[e], ys[e]);
          s_abs += (double)fabsf(df);
          s_sq += (double)sq<float>(df);
          s_map += (double)m;
          if (ssim_map) ssim_map[off + e] = m;
        }
      if (grad) {
        for (int q = 0; q < 3; ++q) window2(dm[q], H, W, tmp, g[q]);
        for (size_t e = 0; e < hw; ++e) {
          const float mask = clamp ? clamp_mask<float>(img[off + e]) : 1.0f;
          grad[off + e] = grad_point<float>(xs[e], ys[e], g[0][e], g[1][e], g[2][e], d->w_l1, d->w_l2, d->w_ssim, inv_n, mask);
        }
      }
    }
    finish_terms(s_abs, s_sq, s_map, (int64_t)d->C * H * W, d->w_l1, d->w_l2, d->w_ssim, terms + (size_t)b * 4);
  }
  return 0;
}
