// The FPN RoI pooler in plain loops over csrc/gsr_fpn.h and csrc/gsr_rcnn.h, the same scalar source the HIP kernels compile:
//   fh_assign     what gsr_fpn_pool's first launch computes: roi_level, level_list (ascending), level_count -- integers,
//                 equal to the kernel's
//   fh_levels64   the levels alone from the same code in double
//   fh_pool       what gsr_fpn_pool's second launch computes, sample by sample, from every RoI's own level
//   fh_pool_bwd   its transpose as a plain scatter in RoI / bin / sample order per level (a different order of the same sum as
//                 gsr_fpn_pool_backward's gather); the caller zeroes the gradients
// Build: g++ -O1 -ffp-contract=off -shared -fPIC -I <csrc> fpn_host.cpp -o libfpnhost.so
#include <cstdint>

#include "gsr_fpn.h"
#include "gsr_rcnn.h"

using namespace gsr_rcnn;
typedef gsr_fpn::Spec FSpec;   // GsrFpnSpec of include/gsraster.h, field for field

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static bool spec_ok(const FSpec* d) {
  if (!d || d->B < 1 || d->S < 1 || d->S > gsr_fpn::MAX_SAMPLE || d->Cf < 1 || d->PH < 1 || d->PH > MAX_POOL || d->PW < 1 ||
      d->PW > MAX_POOL || d->sampling_ratio < 0 || d->nl < 1 || d->nl > gsr_fpn::MAX_LEVELS)
    return false;
  for (int l = 0; l < d->nl; ++l)
    if (d->Hf[l] < 1 || d->Wf[l] < 1) return false;
  return true;
}

extern "C" int fh_assign(const FSpec* d, const float* rois, const int32_t* n_roi, int32_t stride, int32_t* roi_level, int32_t* level_list,
                         int32_t* level_count) {
  if (!spec_ok(d)) return 1;
  for (int b = 0; b < d->B; ++b) {
    const int n = n_roi ? clampi(n_roi[(size_t)b * (size_t)stride], 0, d->S) : d->S;
    for (int l = 0; l < d->nl; ++l) level_count[(size_t)b * (size_t)d->nl + (size_t)l] = 0;
    for (int s = 0; s < d->S; ++s) {
      const size_t q = (size_t)b * (size_t)d->S + (size_t)s;
      const int level = gsr_fpn::roi_level<float>(rois + q * 4, s, n, d->thr, d->nl, d->canonical_size);
      roi_level[q] = level;
      if (level < 0) continue;
      const size_t row = (size_t)b * (size_t)d->nl + (size_t)level;
      level_list[row * (size_t)d->S + (size_t)level_count[row]++] = s;
    }
  }
  return 0;
}

extern "C" int fh_levels64(const FSpec* d, const float* rois, const int32_t* n_roi, int32_t stride, int32_t* roi_level) {
  if (!spec_ok(d)) return 1;
  double thr[gsr_fpn::MAX_LEVELS];
  for (int l = 0; l < gsr_fpn::MAX_LEVELS; ++l) thr[l] = (double)d->thr[l];
  for (int b = 0; b < d->B; ++b) {
    const int n = n_roi ? clampi(n_roi[(size_t)b * (size_t)stride], 0, d->S) : d->S;
    for (int s = 0; s < d->S; ++s) {
      const size_t q = (size_t)b * (size_t)d->S + (size_t)s;
      const double r[4] = {rois[q * 4], rois[q * 4 + 1], rois[q * 4 + 2], rois[q * 4 + 3]};
      roi_level[q] = gsr_fpn::roi_level<double>(r, s, n, thr, d->nl, (double)d->canonical_size);
    }
  }
  return 0;
}

// forward: pooled is written; backward (grad_pooled given): grad_features[l], zeroed by the caller, are added to
static int pool_walk(const FSpec* d, const float* const* features, const float* rois, const int32_t* roi_level, float* pooled,
                     const float* grad_pooled, float* const* grad_features) {
  if (!spec_ok(d)) return 1;
  const size_t bins = (size_t)d->PH * (size_t)d->PW;
  for (int b = 0; b < d->B; ++b)
    for (int s = 0; s < d->S; ++s) {
      const size_t q = (size_t)b * (size_t)d->S + (size_t)s;
      const float* r = rois + q * 4;
      const int l = roi_level[q];
      const bool live = l >= 0 && l < d->nl && roi_finite<float>(r);
      const int Hf = live ? d->Hf[l] : 1, Wf = live ? d->Wf[l] : 1;
      const size_t HW = (size_t)Hf * (size_t)Wf;
      float sx = 0, bx = 0, sy = 0, by = 0;
      int gx = 0, gy = 0;
      if (live) {
        roi_axis<float>(r[0], r[2], d->scale[l], d->PW, d->sampling_ratio, sx, bx, gx);
        roi_axis<float>(r[1], r[3], d->scale[l], d->PH, d->sampling_ratio, sy, by, gy);
      }
      const float cnt = (float)(gx * gy > 1 ? gx * gy : 1);
      for (int c = 0; c < d->Cf; ++c) {
        const size_t fo = ((size_t)b * (size_t)d->Cf + (size_t)c) * HW;
        const size_t po = (q * (size_t)d->Cf + (size_t)c) * bins;
        for (int ph = 0; ph < d->PH; ++ph)
          for (int pw = 0; pw < d->PW; ++pw) {
            const size_t e = po + (size_t)ph * (size_t)d->PW + (size_t)pw;
            float acc = 0.0f;
            const float g = grad_pooled ? grad_pooled[e] / cnt : 0.0f;
            for (int iy = 0; live && iy < gy; ++iy) {
              int yl, yh, xl, xh;
              float hy, ly, hx, lx;
              const bool oky = lerp_axis<float>(sample_pos<float>(sy, by, gy, ph, iy), Hf, yl, yh, hy, ly);
              for (int ix = 0; ix < gx; ++ix) {
                const bool okx = lerp_axis<float>(sample_pos<float>(sx, bx, gx, pw, ix), Wf, xl, xh, hx, lx);
                if (!(oky && okx)) continue;
                const size_t i1 = fo + (size_t)yl * (size_t)Wf + (size_t)xl, i2 = fo + (size_t)yl * (size_t)Wf + (size_t)xh;
                const size_t i3 = fo + (size_t)yh * (size_t)Wf + (size_t)xl, i4 = fo + (size_t)yh * (size_t)Wf + (size_t)xh;
                if (grad_pooled) {
                  float* gf = grad_features[l];
                  gf[i1] += (hy * hx) * g; gf[i2] += (hy * lx) * g;
                  gf[i3] += (ly * hx) * g; gf[i4] += (ly * lx) * g;
                } else {
                  const float* f = features[l];
                  acc = acc + (((hy * hx) * f[i1] + (hy * lx) * f[i2]) + (ly * hx) * f[i3] + (ly * lx) * f[i4]);
                }
              }
            }
            if (!grad_pooled) pooled[e] = acc / cnt;
          }
      }
    }
  return 0;
}

extern "C" int fh_pool(const FSpec* d, const float* const* features, const float* rois, const int32_t* roi_level, float* pooled) {
  return pool_walk(d, features, rois, roi_level, pooled, nullptr, nullptr);
}

extern "C" int fh_pool_bwd(const FSpec* d, const float* rois, const int32_t* roi_level, const float* grad_pooled, float* const* grad_features) {
  return pool_walk(d, nullptr, rois, roi_level, nullptr, grad_pooled, grad_features);
}
