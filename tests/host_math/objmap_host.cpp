// The object-map classifier in plain loops over csrc/gsr_objmap.h, the same scalar source the HIP kernels compile:
//   oh_limits    CH, MAX_CLASSES, OM_THREADS and FLAG_LOSS, as the header holds them
//   oh_objmap    what gsr_objmap computes: ids [B,H,W], and, each when non-null, conf [B,H,W], stats [B,K,5], paint [B,H,W,3],
//                terms [B,2], grad [B,16,H,W].  Ids, stats and paint take the kernels' operations in the kernels' order (the
//                same bits); an image's CE terms are added in pixel order in double -- a different order of the same sum
//                as the kernels' trees -- and expf / logf are the host's.
// Build: g++ -O1 -ffp-contract=off -shared -fPIC -I <csrc> objmap_host.cpp -o libobjmaphost.so
#include <climits>
#include <cmath>
#include <cstdint>

#include "gsr_objmap.h"

using namespace gsr_om;

extern "C" void oh_limits(int32_t* out) {
  out[0] = CH;
  out[1] = MAX_CLASSES;
  out[2] = OM_THREADS;
  out[3] = (int32_t)FLAG_LOSS;
}

extern "C" int oh_objmap(const Spec* d, const float* objmap, const float* weight, const float* bias, const int32_t* target,
                         const uint8_t* palette, int32_t* ids, float* conf, int32_t* stats, uint8_t* paint, float* terms, float* grad) {
  if (!d || d->B < 1 || d->H < 1 || d->W < 1 || d->K < 1 || d->K > MAX_CLASSES || !objmap || !weight || !bias || !ids) return 1;
  if ((paint && !palette) || ((terms || grad) && (!target || !(d->flags & FLAG_LOSS)))) return 1;
  const int K = d->K, W = d->W;
  const size_t hw = (size_t)d->H * (size_t)W;
  const bool loss = terms || grad;
  for (int b = 0; b < d->B; ++b) {
    const float* img = objmap + (size_t)b * CH * hw;
    int32_t* rows = stats ? stats + (size_t)b * K * 5 : nullptr;
    if (rows)
      for (int c = 0; c < K; ++c) { rows[5 * c] = 0; rows[5 * c + 1] = INT_MAX; rows[5 * c + 2] = INT_MAX; rows[5 * c + 3] = 0; rows[5 * c + 4] = 0; }
    float f[CH];
    int32_t valid = 0;
    if (loss)
      for (size_t p = 0; p < hw; ++p) {
        const int t = target[(size_t)b * hw + p];
        if (t < 0 || t >= K) continue;
        for (int k = 0; k < CH; ++k) f[k] = img[(size_t)k * hw + p];
        valid += alive(weight, bias, K, f) ? 1 : 0;
      }
    const float scale = inv_valid(valid);
    double ce_sum = 0.0;
    for (size_t p = 0; p < hw; ++p) {
      const size_t px = (size_t)b * hw + p;
      for (int k = 0; k < CH; ++k) f[k] = img[(size_t)k * hw + p];
      float m;
      int id;
      pass_max(weight, bias, K, f, m, id);
      ids[px] = id;
      if (paint)
        for (int q = 0; q < 3; ++q) paint[3 * px + q] = id >= 0 ? palette[3 * id + q] : (uint8_t)0;
      if (rows && id >= 0) {
        const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
        int32_t* r = rows + 5 * id;
        r[0] += 1;
        r[1] = x < r[1] ? x : r[1];
        r[2] = y < r[2] ? y : r[2];
        r[3] = x + 1 > r[3] ? x + 1 : r[3];
        r[4] = y + 1 > r[4] ? y + 1 : r[4];
      }
      if (!loss && !conf) continue;
      const int t = loss ? target[px] : -1;
      float l_t = 0.0f;
      const float sum = pass_sum(weight, bias, K, f, m, t, l_t);
      const float cf = confidence(id, sum);
      if (conf) conf[px] = cf;
      if (!loss) continue;
      const bool cnt = counted(id, t, K);
      if (cnt) ce_sum += (double)ce_term(m, l_t, sum);
      if (grad) {
        float g[CH];
        pass_grad(weight, bias, K, f, m, cf, t, scale, g);
        for (int k = 0; k < CH; ++k) grad[(size_t)b * CH * hw + (size_t)k * hw + p] = cnt ? g[k] : 0.0f;
      }
    }
    if (rows)
      for (int c = 0; c < K; ++c)
        if (rows[5 * c] == 0) { rows[5 * c + 1] = 0; rows[5 * c + 2] = 0; rows[5 * c + 3] = 0; rows[5 * c + 4] = 0; }
    if (terms) {
      terms[2 * b] = mean_ce((float)ce_sum, valid);
      terms[2 * b + 1] = (float)valid;
    }
  }
  return 0;
}
