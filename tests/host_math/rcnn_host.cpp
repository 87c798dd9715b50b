// The two-stage detector stage in plain loops over csrc/gsr_rcnn.h, the same scalar source the HIP kernels compile:
//   rh_sample         what gsr_rcnn_sample computes (integers and gathered boxes: equal to the kernel's)
//   rh_roi_align      what gsr_roi_align computes, sample by sample
//   rh_roi_align_bwd  its transpose in gsr_roi_align_backward's order (a gather over separable weights)
//   rh_roi_align_bwd_scatter  the same as a plain scatter in RoI / bin / sample order (a different order of the same sum)
//   rh_loss_f32       what gsr_rcnn_loss computes, every sum in the kernels' order (wave_stats, kernel_order_sum)
//   rh_loss_f64       the same code in double
//   rh_post           what gsr_rcnn_postprocess computes: candidates, the NMS walk of csrc/gsr_detect.h, dets and counts
// Build: g++ -O1 -ffp-contract=off -shared -fPIC -I <csrc> rcnn_host.cpp -o librcnnhost.so
#include <algorithm>
#include <cstdint>
#include <vector>

#include "gsr_detect.h"
#include "gsr_rcnn.h"

using namespace gsr_rcnn;

struct HostSpec {   // GsrRcnnSpec of include/gsraster.h
  int32_t B, R, M, S, C, max_pos, append_gt;
  uint32_t seed;
  float fg_iou;
  int32_t Cf, Hf, Wf, PH, PW;
  float spatial_scale;
  int32_t sampling_ratio;
  float bw_x, bw_y, bw_w, bw_h, beta, w_cls, w_box, conf_thr, iou_thr;
  int32_t max_det;
  float img_w, img_h;
  uint32_t flags;
};

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

extern "C" int rh_sample(const HostSpec* d, const float* proposals, const int32_t* n_prop, const float* gt_boxes, const int32_t* gt_cls,
                         int32_t* idx, float* rois, int32_t* labels, int32_t* gt_row, int32_t* counts) {
  if (!d || d->B < 1 || d->R < 1 || d->M < 1 || d->M > MAX_ROWS || d->R + d->M > MAX_CAND || d->S < 1 || d->S > MAX_SAMPLE ||
      d->C < 1 || d->max_pos < 0 || d->max_pos > d->S)
    return 1;
  const int R = d->R, M = d->M, S = d->S, N = R + (d->append_gt ? M : 0);
  std::vector<int32_t> info((size_t)N);
  std::vector<uint32_t> key((size_t)N);
  for (int b = 0; b < d->B; ++b) {
    const float* gb = gt_boxes + (size_t)b * (size_t)M * 4;
    const int32_t* gc = gt_cls + (size_t)b * (size_t)M;
    const int np = n_prop ? clampi(n_prop[b], 0, R) : R;
    auto box = [&](int i) { return i < R ? proposals + ((size_t)b * (size_t)R + (size_t)i) * 4 : gb + (size_t)(i - R) * 4; };
    int nfg = 0, nbg = 0;
    for (int i = 0; i < N; ++i) {
      const bool valid = i < R ? i < np : present(gc[i - R], d->C);
      info[(size_t)i] = -2;
      key[(size_t)i] = sample_key(d->seed, b, i);
      if (!valid) continue;
      float best;
      info[(size_t)i] = match_candidate<float>(box(i), gb, gc, M, d->C, d->fg_iou, best);
      if (info[(size_t)i] >= 0) ++nfg; else ++nbg;
    }
    const int n_pos = std::min(nfg, d->max_pos), n_neg = std::min(nbg, S - n_pos);
    int pos = 0;
    for (int i = 0; i < N; ++i) {
      if (info[(size_t)i] == -2) continue;
      const bool fg = info[(size_t)i] >= 0;
      int rank = 0;
      for (int j = 0; j < N; ++j)
        if (info[(size_t)j] != -2 && (info[(size_t)j] >= 0) == fg && key_before(key[(size_t)j], j, key[(size_t)i], i)) ++rank;
      if (rank >= (fg ? n_pos : n_neg)) continue;
      const size_t o = (size_t)b * (size_t)S + (size_t)pos;
      idx[o] = i;
      for (int c = 0; c < 4; ++c) rois[o * 4 + (size_t)c] = box(i)[c];
      labels[o] = fg ? gc[info[(size_t)i]] : d->C;
      gt_row[o] = fg ? info[(size_t)i] : -1;
      ++pos;
    }
    counts[(size_t)b * 2] = pos;
    counts[(size_t)b * 2 + 1] = n_pos;
    for (; pos < S; ++pos) {
      const size_t o = (size_t)b * (size_t)S + (size_t)pos;
      idx[o] = -1;
      for (int c = 0; c < 4; ++c) rois[o * 4 + (size_t)c] = 0.0f;
      labels[o] = -1;
      gt_row[o] = -1;
    }
  }
  return 0;
}

// forward: pooled is written; backward (grad_pooled given): grad_features, zeroed by the caller, is added to
static int roi_walk(const HostSpec* d, const float* features, const float* rois, const int32_t* n_roi, int32_t stride, float* pooled,
                    const float* grad_pooled, float* grad_features) {
  if (!d || d->B < 1 || d->S < 1 || d->Cf < 1 || d->Hf < 1 || d->Wf < 1 || d->PH < 1 || d->PH > MAX_POOL || d->PW < 1 ||
      d->PW > MAX_POOL || d->sampling_ratio < 0)
    return 1;
  const size_t HW = (size_t)d->Hf * (size_t)d->Wf, bins = (size_t)d->PH * (size_t)d->PW;
  for (int b = 0; b < d->B; ++b) {
    const int n = n_roi ? clampi(n_roi[(size_t)b * (size_t)stride], 0, d->S) : d->S;
    for (int s = 0; s < d->S; ++s) {
      const float* r = rois + ((size_t)b * (size_t)d->S + (size_t)s) * 4;
      const bool live = s < n && roi_finite<float>(r);
      float sx = 0, bx = 0, sy = 0, by = 0;
      int gx = 0, gy = 0;
      if (live) {
        roi_axis<float>(r[0], r[2], d->spatial_scale, d->PW, d->sampling_ratio, sx, bx, gx);
        roi_axis<float>(r[1], r[3], d->spatial_scale, d->PH, d->sampling_ratio, sy, by, gy);
      }
      const float cnt = (float)(gx * gy > 1 ? gx * gy : 1);
      for (int c = 0; c < d->Cf; ++c) {
        const size_t fo = ((size_t)b * (size_t)d->Cf + (size_t)c) * HW;
        const size_t po = (((size_t)b * (size_t)d->S + (size_t)s) * (size_t)d->Cf + (size_t)c) * bins;
        for (int ph = 0; ph < d->PH; ++ph)
          for (int pw = 0; pw < d->PW; ++pw) {
            const size_t e = po + (size_t)ph * (size_t)d->PW + (size_t)pw;
            float acc = 0.0f;
            const float g = grad_pooled ? grad_pooled[e] / cnt : 0.0f;
            for (int iy = 0; live && iy < gy; ++iy) {
              int yl, yh, xl, xh;
              float hy, ly, hx, lx;
              const bool oky = lerp_axis<float>(sample_pos<float>(sy, by, gy, ph, iy), d->Hf, yl, yh, hy, ly);
              for (int ix = 0; ix < gx; ++ix) {
                const bool okx = lerp_axis<float>(sample_pos<float>(sx, bx, gx, pw, ix), d->Wf, xl, xh, hx, lx);
                if (!(oky && okx)) continue;
                const size_t i1 = fo + (size_t)yl * (size_t)d->Wf + (size_t)xl, i2 = fo + (size_t)yl * (size_t)d->Wf + (size_t)xh;
                const size_t i3 = fo + (size_t)yh * (size_t)d->Wf + (size_t)xl, i4 = fo + (size_t)yh * (size_t)d->Wf + (size_t)xh;
                if (grad_pooled) {
                  grad_features[i1] += (hy * hx) * g; grad_features[i2] += (hy * lx) * g;
                  grad_features[i3] += (ly * hx) * g; grad_features[i4] += (ly * lx) * g;
                } else {
                  acc = acc + (((hy * hx) * features[i1] + (hy * lx) * features[i2]) + (ly * hx) * features[i3] + (ly * lx) * features[i4]);
                }
              }
            }
            if (!grad_pooled) pooled[e] = acc / cnt;
          }
      }
    }
  }
  return 0;
}

extern "C" int rh_roi_align(const HostSpec* d, const float* features, const float* rois, const int32_t* n_roi, int32_t stride, float* pooled) {
  return roi_walk(d, features, rois, n_roi, stride, pooled, nullptr, nullptr);
}

extern "C" int rh_roi_align_bwd_scatter(const HostSpec* d, const float* rois, const int32_t* n_roi, int32_t stride, const float* grad_pooled,
                                        float* grad_features) {
  return roi_walk(d, nullptr, rois, n_roi, stride, nullptr, grad_pooled, grad_features);
}

// the weight of map cell `cell` in bin p of one axis, the samples' shares added in sample order (gsr_rcnn.hip.h's axis_weight)
static float axis_weight(float start, float bin, int grid, int p, int n, int cell) {
  float w = 0.0f;
  for (int i = 0; i < grid; ++i) {
    int lo, hi;
    float wl, wh;
    if (!lerp_axis<float>(sample_pos<float>(start, bin, grid, p, i), n, lo, hi, wl, wh)) continue;
    if (lo == cell) w = w + wl;
    if (hi == cell) w = w + wh;
  }
  return w;
}

// The backward in k_roi_align_bwd's order: per element the RoIs in ascending order; of a RoI the separable weights wy, wx,
// the bins with a non-zero weight in (ph, pw) order, (wy * wx) * g added up, the sum divided by the sample count.  The
// scatter above adds every sample's four shares one by one: with 16 x 16 samples in each of 49 bins its rounding grows to
// 5 .. 7 x the float32 oracle's, where the kernel's few sums stay at it.  grad_features, zeroed by the caller, is added to.
extern "C" int rh_roi_align_bwd(const HostSpec* d, const float* rois, const int32_t* n_roi, int32_t stride, const float* grad_pooled,
                                float* grad_features) {
  if (!d || d->B < 1 || d->S < 1 || d->Cf < 1 || d->Hf < 1 || d->Wf < 1 || d->PH < 1 || d->PH > MAX_POOL || d->PW < 1 ||
      d->PW > MAX_POOL || d->sampling_ratio < 0)
    return 1;
  const int Hf = d->Hf, Wf = d->Wf, PH = d->PH, PW = d->PW;
  const size_t HW = (size_t)Hf * (size_t)Wf, bins = (size_t)PH * (size_t)PW;
  std::vector<float> wy((size_t)Hf * (size_t)PH), wx((size_t)Wf * (size_t)PW);
  std::vector<char> any_y((size_t)Hf), any_x((size_t)Wf);
  for (int b = 0; b < d->B; ++b) {
    const int n = n_roi ? clampi(n_roi[(size_t)b * (size_t)stride], 0, d->S) : d->S;
    for (int s = 0; s < n; ++s) {
      const float* r = rois + ((size_t)b * (size_t)d->S + (size_t)s) * 4;
      if (!roi_finite<float>(r)) continue;
      float sx, bx, sy, by;
      int gx, gy;
      roi_axis<float>(r[0], r[2], d->spatial_scale, PW, d->sampling_ratio, sx, bx, gx);
      roi_axis<float>(r[1], r[3], d->spatial_scale, PH, d->sampling_ratio, sy, by, gy);
      if (gx < 1 || gy < 1) continue;
      for (int y = 0; y < Hf; ++y) {
        any_y[(size_t)y] = 0;
        for (int ph = 0; ph < PH; ++ph)
          if ((wy[(size_t)y * (size_t)PH + (size_t)ph] = axis_weight(sy, by, gy, ph, Hf, y)) != 0.0f) any_y[(size_t)y] = 1;
      }
      for (int x = 0; x < Wf; ++x) {
        any_x[(size_t)x] = 0;
        for (int pw = 0; pw < PW; ++pw)
          if ((wx[(size_t)x * (size_t)PW + (size_t)pw] = axis_weight(sx, bx, gx, pw, Wf, x)) != 0.0f) any_x[(size_t)x] = 1;
      }
      const float cnt = (float)(gx * gy);
      for (int c = 0; c < d->Cf; ++c) {
        const float* g0 = grad_pooled + (((size_t)b * (size_t)d->S + (size_t)s) * (size_t)d->Cf + (size_t)c) * bins;
        float* gf = grad_features + ((size_t)b * (size_t)d->Cf + (size_t)c) * HW;
        for (int y = 0; y < Hf; ++y)
          for (int x = 0; x < Wf; ++x) {
            if (!any_y[(size_t)y] || !any_x[(size_t)x]) continue;
            float part = 0.0f;
            for (int ph = 0; ph < PH; ++ph) {
              const float vy = wy[(size_t)y * (size_t)PH + (size_t)ph];
              if (vy == 0.0f) continue;
              for (int pw = 0; pw < PW; ++pw) {
                const float vx = wx[(size_t)x * (size_t)PW + (size_t)pw];
                if (vx == 0.0f) continue;
                const float w = vy * vx;
                part = part + w * g0[(size_t)ph * (size_t)PW + (size_t)pw];
              }
            }
            gf[(size_t)y * (size_t)Wf + (size_t)x] = gf[(size_t)y * (size_t)Wf + (size_t)x] + part / cnt;
          }
      }
    }
  }
  return 0;
}

// The statistics of one row of n logits in the order k_rcnn_rows takes them (gsr_block::wave_softmax_stats): 64 lanes stride
// the row, then an xor butterfly over the lanes.
template <class T>
static void wave_stats(const T* x, int n, T& mx, T& sum) {
  T a[64], o[64];
  for (int l = 0; l < 64; ++l) {
    T m = (T)-INFINITY;
    for (int k = l; k < n; k += 64) m = x[k] > m ? x[k] : m;
    a[l] = m;
  }
  for (int s = 32; s >= 1; s >>= 1) {
    for (int l = 0; l < 64; ++l) o[l] = a[l ^ s] > a[l] ? a[l ^ s] : a[l];
    for (int l = 0; l < 64; ++l) a[l] = o[l];
  }
  mx = a[0];
  for (int l = 0; l < 64; ++l) {
    T t = (T)0;
    for (int k = l; k < n; k += 64) t = t + m_exp(x[k] - mx);
    a[l] = t;
  }
  for (int s = 32; s >= 1; s >>= 1) {
    for (int l = 0; l < 64; ++l) o[l] = a[l] + a[l ^ s];
    for (int l = 0; l < 64; ++l) a[l] = o[l];
  }
  sum = a[0];
}

// One column of the loss's sum in the kernels' order: the rows' terms four to a block, added in wave order (k_rcnn_rows);
// the blocks' partials by 256 lanes, lane t taking the entries t, t + 256, ... in index order, then the stride-halving tree
// (gsr_block::slab_sum in k_rcnn_final).  Summed serially, the 2048 rows of `s1024` put `loss` at 7.6 x the float32 oracle's
// error; in this order it stays where the kernels are.
template <class T>
static T kernel_order_sum(const std::vector<T>& rows) {
  const size_t blocks = (rows.size() + 3) / 4;
  T lane[256];
  for (int t = 0; t < 256; ++t) lane[t] = (T)0;
  for (size_t j = 0; j < blocks; ++j) {
    T s = rows[j * 4];
    for (size_t w = 1; w < 4; ++w) s = s + (j * 4 + w < rows.size() ? rows[j * 4 + w] : (T)0);
    lane[j % 256] = lane[j % 256] + s;
  }
  for (int s = 128; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) lane[t] = lane[t] + lane[t + s];
  return lane[0];
}

template <class T>
static int loss_run(const HostSpec* d, const T* scores, const T* deltas, const T* rois, const int32_t* labels, const int32_t* gt_row,
                    const T* gt_boxes, T* loss, T* grad_scores, T* grad_deltas) {
  if (!d || d->B < 1 || d->S < 1 || d->C < 1 || d->M < 1) return 1;
  const int C = d->C, n1 = C + 1, D = (d->flags & CLASS_AGNOSTIC) ? 4 : 4 * C;
  const size_t rows = (size_t)d->B * (size_t)d->S;
  long long n = 0;
  for (size_t i = 0; i < rows; ++i) n += labels[i] >= 0 && labels[i] <= C ? 1 : 0;
  const T nr = n > 1 ? (T)n : (T)1;
  const T kc = (T)d->w_cls / nr, kb = (T)d->w_box / nr;
  const T w[4] = {(T)d->bw_x, (T)d->bw_y, (T)d->bw_w, (T)d->bw_h};
  std::vector<T> row_ce(rows, (T)0), row_box(rows, (T)0);
  for (size_t i = 0; i < rows; ++i) {
    const int label = labels[i] > C ? -1 : labels[i], row = gt_row[i];
    const bool fg = label >= 0 && label < C && row >= 0 && row < d->M;
    const T* x = scores + i * (size_t)n1;
    if (label >= 0) {
      T mx, sm;
      wave_stats<T>(x, n1, mx, sm);
      row_ce[i] = -log_softmax<T>(x[label], mx, sm);
      if (grad_scores)
        for (int k = 0; k < n1; ++k) grad_scores[i * (size_t)n1 + (size_t)k] = kc * (softmax_prob<T>(x[k], mx, sm) - (k == label ? (T)1 : (T)0));
    } else if (grad_scores) {
      for (int k = 0; k < n1; ++k) grad_scores[i * (size_t)n1 + (size_t)k] = (T)0;
    }
    if (grad_deltas)
      for (int k = 0; k < D; ++k) grad_deltas[i * (size_t)D + (size_t)k] = (T)0;
    if (fg) {
      const size_t b = i / (size_t)d->S;
      const int base = (d->flags & CLASS_AGNOSTIC) ? 0 : 4 * label;
      T tg[4], box = (T)0;
      target_deltas<T>(rois + i * 4, gt_boxes + (b * (size_t)d->M + (size_t)row) * 4, w, tg);
      for (int k = 0; k < 4; ++k) {
        T g;
        box = box + smooth_l1<T>(deltas[i * (size_t)D + (size_t)(base + k)] - tg[k], (T)d->beta, g);
        if (grad_deltas) grad_deltas[i * (size_t)D + (size_t)(base + k)] = kb * g;
      }
      row_box[i] = box;
    }
  }
  loss[0] = kernel_order_sum<T>(row_ce) / nr;
  loss[1] = kernel_order_sum<T>(row_box) / nr;
  loss[2] = (T)d->w_cls * loss[0] + (T)d->w_box * loss[1];
  return 0;
}

extern "C" int rh_loss_f32(const HostSpec* d, const float* scores, const float* deltas, const float* rois, const int32_t* labels,
                           const int32_t* gt_row, const float* gt_boxes, float* loss, float* grad_scores, float* grad_deltas) {
  return loss_run<float>(d, scores, deltas, rois, labels, gt_row, gt_boxes, loss, grad_scores, grad_deltas);
}

extern "C" int rh_loss_f64(const HostSpec* d, const double* scores, const double* deltas, const double* rois, const int32_t* labels,
                           const int32_t* gt_row, const double* gt_boxes, double* loss, double* grad_scores, double* grad_deltas) {
  return loss_run<double>(d, scores, deltas, rois, labels, gt_row, gt_boxes, loss, grad_scores, grad_deltas);
}

extern "C" int rh_post(const HostSpec* d, const float* scores, const float* deltas, const float* proposals, const int32_t* n_prop,
                       float* dets, int32_t* counts) {
  if (!d || d->B < 1 || d->R < 1 || d->R > MAX_CAND || d->C < 1 || d->max_det < 1 || d->max_det > d->R) return 1;
  const int R = d->R, C = d->C, n1 = C + 1, D = (d->flags & CLASS_AGNOSTIC) ? 4 : 4 * C;
  const float w[4] = {d->bw_x, d->bw_y, d->bw_w, d->bw_h};
  struct Cand { float box[4], score; int cls; };
  for (int b = 0; b < d->B; ++b) {
    const int np = n_prop ? clampi(n_prop[b], 0, R) : R;
    std::vector<Cand> cand;
    for (int i = 0; i < np; ++i) {
      const size_t q = (size_t)b * (size_t)R + (size_t)i;
      const float* x = scores + q * (size_t)n1;
      float mx, sm, bp = -INFINITY;
      int bc = 0x7fffffff;
      softmax_stats<float>(x, n1, mx, sm);
      for (int c = 0; c < C; ++c) {
        const float p = softmax_prob<float>(x[c], mx, sm);
        if (score_better<float>(p, c, bp, bc)) { bp = p; bc = c; }
      }
      if (!(bp > d->conf_thr)) continue;
      Cand k;
      apply_deltas<float>(proposals + q * 4, deltas + q * (size_t)D + ((d->flags & CLASS_AGNOSTIC) ? 0 : (size_t)4 * (size_t)bc), w, d->img_w,
                          d->img_h, k.box);
      if (!roi_finite<float>(k.box)) continue;
      k.score = bp;
      k.cls = bc;
      cand.push_back(k);
    }
    const int n = (int)cand.size();
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int c) {
      return gsr_detect::composite(cand[(size_t)a].score, a) < gsr_detect::composite(cand[(size_t)c].score, c);
    });
    std::vector<int> kept;
    for (int j = 0; j < n && (int)kept.size() < d->max_det; ++j) {
      const Cand& c = cand[(size_t)order[(size_t)j]];
      const gsr_detect::Box cb = gsr_detect::decode_box(c.box[0], c.box[1], c.box[2], c.box[3], 1);
      bool dead = false;
      for (int k : kept) {
        const Cand& e = cand[(size_t)k];
        const gsr_detect::Box eb = gsr_detect::decode_box(e.box[0], e.box[1], e.box[2], e.box[3], 1);
        if (gsr_detect::suppresses(eb, gsr_detect::box_area(eb), e.cls, cb, gsr_detect::box_area(cb), c.cls, d->iou_thr, false)) { dead = true; break; }
      }
      if (!dead) kept.push_back(order[(size_t)j]);
    }
    float* out = dets + (size_t)b * (size_t)d->max_det * 6;
    for (int j = 0; j < d->max_det; ++j) {
      float* row = out + (size_t)j * 6;
      if (j < (int)kept.size()) {
        const Cand& c = cand[(size_t)kept[(size_t)j]];
        for (int k = 0; k < 4; ++k) row[k] = c.box[k];
        row[4] = c.score;
        row[5] = (float)c.cls;
      } else {
        for (int k = 0; k < 6; ++k) row[k] = 0.0f;
      }
    }
    counts[(size_t)b * 2] = (int)kept.size();
    counts[(size_t)b * 2 + 1] = n;
  }
  return 0;
}
