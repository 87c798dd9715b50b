// The RPN loss stage in plain loops over csrc/gsr_rpnloss.h, the same scalar source the HIP kernels compile:
//   rlh_total    R, the anchors per image of a spec (0: a spec out of range)
//   rlh_label    what gsr_rpnloss_label computes: pre-labels, labels, matched rows, counts -- integers, equal to the kernels'.
//                The quota-th composite of a kind comes from std::nth_element, not from a radix select.
//   rlh_loss32   what gsr_rpnloss computes, anchor by anchor in flat index order, in float, the terms added pairwise (halves
//   rlh_loss64   of halves: a different order of the same sums as the kernels' blocks and slab), and the same code in
//                double; both hand their results back as doubles
// Build: g++ -O1 -ffp-contract=off -shared -fPIC -I <csrc> rpnloss_host.cpp -o librpnlosshost.so
#include <algorithm>
#include <cstdint>
#include <vector>

#include "gsr_rpnloss.h"

using namespace gsr_rpnl;
typedef gsr_rpnl::Spec RSpec;   // GsrRpnLossSpec of include/gsraster.h, field for field

static long long spec_total(const RSpec* d, int32_t* off) {
  if (!d || d->B < 1 || d->M < 1 || d->M > MAX_ROWS || d->nl < 1 || d->nl > MAX_LEVELS || d->batch_per_image < 1 || d->pos_quota < 0 ||
      d->pos_quota > d->batch_per_image)
    return 0;
  for (int l = 0; l < d->nl; ++l)
    if (d->A[l] < 1 || d->Hf[l] < 1 || d->Wf[l] < 1 || d->stride[l] < 1 || (long long)d->A[l] * d->Hf[l] * d->Wf[l] > MAX_ANCHORS) return 0;
  const long long R = level_offsets(*d, off);
  return R <= MAX_ANCHORS ? R : 0;
}

extern "C" int rlh_total(const RSpec* d) {
  int32_t off[MAX_LEVELS + 1];
  return (int)spec_total(d, off);
}

static uint64_t kth(std::vector<uint64_t>& v, int n) {       // the n-th smallest, 1 <= n < size
  std::nth_element(v.begin(), v.begin() + (n - 1), v.end());
  return v[(size_t)n - 1];
}

extern "C" int rlh_label(const RSpec* d, const float* const* cells, const float* gt_boxes, const int32_t* gt_cls, int32_t* prelabels,
                         int32_t* labels, int32_t* matched, int32_t* counts) {
  int32_t off[MAX_LEVELS + 1];
  const int R = (int)spec_total(d, off);
  if (R < 1) return 1;
  const int M = d->M;
  std::vector<float> rowmax((size_t)M), anc((size_t)R * 4);
  std::vector<uint64_t> kind[2];
  for (int b = 0; b < d->B; ++b) {
    const float* gt = gt_boxes + (size_t)b * (size_t)M * 4;
    const int32_t* cls = gt_cls + (size_t)b * (size_t)M;
    int32_t* pre = prelabels + (size_t)b * (size_t)R;
    std::fill(rowmax.begin(), rowmax.end(), 0.0f);
    for (int r = 0; r < R; ++r) {
      anchor_of<float>(*d, off, cells, r, &anc[(size_t)r * 4]);
      for (int m = 0; m < M; ++m) {
        if (!row_present(cls[m])) continue;
        const float v = gsr_rcnn::pair_iou<float>(gt + (size_t)m * 4, &anc[(size_t)r * 4]);
        if (v > rowmax[m]) rowmax[m] = v;
      }
    }
    kind[0].clear(); kind[1].clear();
    for (int r = 0; r < R; ++r) {
      float best;
      int row;
      const bool promoted = match_anchor<float>(&anc[(size_t)r * 4], gt, cls, M, rowmax.data(), best, row);
      pre[r] = pre_label<float>(best, d->iou_lo, d->iou_hi, promoted);
      matched[(size_t)b * (size_t)R + (size_t)r] = row;
      if (pre[r] == 1) kind[0].push_back(composite(d->seed, b, r));
      if (pre[r] == 0) kind[1].push_back(composite(d->seed, b, r));
    }
    int n_pos, n_neg;
    quotas((int)kind[0].size(), (int)kind[1].size(), d->batch_per_image, d->pos_quota, n_pos, n_neg);
    const uint64_t thr_pos = (n_pos > 0 && n_pos < (int)kind[0].size()) ? kth(kind[0], n_pos) : TAKE_ALL;
    const uint64_t thr_neg = (n_neg > 0 && n_neg < (int)kind[1].size()) ? kth(kind[1], n_neg) : TAKE_ALL;
    for (int r = 0; r < R; ++r)
      labels[(size_t)b * (size_t)R + (size_t)r] = final_label(pre[r], composite(d->seed, b, r), n_pos, thr_pos, n_neg, thr_neg);
    int32_t* c = counts + (size_t)b * 4;
    c[0] = (int32_t)kind[0].size(); c[1] = (int32_t)kind[1].size(); c[2] = n_pos; c[3] = n_neg;
  }
  return 0;
}

template <class T>
static T pair_sum(const T* v, size_t n) {       // halves of halves, runs of 8 in index order
  if (n <= 8) {
    T s = (T)0;
    for (size_t i = 0; i < n; ++i) s = s + v[i];
    return s;
  }
  const size_t h = n / 2;
  return pair_sum<T>(v, h) + pair_sum<T>(v + h, n - h);
}

template <class T>
static int loss_walk(const RSpec* d, const int32_t* labels, const int32_t* matched, const float* const* logits, const float* const* deltas,
                     const float* const* cells, const float* gt_boxes, double* loss, double* const* grad_logits, double* const* grad_deltas) {
  int32_t off[MAX_LEVELS + 1];
  const int R = (int)spec_total(d, off);
  if (R < 1) return 1;
  const T norm = (T)(float)((long long)d->batch_per_image * (long long)d->B);
  const T k_cls = (T)d->w_cls / norm, k_loc = (T)d->w_loc / norm;
  std::vector<T> t_cls((size_t)d->B * (size_t)R), t_loc((size_t)d->B * (size_t)R);
  for (int b = 0; b < d->B; ++b)
    for (int r = 0; r < R; ++r) {
      const int l = level_of(r, off);
      const int A = d->A[l], Wf = d->Wf[l], HW = d->Hf[l] * Wf;
      int a, x, y;
      gsr_rpn::split_index(r - off[l], A, Wf, a, x, y);
      const size_t p = (size_t)y * (size_t)Wf + (size_t)x;
      const size_t le = ((size_t)b * (size_t)A + (size_t)a) * (size_t)HW + p;
      const size_t de = ((size_t)b * (size_t)(4 * A) + (size_t)(4 * a)) * (size_t)HW + p;
      const size_t o = (size_t)b * (size_t)R + (size_t)r;
      const int label = labels[o];
      const bool sampled = label == 0 || label == 1;
      T anc[4], dl[4] = {(T)0, (T)0, (T)0, (T)0}, gt[4] = {(T)0, (T)0, (T)0, (T)0};
      bool located = false;
      anchor_of<T>(*d, off, cells, r, anc);
      const int m = matched[o];
      if (label == 1 && m >= 0 && m < d->M) {
        for (int k = 0; k < 4; ++k) {
          dl[k] = (T)deltas[l][de + (size_t)k * (size_t)HW];
          gt[k] = (T)gt_boxes[((size_t)b * (size_t)d->M + (size_t)m) * 4 + (size_t)k];
        }
        located = true;
      }
      T cls, loc, g_logit, g_d[4];
      anchor_terms<T>(label, located, sampled ? (T)logits[l][le] : (T)0, dl, anc, gt, (T)d->beta, cls, loc, g_logit, g_d);
      t_cls[o] = cls;
      t_loc[o] = loc;
      if (grad_logits) grad_logits[l][le] = sampled ? (double)(k_cls * g_logit) : 0.0;
      if (grad_deltas)
        for (int k = 0; k < 4; ++k) grad_deltas[l][de + (size_t)k * (size_t)HW] = located ? (double)(k_loc * g_d[k]) : 0.0;
    }
  T out[3];
  const T s_cls = pair_sum<T>(t_cls.data(), t_cls.size()), s_loc = pair_sum<T>(t_loc.data(), t_loc.size());
  finish<T>(s_cls, s_loc, (T)d->w_cls, (T)d->w_loc, norm, out);
  for (int k = 0; k < 3; ++k) loss[k] = (double)out[k];
  return 0;
}

extern "C" int rlh_loss32(const RSpec* d, const int32_t* labels, const int32_t* matched, const float* const* logits, const float* const* deltas,
                          const float* const* cells, const float* gt_boxes, double* loss, double* const* grad_logits, double* const* grad_deltas) {
  return loss_walk<float>(d, labels, matched, logits, deltas, cells, gt_boxes, loss, grad_logits, grad_deltas);
}

extern "C" int rlh_loss64(const RSpec* d, const int32_t* labels, const int32_t* matched, const float* const* logits, const float* const* deltas,
                          const float* const* cells, const float* gt_boxes, double* loss, double* const* grad_logits, double* const* grad_deltas) {
  return loss_walk<double>(d, labels, matched, logits, deltas, cells, gt_boxes, loss, grad_logits, grad_deltas);
}
