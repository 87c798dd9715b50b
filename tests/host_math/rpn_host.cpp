// The RPN proposal stage in plain loops over csrc/gsr_rpn.h, the same scalar source the HIP kernels compile:
//   ph_select   what gsr_rpn_select computes: a full sort of the (logit, index) keys, the first min(pre_topk, A*Hf*Wf) ranks
//               decoded into their slots; rank_index [B, that many] also receives the candidate index of every rank (-1:
//               unused), which the C entry does not return
//   ph_nms      what gsr_rpn_nms computes: a full sort of the (score, slot) keys and the greedy walk, every box tested
//               against every kept box
// Build: g++ -O1 -ffp-contract=off -shared -fPIC -I <csrc> rpn_host.cpp -o librpnhost.so
#include <algorithm>
#include <cstdint>
#include <vector>

#include "gsr_rpn.h"

using namespace gsr_rpn;

struct HostSpec {   // GsrRpnSpec of include/gsraster.h
  int32_t B, A, Hf, Wf, stride;
  float shift0, img_w, img_h, min_size;
  int32_t pre_topk, level, cand_offset, N, post_topk;
  float iou_thr;
  uint32_t flags;
};

static Spec to_spec(const HostSpec* d) {
  Spec sp;
  sp.B = d->B; sp.A = d->A; sp.Hf = d->Hf; sp.Wf = d->Wf; sp.stride = d->stride; sp.shift0 = d->shift0; sp.img_w = d->img_w;
  sp.img_h = d->img_h; sp.min_size = d->min_size; sp.pre_topk = d->pre_topk; sp.level = d->level; sp.cand_offset = d->cand_offset;
  sp.N = d->N; sp.post_topk = d->post_topk; sp.iou_thr = d->iou_thr; sp.flags = d->flags;
  return sp;
}

extern "C" int ph_select(const HostSpec* d, const float* logits, const float* deltas, const float* cell_anchors, float* cand_boxes,
                         float* cand_scores, int32_t* cand_level, int32_t* rank_index) {
  if (!d || d->B < 1 || d->A < 1 || d->Hf < 1 || d->Wf < 1 || d->stride < 1 || d->pre_topk < 1 || d->N < 1 || d->N > MAX_SLOTS ||
      d->cand_offset < 0 || d->level < 0)
    return 1;
  const Spec sp = to_spec(d);
  const int A = d->A, HW = d->Hf * d->Wf, n_in = A * HW, slots = (int)level_slots(sp);
  if (d->cand_offset + slots > d->N) return 1;
  std::vector<uint64_t> keys;
  for (int b = 0; b < d->B; ++b) {
    const float* lg = logits + (size_t)b * (size_t)n_in;
    keys.clear();
    for (int i = 0; i < n_in; ++i) {
      int a, x, y;
      split_index(i, A, d->Wf, a, x, y);
      const float v = lg[(size_t)a * (size_t)HW + (size_t)(y * d->Wf + x)];
      if (!is_nan(v)) keys.push_back(order_key(v, i));
    }
    std::sort(keys.begin(), keys.end());
    for (int r = 0; r < slots; ++r) {
      const size_t o = (size_t)b * (size_t)d->N + (size_t)d->cand_offset + (size_t)r;
      float box[4] = {0.0f, 0.0f, 0.0f, 0.0f}, score = 0.0f;
      int level = -1, index = -1;
      if ((size_t)r < keys.size()) {
        index = (int)(uint32_t)keys[(size_t)r];
        int a, x, y;
        split_index(index, A, d->Wf, a, x, y);
        const size_t p = (size_t)(y * d->Wf + x);
        float anc[4], dl[4], out[4];
        for (int k = 0; k < 4; ++k) dl[k] = deltas[((size_t)b * (size_t)(4 * A) + (size_t)(4 * a + k)) * (size_t)HW + p];
        anchor_at<float>(cell_anchors + (size_t)a * 4, x, y, d->stride, d->shift0, anc);
        if (decode_candidate<float>(anc, dl, d->img_w, d->img_h, d->min_size, out)) {
          for (int k = 0; k < 4; ++k) box[k] = out[k];
          score = lg[(size_t)a * (size_t)HW + p];
          level = d->level;
        }
      }
      for (int k = 0; k < 4; ++k) cand_boxes[o * 4 + (size_t)k] = box[k];
      cand_scores[o] = score;
      cand_level[o] = level;
      if (rank_index) rank_index[(size_t)b * (size_t)slots + (size_t)r] = index;
    }
  }
  return 0;
}

extern "C" int ph_nms(const HostSpec* d, const float* cand_boxes, const float* cand_scores, const int32_t* cand_level, float* proposals,
                      float* scores, int32_t* keep, int32_t* counts) {
  if (!d || d->B < 1 || d->N < 1 || d->N > MAX_SLOTS || d->post_topk < 1 || d->post_topk > d->N || d->post_topk > MAX_POST) return 1;
  const int N = d->N, post = d->post_topk;
  std::vector<uint64_t> keys;
  std::vector<int> kept;
  for (int b = 0; b < d->B; ++b) {
    const float* bx = cand_boxes + (size_t)b * (size_t)N * 4;
    const float* sc = cand_scores + (size_t)b * (size_t)N;
    const int32_t* lv = cand_level + (size_t)b * (size_t)N;
    auto box = [&](int s) { return Box{bx[(size_t)s * 4], bx[(size_t)s * 4 + 1], bx[(size_t)s * 4 + 2], bx[(size_t)s * 4 + 3]}; };
    keys.clear();
    for (int s = 0; s < N; ++s)
      if (lv[s] >= 0 && !is_nan(sc[s])) keys.push_back(order_key(sc[s], s));
    std::sort(keys.begin(), keys.end());
    kept.clear();
    for (size_t q = 0; q < keys.size() && (int)kept.size() < post; ++q) {
      const int s = (int)(uint32_t)keys[q];
      const Box later = box(s);
      const float area = box_area(later);
      bool sup = false;
      for (size_t j = 0; j < kept.size() && !sup; ++j) {
        const Box kb = box(kept[j]);
        sup = suppresses(kb, box_area(kb), lv[kept[j]], later, area, lv[s], d->iou_thr);
      }
      if (!sup) kept.push_back(s);
    }
    for (int j = 0; j < post; ++j) {
      const size_t o = (size_t)b * (size_t)post + (size_t)j;
      const bool in = j < (int)kept.size();
      for (int k = 0; k < 4; ++k) proposals[o * 4 + (size_t)k] = in ? bx[(size_t)kept[(size_t)j] * 4 + (size_t)k] : 0.0f;
      scores[o] = in ? sc[kept[(size_t)j]] : 0.0f;
      keep[o] = in ? kept[(size_t)j] : -1;
    }
    counts[b] = (int32_t)kept.size();
  }
  return 0;
}
