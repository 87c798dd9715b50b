// Host build of csrc/gsr_detect.h: the detector output stage over whole tensors, the same scalar source the HIP
// kernels compile, in plain sequential loops.  g++ -O1 -ffp-contract=off -shared -fPIC (tests/detect_cases.py builds
// it); detect_harness.cpp includes this file and adds a main for the sanitised run.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "gsr_detect.h"

namespace {

using gsr_detect::Box;
using gsr_detect::Spec;

struct Entry {
  Box box;
  float area;
  int cls, anchor;
};

// the greedy walk over entries in order; returns the positions kept
std::vector<int> walk(const std::vector<Entry>& e, float iou_thr, bool agnostic, int max_det) {
  std::vector<int> kept;
  for (size_t j = 0; j < e.size() && (int)kept.size() < max_det; ++j) {
    bool dead = false;
    for (int i : kept)
      if (gsr_detect::suppresses(e[i].box, e[i].area, e[i].cls, e[j].box, e[j].area, e[j].cls, iou_thr, agnostic)) {
        dead = true;
        break;
      }
    if (!dead) kept.push_back((int)j);
  }
  return kept;
}

bool spec_ok(const Spec& sp) {
  return sp.B >= 1 && sp.A >= 1 && sp.C >= 1 && (sp.layout == 0 || sp.layout == 1) && (sp.has_obj == 0 || sp.has_obj == 1) &&
         (sp.box_format == 0 || sp.box_format == 1) && sp.max_candidates >= 1 && sp.max_candidates <= gsr_detect::MAX_CAND &&
         sp.max_det >= 1 && sp.max_det <= sp.max_candidates && (sp.flags & ~gsr_detect::CLASS_AGNOSTIC) == 0u;
}

}  // namespace

extern "C" {

// spec: the 15 fields of GsrDetSpec in order, as the C struct lays them out
int dh_postprocess(const Spec* spp, const float* pred, float* dets, int32_t* counts) {
  if (!spp || !spec_ok(*spp) || !pred || !dets || !counts) return 1;
  const Spec sp = *spp;
  const int K = gsr_detect::channels(sp);
  const bool agnostic = (sp.flags & gsr_detect::CLASS_AGNOSTIC) != 0u;
  for (int b = 0; b < sp.B; ++b) {
    std::vector<uint64_t> comp;
    std::vector<float> score(sp.A);
    std::vector<int> cls(sp.A);
    for (int a = 0; a < sp.A; ++a) {
      const float obj = sp.has_obj ? pred[gsr_detect::pred_index(sp, b, a, 4)] : 1.0f;
      const float* first = pred + gsr_detect::pred_index(sp, b, a, 4 + sp.has_obj);
      const size_t stride = sp.layout == 0 ? 1 : (size_t)sp.A;
      gsr_detect::anchor_best(first, stride, sp.C, obj, sp.has_obj, score[a], cls[a]);
      if (gsr_detect::is_candidate(score[a], sp.conf_thr)) comp.push_back(gsr_detect::composite(score[a], a));
    }
    (void)K;
    counts[2 * b + 1] = (int32_t)comp.size();
    std::sort(comp.begin(), comp.end());
    if ((int)comp.size() > sp.max_candidates) comp.resize(sp.max_candidates);
    std::vector<Entry> e(comp.size());
    for (size_t j = 0; j < comp.size(); ++j) {
      const int a = (int)(uint32_t)comp[j];
      e[j].box = gsr_detect::load_box(sp, pred, b, a);
      e[j].area = gsr_detect::box_area(e[j].box);
      e[j].cls = cls[a];
      e[j].anchor = a;
    }
    const std::vector<int> kept = walk(e, sp.iou_thr, agnostic, sp.max_det);
    counts[2 * b] = (int32_t)kept.size();
    float* d = dets + (size_t)b * sp.max_det * 6;
    for (int i = 0; i < sp.max_det * 6; ++i) d[i] = 0.0f;
    for (size_t r = 0; r < kept.size(); ++r) {
      const Entry& k = e[kept[r]];
      const Box o = gsr_detect::to_render_frame(k.box, sp.ox, sp.oy, sp.sx, sp.sy);
      d[r * 6 + 0] = o.x1; d[r * 6 + 1] = o.y1; d[r * 6 + 2] = o.x2; d[r * 6 + 3] = o.y2;
      d[r * 6 + 4] = score[k.anchor];
      d[r * 6 + 5] = (float)k.cls;
    }
  }
  return 0;
}

int dh_nms(int B, int n, const float* boxes, const float* scores, const int32_t* classes, const int32_t* n_valid,
           float iou_thr, int max_det, int32_t* keep, int32_t* counts) {
  if (B < 1 || n < 1 || n > gsr_detect::MAX_CAND || max_det < 1 || max_det > n || !boxes || !scores || !keep || !counts) return 1;
  for (int b = 0; b < B; ++b) {
    int nv = n_valid ? n_valid[b] : n;
    nv = nv < 0 ? 0 : nv > n ? n : nv;
    std::vector<uint64_t> comp;
    for (int a = 0; a < nv; ++a) comp.push_back(gsr_detect::composite(scores[(size_t)b * n + a], a));
    std::sort(comp.begin(), comp.end());
    std::vector<Entry> e(comp.size());
    for (size_t j = 0; j < comp.size(); ++j) {
      const int a = (int)(uint32_t)comp[j];
      const float* q = boxes + ((size_t)b * n + a) * 4;
      e[j].box = gsr_detect::decode_box(q[0], q[1], q[2], q[3], 1);
      e[j].area = gsr_detect::box_area(e[j].box);
      e[j].cls = classes ? classes[(size_t)b * n + a] : 0;
      e[j].anchor = a;
    }
    const std::vector<int> kept = walk(e, iou_thr, classes == nullptr, max_det);
    counts[b] = (int32_t)kept.size();
    for (int r = 0; r < max_det; ++r) keep[(size_t)b * max_det + r] = r < (int)kept.size() ? e[kept[r]].anchor : -1;
  }
  return 0;
}

int dh_box_iou(const float* a, int n, const float* b, int m, float* out) {
  if (n < 1 || m < 1 || !a || !b || !out) return 1;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < m; ++j) {
      const Box p = gsr_detect::decode_box(a[i * 4], a[i * 4 + 1], a[i * 4 + 2], a[i * 4 + 3], 1);
      const Box q = gsr_detect::decode_box(b[j * 4], b[j * 4 + 1], b[j * 4 + 2], b[j * 4 + 3], 1);
      out[(size_t)i * m + j] = gsr_detect::iou(p, gsr_detect::box_area(p), q, gsr_detect::box_area(q));
    }
  return 0;
}

int dh_verdict(const float* dets, const int32_t* counts, int B, int max_det, const float* gt, int target, int untarget,
               int is_targeted, float iou_match, int32_t* verdict, float* best) {
  if (B < 1 || max_det < 1 || !dets || !counts || !verdict || !best) return 1;
  if (untarget < 0) untarget = -1;
  for (int b = 0; b < B; ++b) {
    int n = counts[2 * b];
    n = n < 0 ? 0 : n > max_det ? max_det : n;
    const float* rows = dets + (size_t)b * max_det * 6;
    const float* g = gt ? gt + (size_t)b * 4 : nullptr;
    const bool has_gt = gsr_detect::gt_present(g);
    Box gb = {0.0f, 0.0f, 0.0f, 0.0f};
    float ga = 0.0f;
    if (has_gt) {
      gb.x1 = g[0]; gb.y1 = g[1]; gb.x2 = g[2]; gb.y2 = g[3];
      ga = gsr_detect::box_area(gb);
    }
    float bi = 0.0f;
    int bidx = -1;
    bool any_t = false, any_u = false;
    for (int i = 0; i < n; ++i) {
      const int c = (int)rows[i * 6 + 5];
      any_t = any_t || c == target;
      any_u = any_u || c == untarget;
      if (has_gt) {
        const float v = gsr_detect::verdict_iou(rows + i * 6, gb, ga);
        if (bidx < 0 || v > bi) { bi = v; bidx = i; }
      }
    }
    const bool has_best = has_gt && n > 0;
    const int bc = has_best ? (int)rows[bidx * 6 + 5] : -1;
    verdict[b] = gsr_detect::verdict_bits(has_best, bi, bc, any_t, any_u, n, target, untarget, is_targeted != 0, iou_match);
    float* o = best + (size_t)b * 4;
    if (has_best) {
      o[0] = bi; o[1] = rows[bidx * 6 + 4]; o[2] = (float)bc; o[3] = (float)bidx;
    } else {
      o[0] = o[1] = o[2] = o[3] = -1.0f;
    }
  }
  return 0;
}

// the header's small pieces on their own
uint32_t dh_score_key(float s) { return gsr_detect::score_key(s); }

}  // extern "C"
