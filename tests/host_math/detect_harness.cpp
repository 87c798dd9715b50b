// Stand-alone run of the detector output stage's host build on small shapes, for a build with
// -fsanitize=address,undefined: every buffer is exactly as large as the shape says, so an index outside a tensor is
// reported.  Also checks what must hold whatever the numbers: kept <= above_thr, kept <= max_det, scores descending,
// zero rows behind the kept ones.  Prints "detect_harness ok" and returns 0.
#include <cmath>
#include <cstdio>
#include <vector>

#include "detect_host.cpp"

namespace {

float noise(uint32_t& s) {
  s = s * 1664525u + 1013904223u;
  return (float)(s >> 8) * (1.0f / 16777216.0f);
}

int run(int B, int A, int C, int layout, int has_obj, int box_format, int maxc, int max_det, uint32_t flags) {
  Spec sp;
  sp.B = B; sp.A = A; sp.C = C; sp.layout = layout; sp.has_obj = has_obj; sp.box_format = box_format;
  sp.conf_thr = 0.3f; sp.iou_thr = 0.45f; sp.max_candidates = maxc; sp.max_det = max_det; sp.flags = flags;
  sp.ox = 2.0f; sp.oy = 3.0f; sp.sx = 1.5f; sp.sy = 0.5f;
  const int K = gsr_detect::channels(sp);
  uint32_t seed = 99u + (uint32_t)(A * 17 + C);
  std::vector<float> pred((size_t)B * A * K), dets((size_t)B * max_det * 6), best((size_t)B * 4), gt((size_t)B * 4);
  std::vector<int32_t> counts((size_t)B * 2), verdict((size_t)B);
  for (int b = 0; b < B; ++b)
    for (int a = 0; a < A; ++a)
      for (int k = 0; k < K; ++k) {
        float v = noise(seed);
        if (k < 4) v = (box_format == 0 || k < 2) ? 20.0f + 10.0f * v + (k >= 2 ? 10.0f : 40.0f * (float)(a % 5)) : 0.0f;
        pred[gsr_detect::pred_index(sp, b, a, k)] = v;
      }
  if (box_format == 1)
    for (int b = 0; b < B; ++b)
      for (int a = 0; a < A; ++a)
        for (int k = 2; k < 4; ++k)
          pred[gsr_detect::pred_index(sp, b, a, k)] = pred[gsr_detect::pred_index(sp, b, a, k - 2)] + 25.0f + 5.0f * noise(seed);
  if (dh_postprocess(&sp, pred.data(), dets.data(), counts.data())) return 1;
  for (int b = 0; b < B; ++b) {
    const int kept = counts[2 * b], above = counts[2 * b + 1];
    if (kept < 0 || kept > max_det || kept > above || above > A) return 2;
    for (int r = 0; r < max_det; ++r) {
      const float* d = dets.data() + ((size_t)b * max_det + r) * 6;
      if (r >= kept) {
        for (int i = 0; i < 6; ++i) if (d[i] != 0.0f) return 3;
      } else {
        if (!(d[4] > sp.conf_thr) || d[5] < 0.0f || d[5] >= (float)C) return 4;
        if (r > 0 && d[4] > d[-2]) return 5;
      }
    }
    gt[b * 4 + 0] = 20.0f; gt[b * 4 + 1] = 10.0f; gt[b * 4 + 2] = 60.0f; gt[b * 4 + 3] = 30.0f;
  }
  gt[0] = NAN;
  if (dh_verdict(dets.data(), counts.data(), B, max_det, gt.data(), 0, 1, 1, 0.5f, verdict.data(), best.data())) return 6;
  if (dh_verdict(dets.data(), counts.data(), B, max_det, nullptr, 0, -1, 0, 0.5f, verdict.data(), best.data())) return 7;
  // the same boxes through the nms entry and box_iou
  const int n = A < 64 ? A : 64;
  std::vector<float> boxes((size_t)B * n * 4), scores((size_t)B * n), ious((size_t)n * n);
  std::vector<int32_t> classes((size_t)B * n), nv((size_t)B), keep((size_t)B * n), cnt((size_t)B);
  for (int b = 0; b < B; ++b) {
    nv[b] = b == 0 ? n : n / 2;
    for (int a = 0; a < n; ++a) {
      const Box q = gsr_detect::load_box(sp, pred.data(), b, a);
      float* o = boxes.data() + ((size_t)b * n + a) * 4;
      o[0] = q.x1; o[1] = q.y1; o[2] = q.x2; o[3] = q.y2;
      scores[(size_t)b * n + a] = noise(seed);
      classes[(size_t)b * n + a] = a % 3;
    }
  }
  if (dh_nms(B, n, boxes.data(), scores.data(), classes.data(), nv.data(), 0.45f, n, keep.data(), cnt.data())) return 8;
  if (dh_nms(B, n, boxes.data(), scores.data(), nullptr, nullptr, 0.45f, 1, keep.data(), cnt.data())) return 9;
  if (dh_box_iou(boxes.data(), n, boxes.data(), n, ious.data())) return 10;
  for (int i = 0; i < n; ++i)
    if (std::fabs(ious[(size_t)i * n + i] - 1.0f) > 1e-6f) return 11;
  return 0;
}

}  // namespace

int main() {
  const int shapes[][3] = {{1, 1, 1}, {2, 63, 3}, {3, 130, 80}};
  for (const auto& q : shapes)
    for (int mode = 0; mode < 16; ++mode) {
      const int rc = run(q[0], q[1], q[2], mode & 1, (mode >> 1) & 1, (mode >> 2) & 1, q[1] > 20 ? 20 : q[1],
                         q[1] > 7 ? 7 : q[1], (mode >> 3) & 1);
      if (rc) {
        std::fprintf(stderr, "detect_harness: B=%d A=%d C=%d mode=%d failed with %d\n", q[0], q[1], q[2], mode, rc);
        return 1;
      }
    }
  std::printf("detect_harness ok\n");
  return 0;
}
