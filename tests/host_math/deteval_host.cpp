// The detection metrics on the CPU, from csrc/gsr_deteval.h -- the scalar source the HIP kernels compile -- in plain loops.
//   deh_match       gsr_deteval_match's arguments without the stream
//   deh_accumulate  gsr_deteval_accumulate without workspace and stream
//   deh_summarize   gsr_deteval_summarize without the stream
//   deh_limits      the header's constants, for the tests: ACC_CHUNK, MAX_D, MAX_M, MAX_T, MAX_A, MAX_K, MAX_R, MAX_ROWS
//   deh_iou, deh_score_key   the scalars
// Every entry returns 0, or 1 for a refusal (the same ones as the library's).
// Build: g++ -O1 -ffp-contract=off -shared -fPIC -I <csrc> deteval_host.cpp -o libdetevalhost.so
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "gsr_deteval.h"

using namespace gsr_de;

extern "C" void deh_limits(int64_t* out8) {
  out8[0] = ACC_CHUNK; out8[1] = MAX_D; out8[2] = MAX_M; out8[3] = MAX_T; out8[4] = MAX_A; out8[5] = MAX_K; out8[6] = MAX_R; out8[7] = MAX_ROWS;
}

extern "C" double deh_iou(const float* d, const float* g) {
  double a[4], b[4];
  widen4(d, a);
  widen4(g, b);
  return iou(a, area(a), b, area(b));
}

extern "C" uint32_t deh_score_key(float s) { return score_key(s); }

extern "C" int deh_match(const Spec* sp, int32_t B, const float* dets, const int32_t* counts, const float* gt_boxes, const int32_t* gt_cls,
                         int32_t* dt_order, int32_t* dt_rank, int32_t* dt_match, uint8_t* dt_ignore, uint8_t* gt_ignore, int32_t* gt_match) {
  if (!sp || spec_error(*sp)) return 1;
  const Spec& s = *sp;
  const int D = s.D, M = s.M, A = s.A, T = s.T;
  if (B < 1 || (long long)B * D > MAX_ROWS) return 1;
  if (!dets || !counts || !dt_order || !dt_rank || !dt_match || !dt_ignore) return 1;
  if (M > 0 && (!gt_boxes || !gt_cls || !gt_ignore || !gt_match)) return 1;
  std::vector<double> gbox((size_t)M * 4 + 4), garea((size_t)M + 1);
  std::vector<int32_t> gcls((size_t)M + 1);
  std::vector<uint8_t> gign((size_t)M + 1);
  for (int b = 0; b < B; ++b) {
    const float* img = dets + (size_t)b * D * 6;
    const int cnt = std::min(std::max(counts[2 * b], 0), D);
    std::vector<uint64_t> keys;
    for (int i = 0; i < cnt; ++i)
      if (det_class(img + (size_t)i * 6, s.K) >= 0) keys.push_back(((uint64_t)score_key(img[(size_t)i * 6 + 4]) << 32) | (uint64_t)i);
    std::sort(keys.begin(), keys.end());
    const int nlive = (int)keys.size();
    std::vector<int> cls(nlive);
    for (int j = 0; j < D; ++j) {
      const int row = j < nlive ? (int)(uint32_t)keys[j] : -1;
      dt_order[(size_t)b * D + j] = row;
      int r = -1;
      if (row >= 0) {
        cls[j] = (int)img[(size_t)row * 6 + 5];
        r = 0;
        for (int q = 0; q < j; ++q) r += cls[q] == cls[j];
      }
      dt_rank[(size_t)b * D + j] = r;
    }
    for (int g = 0; g < M; ++g) {
      const float* box = gt_boxes + ((size_t)b * M + g) * 4;
      gcls[g] = gt_class(box, gt_cls[(size_t)b * M + g], s.K);
      widen4(box, &gbox[4 * (size_t)g]);
      garea[g] = area(&gbox[4 * (size_t)g]);
    }
    for (int a = 0; a < A; ++a) {
      for (int g = 0; g < M; ++g) {
        gign[g] = gcls[g] < 0 ? 2 : (outside(garea[g], s.lo[a], s.hi[a]) ? 1 : 0);
        gt_ignore[((size_t)b * A + a) * M + g] = gign[g];
      }
      for (int t = 0; t < T; ++t) {
        const size_t at = ((size_t)b * A + a) * T + t;
        uint32_t matched[MAX_M / 32] = {0};
        for (int g = 0; g < M; ++g) gt_match[at * M + g] = -1;
        for (int j = 0; j < D; ++j) {
          int m = -1;
          uint8_t ig = 0;
          if (j < nlive) {
            double db[4];
            widen4(img + (size_t)(uint32_t)keys[j] * 6, db);
            const double ad = area(db);
            m = walk(db, ad, cls[j], gbox.data(), garea.data(), gcls.data(), gign.data(), M, matched, s.iou[t]);
            ig = m >= 0 ? gign[m] : (uint8_t)(outside(ad, s.lo[a], s.hi[a]) ? 1 : 0);
            if (m >= 0) gt_match[at * M + m] = j;
          }
          dt_match[at * D + j] = m;
          dt_ignore[at * D + j] = ig;
        }
      }
    }
  }
  return 0;
}

extern "C" int deh_accumulate(const Spec* sp, int64_t N, const float* dets, const int32_t* dt_order, const int32_t* dt_rank,
                              const int32_t* dt_match, const uint8_t* dt_ignore, const int32_t* gt_cls, const uint8_t* gt_ignore,
                              const double* rec_thrs, double* precision, double* scores, double* recall, int32_t* npig) {
  if (!sp || spec_error(*sp)) return 1;
  const Spec& s = *sp;
  const int D = s.D, M = s.M, A = s.A, T = s.T, K = s.K, R = s.R, Mx = s.n_caps;
  if (N < 1 || N * D > MAX_ROWS) return 1;
  if (!dets || !dt_order || !dt_rank || !dt_match || !dt_ignore || !rec_thrs || !precision || !scores || !recall || !npig) return 1;
  if (M > 0 && (!gt_cls || !gt_ignore)) return 1;
  std::fill(npig, npig + (size_t)K * A, 0);
  for (int64_t n = 0; n < N; ++n)
    for (int a = 0; a < A; ++a)
      for (int g = 0; g < M; ++g)
        if (gt_ignore[((size_t)n * A + a) * M + g] == 0) {
          const int k = gt_cls[(size_t)n * M + g];
          if (k >= 0 && k < K) ++npig[(size_t)k * A + a];
        }
  // per class, the elements (image * D + position) by score descending, then image, then rank (= position order)
  struct El { uint32_t key, e; };
  std::vector<std::vector<El>> seg(K);
  for (int64_t e = 0; e < N * D; ++e) {
    const int row = dt_order[e];
    if (row < 0) continue;
    const float* r = dets + ((size_t)(e / D) * D + (size_t)row) * 6;
    seg[(int)r[5]].push_back({score_key(r[4]), (uint32_t)e});
  }
  for (auto& v : seg) std::stable_sort(v.begin(), v.end(), [](const El& x, const El& y) { return x.key < y.key; });
  std::vector<double> rc, pr, sc;
  for (int k = 0; k < K; ++k)
    for (int a = 0; a < A; ++a)
      for (int m = 0; m < Mx; ++m)
        for (int t = 0; t < T; ++t) {
          const long long np = npig[(size_t)k * A + a];
          if (np == 0) {
            for (int r = 0; r < R; ++r) precision[prec_index(s, t, r, k, a, m)] = scores[prec_index(s, t, r, k, a, m)] = -1.0;
            recall[rec_index(s, t, k, a, m)] = -1.0;
            continue;
          }
          rc.clear(); pr.clear(); sc.clear();
          long long tp = 0, fp = 0;
          for (const El& el : seg[k]) {
            if (dt_rank[el.e] >= s.caps[m]) continue;
            const size_t img = el.e / (uint32_t)D, j = el.e % (uint32_t)D;
            const size_t o = ((img * A + a) * T + t) * (size_t)D + j;
            if (dt_ignore[o] == 0) (dt_match[o] >= 0 ? tp : fp) += 1;
            rc.push_back(recall_at(tp, np));
            pr.push_back(precision_at(tp, fp));
            sc.push_back((double)dets[(img * D + (size_t)dt_order[el.e]) * 6 + 4]);
          }
          const size_t nd = rc.size();
          recall[rec_index(s, t, k, a, m)] = nd ? rc[nd - 1] : 0.0;
          for (size_t i = nd; i-- > 1;)
            if (pr[i] > pr[i - 1]) pr[i - 1] = pr[i];
          for (int r = 0; r < R; ++r) {
            size_t i = 0;
            while (i < nd && !(rc[i] >= rec_thrs[r])) ++i;
            precision[prec_index(s, t, r, k, a, m)] = i < nd ? pr[i] : 0.0;
            scores[prec_index(s, t, r, k, a, m)] = i < nd ? sc[i] : 0.0;
          }
        }
  return 0;
}

extern "C" int deh_summarize(const Spec* sp, const double* precision, const double* recall, double* stats) {
  if (!sp || spec_error(*sp) || !precision || !recall || !stats) return 1;
  for (int i = 0; i < N_STATS; ++i) {
    const StatSel q = stat_sel(i, *sp);
    const double* src = q.ap ? precision : recall;
    const long long n = stat_entries(*sp, q);
    double sum = 0.0;
    long long cnt = 0;
    for (long long e = 0; e < n; ++e) {
      const double x = src[stat_element(*sp, q, (uint32_t)e)];
      if (x > -1.0) { sum = sum + x; ++cnt; }
    }
    stats[i] = cnt > 0 ? sum / (double)cnt : -1.0;
  }
  return 0;
}
