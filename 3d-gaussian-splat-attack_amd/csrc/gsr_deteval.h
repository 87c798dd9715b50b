// gsr_deteval.h -- the scalar side of the detection metrics (gsr_deteval_match / gsr_deteval_accumulate /
// gsr_deteval_summarize of include/gsraster.h): COCOeval's evaluateImg, accumulate and summarize for boxes, restated so that
// every number is one IEEE double operation in a fixed order.
//
// One source, compiled twice: by hipcc into the kernels of gsr_deteval.hip.h and by g++ into a host harness
// (tests/host_math/deteval_host.cpp) that runs the stage in plain loops.  Everything is DOUBLE: float32 inputs are widened
// once, every function that rounds is GSR_FP_STRICT (no contraction), and no library call takes part, so both builds and the
// NumPy oracle (tests/deteval_cases.py) give the same bits.
//
// Rows are x1 y1 x2 y2.  A detection row is live iff it lies below counts[b, 0] (clamped to 0..D), none of its six floats is a
// NaN and its class float is an integer in 0..K-1; a ground-truth row is live iff its class is in 0..K-1 and its box holds no
// NaN.  Dead rows take no part anywhere.  Deviations from COCOeval, all stated in INTEGRATION.md section 8q: a NaN IoU counts
// as 0 (COCOeval would match it), no crowd and no `ignore` flags, and the caps / area ranges of the summary are taken by
// position, not by value.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gsr_math.h"   // GSR_HD, GSR_FP_STRICT

namespace gsr_de {

constexpr int MAX_D = 4096;          // detections per image
constexpr int MAX_M = 256;           // ground-truth rows per image
constexpr int MAX_T = 10;            // IoU thresholds
constexpr int MAX_A = 4;             // area ranges
constexpr int MAX_K = 65535;         // classes
constexpr int MAX_CAPS = 3;          // max_dets
constexpr int MAX_R = 1024;          // recall thresholds
constexpr long long MAX_ROWS = 1ll << 20;   // N * D of one accumulate
constexpr int MATCH_THREADS = 256;
constexpr int ACC_CHUNK = 64;        // the elements of a class segment one step of the curve kernel's scans covers (one wave)
constexpr int N_STATS = 14;
constexpr int FIELD_BITS = 21;       // tp | fp << 21 | nd << 42 travel through one 64-bit scan: each is at most 2^20

// GsrDetEvalSpec of include/gsraster.h, member for member
struct Spec {
  int32_t K, D, M, T, A, n_caps;
  int32_t caps[MAX_CAPS];
  int32_t R;
  double iou[MAX_T];
  double lo[MAX_A], hi[MAX_A];
};

GSR_HD bool is_nan(float v) { return v != v; }

// the class of a detection row of six floats, or -1 for a dead one
GSR_HD int det_class(const float* row, int K) {
  for (int i = 0; i < 6; ++i)
    if (is_nan(row[i])) return -1;
  const float c = row[5];
  if (!(c >= 0.0f) || !(c < (float)K)) return -1;
  const int k = (int)c;
  return (float)k == c ? k : -1;
}

// the class of a ground-truth row, or -1 for a dead one
GSR_HD int gt_class(const float* box, int cls, int K) {
  if (cls < 0 || cls >= K) return -1;
  for (int i = 0; i < 4; ++i)
    if (is_nan(box[i])) return -1;
  return cls;
}

// ascending in this key = descending in the score; -0 and +0 share a key.  (Scores are never NaN here: such rows are dead.)
GSR_HD uint32_t score_key(float s) {
  uint32_t u = 0u;
  if (!(s == 0.0f)) __builtin_memcpy(&u, &s, 4);
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

GSR_HD void widen4(const float* b, double* o) {
  o[0] = (double)b[0]; o[1] = (double)b[1]; o[2] = (double)b[2]; o[3] = (double)b[3];
}

GSR_HD double area(const double* b) {
  GSR_FP_STRICT
  return (b[2] - b[0]) * (b[3] - b[1]);
}

GSR_HD bool outside(double ar, double lo, double hi) { return ar < lo || ar > hi; }

// a NaN counts as 0
GSR_HD double iou(const double* d, double area_d, const double* g, double area_g) {
  GSR_FP_STRICT
  const double iw = (d[2] < g[2] ? d[2] : g[2]) - (d[0] > g[0] ? d[0] : g[0]);
  const double ih = (d[3] < g[3] ? d[3] : g[3]) - (d[1] > g[1] ? d[1] : g[1]);
  const double inter = (iw <= 0.0 || ih <= 0.0) ? 0.0 : iw * ih;
  const double v = inter / ((area_d + area_g) - inter);
  return v != v ? 0.0 : v;
}

GSR_HD bool bit_get(const uint32_t* bits, int g) { return (bits[g >> 5] >> (g & 31)) & 1u; }
GSR_HD void bit_set(uint32_t* bits, int g) { bits[g >> 5] |= 1u << (g & 31); }

// COCOeval.evaluateImg's inner loop for one detection under one (area range, threshold): the ground truth of the
// detection's class, counted rows first and ignored rows after them, each part in row order.  gcls[g]: the row's class, -1
// for a dead row; gign[g]: 0 counted, 1 ignored by area, 2 dead.  -> the matched row (its bit set in `matched`) or -1.
GSR_HD int walk(const double* db, double area_d, int dc, const double* gbox, const double* garea, const int32_t* gcls,
                const uint8_t* gign, int M, uint32_t* matched, double thr) {
  const double cap = 1.0 - 1e-10;
  double best = thr < cap ? thr : cap;
  int m = -1;
  for (int part = 0; part < 2; ++part) {
    if (part == 1 && m >= 0) break;                // a counted row is matched and every row from here on is ignored: stop
    for (int g = 0; g < M; ++g) {
      if (gcls[g] != dc || (int)gign[g] != part) continue;
      if (bit_get(matched, g)) continue;
      const double v = iou(db, area_d, gbox + 4 * g, garea[g]);
      if (v < best) continue;
      best = v;                                    // (>=: a later row of equal IoU replaces an earlier one)
      m = g;
    }
  }
  if (m >= 0) bit_set(matched, m);
  return m;
}

GSR_HD double recall_at(long long tp, long long npig) {
  GSR_FP_STRICT
  return (double)tp / (double)npig;
}

GSR_HD double precision_at(long long tp, long long fp) {
  GSR_FP_STRICT
  return (double)tp / (((double)fp + (double)tp) + 2.220446049250313e-16);
}

// element strides of the outputs: precision / scores [T,R,K,A,Mx], recall [T,K,A,Mx]
GSR_HD size_t prec_index(const Spec& s, int t, int r, int k, int a, int m) {
  return ((((size_t)t * (size_t)s.R + (size_t)r) * (size_t)s.K + (size_t)k) * (size_t)s.A + (size_t)a) * (size_t)s.n_caps + (size_t)m;
}
GSR_HD size_t rec_index(const Spec& s, int t, int k, int a, int m) {
  return (((size_t)t * (size_t)s.K + (size_t)k) * (size_t)s.A + (size_t)a) * (size_t)s.n_caps + (size_t)m;
}

// One of the 14 statistics: the mean over precision[t0 .. t1, :, :, a, m] (ap) or recall[t0 .. t1, :, a, m] of the entries
// above -1, or -1 when the slice is empty.  0..11 are COCOeval.summarize's, 12 and 13 the reference's AP (all areas, last cap)
// and AR (all areas, first cap).  Area ranges and caps go by position: all, small, medium, large; AR's caps are 0, 1, 2.
struct StatSel {
  int ap, t0, t1, a, m;          // t0 >= t1: nothing to average
};

GSR_HD int find_thr(const Spec& s, double v) {
  for (int t = 0; t < s.T; ++t)
    if (s.iou[t] == v) return t;
  return -1;
}

GSR_HD StatSel stat_sel(int i, const Spec& s) {
  const int last = s.n_caps - 1;
  StatSel r = {1, 0, s.T, 0, last};
  switch (i) {
    case 0: case 12: break;
    case 1: case 2: {
      const int t = find_thr(s, i == 1 ? 0.5 : 0.75);
      r.t0 = t; r.t1 = t < 0 ? t : t + 1;
      break;
    }
    case 3: case 4: case 5: r.a = i - 2; break;
    case 6: case 7: case 8: r.ap = 0; r.m = i - 6; break;
    case 9: case 10: case 11: r.ap = 0; r.a = i - 8; break;
    default: r.ap = 0; r.m = 0; break;             // 13
  }
  if (r.a >= s.A || r.m >= s.n_caps) r.t1 = r.t0;
  return r;
}

// the number of entries of a statistic's slice, and the element of its e-th entry in index order
GSR_HD long long stat_entries(const Spec& s, const StatSel& q) {
  if (q.t1 <= q.t0) return 0;
  return (long long)(q.t1 - q.t0) * (long long)(q.ap ? s.R : 1) * (long long)s.K;
}
GSR_HD size_t stat_element(const Spec& s, const StatSel& q, uint32_t e) {    // (at most 10 * 1024 * 65535 entries: 32-bit divisions)
  const uint32_t K = (uint32_t)s.K, R = (uint32_t)s.R;
  const int k = (int)(e % K);
  const uint32_t u = e / K;
  if (q.ap) return prec_index(s, q.t0 + (int)(u / R), (int)(u % R), k, q.a, q.m);
  return rec_index(s, q.t0 + (int)u, k, q.a, q.m);
}

// why a spec is refused, or null.  Thresholds and area bounds may be any doubles but NaN.
inline const char* spec_error(const Spec& s) {
  if (s.K < 1 || s.K > MAX_K) return "K (1..65535 classes)";
  if (s.D < 1 || s.D > MAX_D) return "D (1..4096 detections per image)";
  if (s.M < 0 || s.M > MAX_M) return "M (0..256 ground-truth rows per image)";
  if (s.T < 1 || s.T > MAX_T) return "T (1..10 IoU thresholds)";
  if (s.A < 1 || s.A > MAX_A) return "A (1..4 area ranges)";
  if (s.n_caps < 1 || s.n_caps > MAX_CAPS) return "n_caps (1..3 max_dets)";
  if (s.R < 1 || s.R > MAX_R) return "R (1..1024 recall thresholds)";
  for (int m = 0; m < s.n_caps; ++m) {
    if (s.caps[m] < 1 || s.caps[m] > s.D) return "max_dets (each 1..D)";
    if (m > 0 && s.caps[m] < s.caps[m - 1]) return "max_dets (ascending)";
  }
  for (int t = 0; t < s.T; ++t)
    if (s.iou[t] != s.iou[t]) return "iou_thrs (a NaN)";
  for (int a = 0; a < s.A; ++a)
    if (s.lo[a] != s.lo[a] || s.hi[a] != s.hi[a]) return "area bounds (a NaN)";
  return nullptr;
}

}  // namespace gsr_de
