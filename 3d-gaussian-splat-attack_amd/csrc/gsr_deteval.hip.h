// gsr_deteval.hip.h -- the detection metrics' kernels (gfx950), over the arithmetic of gsr_deteval.h.
//
//   k_de_match     one workgroup per image: the live rows sorted by (score descending, row) with block_sort_u64, the rank
//                  within image and class, the ground truth widened into LDS, then lane (a, t) of the first wave walks the
//                  detections in order -- the walk is sequential by definition -- with its matched set in LDS and the IoUs
//                  computed where they are needed
//   k_de_keys      per (image, position): the score key, the class (K for a dead position) and the class histogram
//   k_de_classes   the class of every value after the score sort, the key of the second (stable) sort
//   k_de_npig      the live, counted ground-truth rows per (class, area range)
//   k_de_curve     one wave per (class, area range, cap, threshold): tp / fp / list length of the class segment as ONE packed
//                  64-bit scan in steps of ACC_CHUNK from the back, the running maximum of the precision carried along, and
//                  every recall threshold settled at the element where the recall first reaches it -- no per-detection buffer
//   k_de_summarize one wave per statistic, the entries added in index order
//
// Integer atomics only (counts: the same totals in whatever order); every double is computed by one lane from integers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_block.hip.h"
#include "gsr_deteval.h"

namespace gsr_de {

__global__ void __launch_bounds__(MATCH_THREADS) k_de_match(const Spec s, const int P, const float* __restrict__ dets,
                                                            const int32_t* __restrict__ counts, const float* __restrict__ gt_boxes,
                                                            const int32_t* __restrict__ gt_cls, int32_t* __restrict__ dt_order,
                                                            int32_t* __restrict__ dt_rank, int32_t* __restrict__ dt_match,
                                                            uint8_t* __restrict__ dt_ignore, uint8_t* __restrict__ gt_ignore,
                                                            int32_t* __restrict__ gt_match) {
  extern __shared__ uint64_t s_key[];                        // P keys, then P classes (u16)
  uint16_t* s_cls = reinterpret_cast<uint16_t*>(s_key + P);
  __shared__ double s_gbox[MAX_M * 4], s_garea[MAX_M], s_lo[MAX_A], s_hi[MAX_A], s_iou[MAX_T];
  __shared__ int32_t s_gcls[MAX_M];
  __shared__ uint8_t s_gign[MAX_A][MAX_M];
  __shared__ uint32_t s_matched[MAX_A * MAX_T][MAX_M / 32];
  __shared__ int s_nlive;
  const int t = threadIdx.x, b = blockIdx.x, D = s.D, M = s.M, A = s.A, T = s.T;
  const float* img = dets + (size_t)b * (size_t)D * 6;
  int cnt = counts[2 * b];
  cnt = cnt < 0 ? 0 : (cnt > D ? D : cnt);
  if (t == 0) s_nlive = 0;
  if (t < MAX_A) { s_lo[t] = t < A ? s.lo[t] : 0.0; s_hi[t] = t < A ? s.hi[t] : 0.0; }
  if (t < MAX_T) s_iou[t] = t < T ? s.iou[t] : 0.0;
  __syncthreads();
  int mine = 0;
  for (int i = t; i < P; i += MATCH_THREADS) {
    uint64_t key = ~0ull;
    if (i < cnt && det_class(img + (size_t)i * 6, s.K) >= 0) {
      key = ((uint64_t)score_key(img[(size_t)i * 6 + 4]) << 32) | (uint64_t)(uint32_t)i;
      ++mine;
    }
    s_key[i] = key;
  }
  if (mine) atomicAdd(&s_nlive, mine);
  gsr_block::block_sort_u64<MATCH_THREADS>(s_key, P);       // (a barrier on either side)
  const int nlive = s_nlive;
  for (int j = t; j < D; j += MATCH_THREADS) {
    const int row = j < nlive ? (int)(uint32_t)s_key[j] : -1;
    dt_order[(size_t)b * D + j] = row;
    s_cls[j] = row >= 0 ? (uint16_t)(int)img[(size_t)row * 6 + 5] : (uint16_t)0xffff;
  }
  // the ground truth, widened once; every gt_match of the image starts at -1
  for (int g = t; g < M; g += MATCH_THREADS) {
    const float* box = gt_boxes + ((size_t)b * M + g) * 4;
    const int c = gt_class(box, gt_cls[(size_t)b * M + g], s.K);
    double w[4];
    widen4(box, w);
    const double ar = area(w);
    s_gcls[g] = c;
    s_garea[g] = ar;
    for (int i = 0; i < 4; ++i) s_gbox[4 * g + i] = w[i];
    for (int a = 0; a < A; ++a) {
      const uint8_t ig = c < 0 ? (uint8_t)2 : (uint8_t)(outside(ar, s_lo[a], s_hi[a]) ? 1 : 0);
      s_gign[a][g] = ig;
      gt_ignore[((size_t)b * A + a) * M + g] = ig;
    }
  }
  for (int i = t; i < A * T * M; i += MATCH_THREADS) gt_match[(size_t)b * A * T * M + i] = -1;
  __syncthreads();
  // the rank within image and class: the earlier positions of the same class
  for (int j = t; j < D; j += MATCH_THREADS) {
    int r = -1;
    if (j < nlive) {
      const uint16_t c = s_cls[j];
      r = 0;
      for (int q = 0; q < j; ++q) r += s_cls[q] == c ? 1 : 0;
    }
    dt_rank[(size_t)b * D + j] = r;
  }
  // beyond the live rows: no match, not ignored
  const int dead = D - nlive;
  for (int i = t; i < A * T * dead; i += MATCH_THREADS) {
    const size_t o = ((size_t)b * A * T + (size_t)(i / dead)) * D + (size_t)(nlive + i % dead);
    dt_match[o] = -1;
    dt_ignore[o] = 0;
  }
  if (t >= A * T) return;
  // ---- the walk: lane (a, ti), detections in order
  const int a = t / T, ti = t % T;
  uint32_t* matched = s_matched[t];
  for (int i = 0; i < MAX_M / 32; ++i) matched[i] = 0u;
  const double thr = s_iou[ti], lo = s_lo[a], hi = s_hi[a];
  const size_t at = ((size_t)b * A + a) * T + ti;
  for (int j = 0; j < nlive; ++j) {
    const float* row = img + (size_t)(uint32_t)s_key[j] * 6;
    double db[4];
    widen4(row, db);
    const double ad = area(db);
    const int m = walk(db, ad, (int)s_cls[j], s_gbox, s_garea, s_gcls, s_gign[a], M, matched, thr);
    dt_match[at * D + j] = m;
    dt_ignore[at * D + j] = m >= 0 ? s_gign[a][m] : (uint8_t)(outside(ad, lo, hi) ? 1 : 0);
    if (m >= 0) gt_match[at * M + m] = j;
  }
}

// e = image * D + position.  keys[e]: the score key; cls[e]: the class, K for a position beyond the live rows; count[K + 1]
// (zeroed by the caller): the class histogram
__global__ void __launch_bounds__(256) k_de_keys(const float* __restrict__ dets, const int32_t* __restrict__ dt_order, uint32_t n, int D,
                                                 int K, uint32_t* __restrict__ keys, uint32_t* __restrict__ cls,
                                                 uint32_t* __restrict__ count) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n) return;
  const int row = dt_order[e];
  uint32_t key = 0xffffffffu, c = (uint32_t)K;
  if (row >= 0 && row < D) {                                 // (a row the match did not write, or a dead one, counts as beyond the live rows)
    const float* r = dets + ((size_t)(e / (uint32_t)D) * (size_t)D + (size_t)row) * 6;
    const int k = det_class(r, K);
    if (k >= 0) { key = score_key(r[4]); c = (uint32_t)k; }
  }
  keys[e] = key;
  cls[e] = c;
  atomicAdd(&count[c], 1u);
}

__global__ void __launch_bounds__(256) k_de_classes(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ cls, uint32_t n,
                                                    uint32_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) keys[i] = cls[vals[i]];
}

// npig [K,A] (zeroed by the caller)
__global__ void __launch_bounds__(256) k_de_npig(const int32_t* __restrict__ gt_cls, const uint8_t* __restrict__ gt_ignore, uint32_t total,
                                                 int A, int M, int K, int32_t* __restrict__ npig) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;       // ((image * A) + a) * M + g
  if (i >= total || gt_ignore[i] != 0) return;
  const uint32_t g = i % (uint32_t)M, a = (i / (uint32_t)M) % (uint32_t)A, img = i / (uint32_t)(M * A);
  const int k = gt_cls[(size_t)img * M + g];
  if (k >= 0 && k < K) atomicAdd(&npig[(size_t)k * A + a], 1);
}

__device__ __forceinline__ uint64_t wave_incl_scan_u64(uint64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

struct CurveArgs {
  const float* dets;
  const int32_t *dt_order, *dt_rank, *dt_match;
  const uint8_t* dt_ignore;
  const uint32_t *vals, *off;      // the values sorted by (class, score descending, image, rank); off[k .. k + 1]: class k's segment
  const int32_t* npig;
  const double* rec_thrs;
  double *precision, *scores, *recall;
};

// the packed flags of sorted element i under (a, t, cap): tp | fp << 21 | in the list << 42, and its score
__device__ __forceinline__ uint64_t curve_flags(const CurveArgs& c, const Spec& s, uint32_t i, int a, int t, int cap, float* score) {
  const uint32_t e = c.vals[i];
  if (c.dt_rank[e] >= cap) return 0ull;
  const uint32_t img = e / (uint32_t)s.D, j = e % (uint32_t)s.D;
  const size_t o = (((size_t)img * s.A + a) * s.T + t) * (size_t)s.D + j;
  if (score) *score = c.dets[((size_t)img * s.D + (size_t)c.dt_order[e]) * 6 + 4];
  uint64_t f = 1ull << (2 * FIELD_BITS);
  if (c.dt_ignore[o] == 0) f |= c.dt_match[o] >= 0 ? 1ull : (1ull << FIELD_BITS);
  return f;
}

__global__ void __launch_bounds__(ACC_CHUNK) k_de_curve(const Spec s, const CurveArgs c) {
  extern __shared__ double s_prec[];                         // R precisions, then R scores
  double* s_score = s_prec + s.R;
  constexpr uint64_t FIELD = (1ull << FIELD_BITS) - 1ull;
  const int lane = threadIdx.x, T = s.T, Mx = s.n_caps, A = s.A, R = s.R;
  const uint32_t task = blockIdx.x;
  const int t = (int)(task % (uint32_t)T), m = (int)((task / (uint32_t)T) % (uint32_t)Mx);
  const int a = (int)((task / (uint32_t)(T * Mx)) % (uint32_t)A), k = (int)(task / (uint32_t)(T * Mx * A));
  const long long np = c.npig[(size_t)k * A + a];
  if (np == 0) {                                             // no counted ground truth: the class stays out of every mean
    for (int r = lane; r < R; r += ACC_CHUNK) {
      c.precision[prec_index(s, t, r, k, a, m)] = -1.0;
      c.scores[prec_index(s, t, r, k, a, m)] = -1.0;
    }
    if (lane == 0) c.recall[rec_index(s, t, k, a, m)] = -1.0;
    return;
  }
  const uint32_t lo = c.off[k], hi = c.off[k + 1];
  const int cap = s.caps[m];
  uint64_t tot = 0ull;
  for (uint32_t i = lo + (uint32_t)lane; i < hi; i += ACC_CHUNK) tot += curve_flags(c, s, i, a, t, cap, nullptr);
  tot = wave_sum_u64(tot);
  for (int r = lane; r < R; r += ACC_CHUNK) { s_prec[r] = 0.0; s_score[r] = 0.0; }
  if (lane == 0) c.recall[rec_index(s, t, k, a, m)] = (tot >> (2 * FIELD_BITS)) == 0ull ? 0.0 : recall_at((long long)(tot & FIELD), np);
  __syncthreads();
  double env = 0.0;                                          // the largest precision behind the step (every precision is >= 0)
  uint64_t rem = tot;                                        // the totals of the elements not yet visited
  for (uint32_t ch = hi; ch > lo;) {
    const uint32_t cl = ch - lo > (uint32_t)ACC_CHUNK ? ch - ACC_CHUNK : lo;
    const uint32_t i = cl + (uint32_t)lane;
    float score = 0.0f;
    const uint64_t f = i < ch ? curve_flags(c, s, i, a, t, cap, &score) : 0ull;
    const uint64_t incl = wave_incl_scan_u64(f, lane);
    const uint64_t base = rem - __shfl(incl, ACC_CHUNK - 1, 64);
    const uint64_t at = base + incl;
    const long long tp = (long long)(at & FIELD), fp = (long long)((at >> FIELD_BITS) & FIELD), nd = (long long)(at >> (2 * FIELD_BITS));
    const bool in_list = (f >> (2 * FIELD_BITS)) != 0ull;
    double pr = in_list ? precision_at(tp, fp) : 0.0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {                       // the running maximum from the back
      const double o = __shfl_down(pr, d, 64);
      if (lane + d < 64 && o > pr) pr = o;
    }
    if (env > pr) pr = env;
    env = __shfl(pr, 0, 64);
    const bool is_tp = (f & 1ull) != 0ull, first = in_list && nd == 1;
    if (in_list && (is_tp || first)) {
      const double rc = recall_at(tp, np), before = recall_at(tp - (is_tp ? 1 : 0), np);
      for (int r = 0; r < R; ++r) {
        const double thr = c.rec_thrs[r];
        if (rc >= thr && (first || !(before >= thr))) { s_prec[r] = pr; s_score[r] = (double)score; }
      }
    }
    rem = base;
    ch = cl;
  }
  __syncthreads();
  for (int r = lane; r < R; r += ACC_CHUNK) {
    c.precision[prec_index(s, t, r, k, a, m)] = s_prec[r];
    c.scores[prec_index(s, t, r, k, a, m)] = s_score[r];
  }
}

// lane l's double, in every lane (l is the same in all of them): two scalar reads, no trip through LDS
__device__ __forceinline__ double read_lane_f64(double v, int l) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__global__ void __launch_bounds__(N_STATS * 64) k_de_summarize(const Spec s, const double* __restrict__ precision,
                                                               const double* __restrict__ recall, double* __restrict__ stats) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const StatSel q = stat_sel(w, s);
  const double* src = q.ap ? precision : recall;
  const uint32_t n = (uint32_t)stat_entries(s, q);
  double sum = 0.0;
  uint32_t cnt = 0;
  constexpr int AHEAD = 4;                                   // 64-entry pieces loaded before the first of them is added
  for (uint32_t base = 0; base < n; base += 64 * AHEAD) {
    double v[AHEAD];
#pragma unroll
    for (int p = 0; p < AHEAD; ++p) {
      const uint32_t e = base + 64u * p + (uint32_t)lane;
      v[p] = e < n ? src[stat_element(s, q, e)] : -1.0;      // (-1 is never added)
    }
#pragma unroll
    for (int p = 0; p < AHEAD; ++p) {
      // which entries count is settled by all lanes at once; the chain that remains is one addition per entry.  An entry
      // that stays out adds +0, which changes no bit: the sum starts at +0 and x + (+0) is x for every x but -0, and no
      // sum of doubles that starts at +0 is ever -0.
      const bool in = v[p] > -1.0;
      cnt += (uint32_t)__popcll(__ballot(in));
      const double a = in ? v[p] : 0.0;
#pragma unroll
      for (int l = 0; l < 64; ++l) sum = sum + read_lane_f64(a, l);          // index order, in every lane alike
    }
  }
  if (lane == 0) stats[w] = cnt > 0 ? sum / (double)cnt : -1.0;
}

}  // namespace gsr_de
