// gsr_detect.hip.h -- kernels of the detector's output stage (gsr_det_postprocess, gsr_det_nms, gsr_det_box_iou,
// gsr_det_verdict).  The arithmetic is gsr_detect.h's, the same source the host harness compiles: results are bit for
// bit the host's, and every output is the same on every run (integer atomics only, and nothing depends on the order
// in which they land).
//
//   k_det_score<LAYOUT>  streams pred once -> per-anchor (score, class) in the workspace.  Layout 1 ([B,K,A], contiguous
//                        in A): one lane per anchor loops over the channels.  Layout 0 ([B,A,K], contiguous in K): 16
//                        lanes per anchor stride over its row and combine with 4 shuffles; the preference is a total
//                        order, so the combination tree gives the sequential answer.
//   k_det_select_sort    one workgroup per image: counts the candidates; beyond max_candidates gsr_block's select over the
//                        64-bit composite finds the cut; its gather and sort put the candidates at or below the cut into
//                        LDS, best first (32 KiB).
//   k_det_nms            one workgroup per image, greedy sweep: every thread holds 8 entries (box, area, class) in
//                        registers, a 4096-bit alive mask sits in LDS; per kept box: all threads find the next alive
//                        entry from the mask, its owner publishes the box, every thread tests its later entries and
//                        clears their bits.  Two barriers per KEPT box, none per suppressed one.
//   k_det_box_iou        one thread per (i, j).
//   k_det_verdict        one wave per image.
#pragma once
#include <hip/hip_runtime.h>

#include "gsr_block.hip.h"
#include "gsr_detect.h"

namespace gsr_detect {

constexpr int SCORE_THREADS = 256;
constexpr int SEL_THREADS = 1024;
constexpr int NMS_THREADS = 512;
constexpr int NMS_PER_THREAD = MAX_CAND / NMS_THREADS;   // 8
constexpr int NMS_WORDS = MAX_CAND / 32;                 // 128

// ---- score pass ------------------------------------------------------------------------------------------------------
template <int LAYOUT>
__global__ void __launch_bounds__(SCORE_THREADS) k_det_score(Spec sp, const float* __restrict__ pred,
                                                             float* __restrict__ score, int32_t* __restrict__ cls) {
  const int K = channels(sp);
  const long long total = (long long)sp.B * (long long)sp.A;
  if (LAYOUT == 1) {
    const long long g = (long long)blockIdx.x * SCORE_THREADS + threadIdx.x;
    if (g >= total) return;
    const int b = (int)(g / sp.A), a = (int)(g % sp.A);
    const float* p = pred + (size_t)b * (size_t)K * (size_t)sp.A + (size_t)a;
    const float obj = sp.has_obj ? p[(size_t)4 * (size_t)sp.A] : 1.0f;
    float s;
    int c;
    anchor_best(p + (size_t)(4 + sp.has_obj) * (size_t)sp.A, (size_t)sp.A, sp.C, obj, sp.has_obj, s, c);
    score[g] = s;
    cls[g] = c;
  } else {
    const int sub = threadIdx.x & 15;
    const long long g = ((long long)blockIdx.x * SCORE_THREADS + threadIdx.x) >> 4;   // one anchor per 16 lanes
    const bool live = g < total;
    float bs = neg_inf();
    int bc = 0;
    if (live) {
      const float* p = pred + (size_t)g * (size_t)K;
      const float obj = sp.has_obj ? p[4] : 1.0f;
      const float* q = p + 4 + sp.has_obj;
      for (int c = sub; c < sp.C; c += 16) {
        const float s = class_score(obj, q[c], sp.has_obj);
        if (better(s, c, bs, bc)) { bs = s; bc = c; }
      }
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {               // every lane of the wave takes part; groups of 16 stay apart
      const float os = __shfl_xor(bs, m);
      const int oc = __shfl_xor(bc, m);
      if (better(os, oc, bs, bc)) { bs = os; bc = oc; }
    }
    if (live && sub == 0) {
      score[g] = bs;
      cls[g] = bc;
    }
  }
}

// ---- select + sort ---------------------------------------------------------------------------------------------------
// score: [B, A] (the workspace's, or the caller's for gsr_det_nms).  use_thr: a candidate is score > conf_thr; otherwise
// every entry below n_valid[b] (NULL: A) is one.  order[b, 0 .. ncand[b]): the candidates' anchors, best first.
// above[b * above_stride]: the number of candidates before the cap (may be NULL).
__global__ void __launch_bounds__(SEL_THREADS) k_det_select_sort(int A, int maxc, const float* __restrict__ score,
                                                                 int use_thr, float conf_thr,
                                                                 const int32_t* __restrict__ n_valid,
                                                                 int32_t* __restrict__ order, int32_t* __restrict__ ncand,
                                                                 int32_t* __restrict__ above, int above_stride) {
  __shared__ uint64_t keys[MAX_CAND];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_count;
  const int b = blockIdx.x, t = threadIdx.x;
  const float* sc = score + (size_t)b * (size_t)A;
  int n_in = A;
  if (n_valid) {
    n_in = n_valid[b];
    n_in = n_in < 0 ? 0 : n_in > A ? A : n_in;
  }
  if (t == 0) s_count = 0u;
  __syncthreads();
  uint32_t mine = 0;
  for (int a = t; a < n_in; a += SEL_THREADS) mine += (!use_thr || is_candidate(sc[a], conf_thr)) ? 1u : 0u;
  if (mine) atomicAdd(&s_count, mine);
  __syncthreads();
  const uint32_t total = s_count;
  __syncthreads();
  const int n = total < (uint32_t)maxc ? (int)total : maxc;
  if (t == 0) {
    if (above) above[(size_t)b * (size_t)above_stride] = (int32_t)total;
    ncand[b] = n;
  }
  const auto key_at = [&](int a, uint64_t& key) {
    const float s = sc[a];
    key = composite(s, a);
    return !use_thr || is_candidate(s, conf_thr);
  };
  uint64_t cut = ~0ull;                              // every candidate lies at or below it
  int taken = n;
  if (total > (uint32_t)maxc) cut = gsr_block::block_select_u64<SEL_THREADS>(hist, n_in, maxc, key_at, taken, (int)total);
  gsr_block::block_gather_sort_u64<SEL_THREADS>(keys, &s_count, n_in, taken, cut, key_at);
  for (int i = t; i < n; i += SEL_THREADS) order[(size_t)b * (size_t)maxc + (size_t)i] = (int32_t)(uint32_t)keys[i];
}

// ---- NMS ---------------------------------------------------------------------------------------------------------------
// What the walk reads and writes: FROM_PRED decodes the boxes of `pred` and writes dets rows (gsr_det_postprocess);
// otherwise boxes [B,n,4] are read as given and the kept indices are written (gsr_det_nms).
struct NmsArgs {
  Spec sp;                     // FROM_PRED: the whole spec; otherwise A = n, iou_thr, max_det, max_candidates = n, flags
  const float* pred;           // FROM_PRED
  const float* score;          // [B, A]
  const int32_t* cls;          // [B, A], or NULL (every class 0: agnostic)
  const float* boxes;          // !FROM_PRED: [B, n, 4]
  const int32_t* order;        // [B, max_candidates]
  const int32_t* ncand;        // [B]
  float* dets;                 // FROM_PRED: [B, max_det, 6]
  int32_t* keep;               // !FROM_PRED: [B, max_det]
  int32_t* counts;             // FROM_PRED: [B, 2], kept into [b, 0]; otherwise [B]
};

template <bool FROM_PRED>
__global__ void __launch_bounds__(NMS_THREADS) k_det_nms(NmsArgs na) {
  __shared__ uint32_t alive[NMS_WORDS];
  __shared__ float s_box[5];
  __shared__ int s_cls;
  const Spec& sp = na.sp;
  const int b = blockIdx.x, t = threadIdx.x;
  int n = na.ncand[b];
  n = n < 0 ? 0 : n > sp.max_candidates ? sp.max_candidates : n;
  const bool agnostic = (sp.flags & CLASS_AGNOSTIC) != 0u || !na.cls;
  const int32_t* ord = na.order + (size_t)b * (size_t)sp.max_candidates;

  Box bx[NMS_PER_THREAD];
  float ar[NMS_PER_THREAD];
  int cl[NMS_PER_THREAD], an[NMS_PER_THREAD];
#pragma unroll
  for (int k = 0; k < NMS_PER_THREAD; ++k) {
    const int j = t + k * NMS_THREADS;
    bx[k].x1 = bx[k].y1 = bx[k].x2 = bx[k].y2 = 0.0f;
    ar[k] = 0.0f;
    cl[k] = 0;
    an[k] = 0;
    if (j < n) {
      const int a = ord[j];
      an[k] = a;
      if (FROM_PRED) {
        bx[k] = load_box(sp, na.pred, b, a);
      } else {
        const float* q = na.boxes + ((size_t)b * (size_t)sp.A + (size_t)a) * 4;
        bx[k] = decode_box(q[0], q[1], q[2], q[3], 1);
      }
      ar[k] = box_area(bx[k]);
      cl[k] = na.cls ? na.cls[(size_t)b * (size_t)sp.A + (size_t)a] : 0;
    }
  }
  for (int w = t; w < NMS_WORDS; w += NMS_THREADS) {
    const int lo = w * 32;
    alive[w] = n >= lo + 32 ? 0xffffffffu : n > lo ? ((1u << (n - lo)) - 1u) : 0u;
  }
  __syncthreads();

  int kept = 0, start = 0;
  while (kept < sp.max_det) {
    // the next alive entry at or after `start`: the same for every thread (the mask is not written in this phase)
    int nxt = -1;
    for (int w = start >> 5; w < NMS_WORDS && w * 32 < n; ++w) {
      uint32_t m = alive[w];
      if (w == (start >> 5)) m &= ~0u << (start & 31);
      if (m) { nxt = w * 32 + (__ffs((int)m) - 1); break; }
    }
    if (nxt < 0) break;
    if ((nxt & (NMS_THREADS - 1)) == t) {            // its owner publishes it and writes the output row
      const int kk = nxt / NMS_THREADS;
      Box o = bx[0];
      float oa = ar[0];
      int oc = cl[0], oan = an[0];
#pragma unroll
      for (int k = 1; k < NMS_PER_THREAD; ++k)
        if (k == kk) { o = bx[k]; oa = ar[k]; oc = cl[k]; oan = an[k]; }
      s_box[0] = o.x1; s_box[1] = o.y1; s_box[2] = o.x2; s_box[3] = o.y2; s_box[4] = oa;
      s_cls = oc;
      if (FROM_PRED) {
        const Box r = to_render_frame(o, sp.ox, sp.oy, sp.sx, sp.sy);
        float* d = na.dets + ((size_t)b * (size_t)sp.max_det + (size_t)kept) * 6;
        d[0] = r.x1; d[1] = r.y1; d[2] = r.x2; d[3] = r.y2;
        d[4] = na.score[(size_t)b * (size_t)sp.A + (size_t)oan];
        d[5] = (float)oc;
      } else {
        na.keep[(size_t)b * (size_t)sp.max_det + (size_t)kept] = oan;
      }
    }
    __syncthreads();
    Box kb;
    kb.x1 = s_box[0]; kb.y1 = s_box[1]; kb.x2 = s_box[2]; kb.y2 = s_box[3];
    const float ka = s_box[4];
    const int kc = s_cls;
#pragma unroll
    for (int k = 0; k < NMS_PER_THREAD; ++k) {
      const int j = t + k * NMS_THREADS;
      if (j > nxt && j < n && suppresses(kb, ka, kc, bx[k], ar[k], cl[k], sp.iou_thr, agnostic))
        atomicAnd(&alive[j >> 5], ~(1u << (j & 31)));
    }
    ++kept;
    start = nxt + 1;
    __syncthreads();
  }
  if (t == 0) na.counts[FROM_PRED ? (size_t)b * 2 : (size_t)b] = kept;
  if (FROM_PRED) {
    float* d = na.dets + (size_t)b * (size_t)sp.max_det * 6;
    for (int i = kept * 6 + t; i < sp.max_det * 6; i += NMS_THREADS) d[i] = 0.0f;
  } else {
    for (int i = kept + t; i < sp.max_det; i += NMS_THREADS) na.keep[(size_t)b * (size_t)sp.max_det + (size_t)i] = -1;
  }
}

// ---- box IoU -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_det_box_iou(const float* __restrict__ a, int n, const float* __restrict__ bb, int m,
                                                     float* __restrict__ out) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)n * (long long)m) return;
  const int i = (int)(g / m), j = (int)(g % m);
  const Box p = decode_box(a[(size_t)i * 4], a[(size_t)i * 4 + 1], a[(size_t)i * 4 + 2], a[(size_t)i * 4 + 3], 1);
  const Box q = decode_box(bb[(size_t)j * 4], bb[(size_t)j * 4 + 1], bb[(size_t)j * 4 + 2], bb[(size_t)j * 4 + 3], 1);
  out[g] = iou(p, box_area(p), q, box_area(q));
}

// ---- verdict -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_det_verdict(const float* __restrict__ dets, const int32_t* __restrict__ counts,
                                                    int max_det, const float* __restrict__ gt, int target, int untarget,
                                                    int is_targeted, float iou_match, int32_t* __restrict__ verdict,
                                                    float* __restrict__ best) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int n = counts[(size_t)b * 2];
  n = n < 0 ? 0 : n > max_det ? max_det : n;
  const float* rows = dets + (size_t)b * (size_t)max_det * 6;
  const float* g = gt ? gt + (size_t)b * 4 : nullptr;
  const bool has_gt = gt_present(g);
  Box gb;
  gb.x1 = gb.y1 = gb.x2 = gb.y2 = 0.0f;
  float ga = 0.0f;
  if (has_gt) {
    gb.x1 = g[0]; gb.y1 = g[1]; gb.x2 = g[2]; gb.y2 = g[3];
    ga = box_area(gb);
  }
  constexpr int NONE = 0x7fffffff;
  float bi = 0.0f;
  int bidx = NONE;                                   // no row yet: the first one is taken whatever its IoU
  bool any_t = false, any_u = false;
  for (int i = lane; i < n; i += 64) {
    const float* r = rows + (size_t)i * 6;
    const int c = (int)r[5];
    any_t = any_t || c == target;
    any_u = any_u || c == untarget;
    if (has_gt) {
      const float v = verdict_iou(r, gb, ga);
      if (bidx == NONE || v > bi) { bi = v; bidx = i; }   // ascending i inside a lane: the first maximum stays
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float oi = __shfl_xor(bi, m);
    const int ox = __shfl_xor(bidx, m);
    if (ox != NONE && (bidx == NONE || oi > bi || (oi == bi && ox < bidx))) { bi = oi; bidx = ox; }
  }
  const bool at = __any(any_t ? 1 : 0) != 0, au = __any(any_u ? 1 : 0) != 0;
  if (lane == 0) {
    const bool has_best = has_gt && n > 0;
    const int bc = has_best ? (int)rows[(size_t)bidx * 6 + 5] : -1;
    verdict[b] = verdict_bits(has_best, bi, bc, at, au, n, target, untarget, is_targeted, iou_match);
    float* o = best + (size_t)b * 4;
    if (has_best) {
      o[0] = bi; o[1] = rows[(size_t)bidx * 6 + 4]; o[2] = (float)bc; o[3] = (float)bidx;
    } else {
      o[0] = o[1] = o[2] = o[3] = -1.0f;
    }
  }
}

}  // namespace gsr_detect
