// gsr_rpn.hip.h -- kernels of the RPN proposal stage (gsr_rpn_select, gsr_rpn_nms).  The arithmetic is gsr_rpn.h's, the
// same source the host harness compiles.  No float atomics and no float sums at all: the stage orders, decodes and
// compares.  The integer LDS atomics below count (any order gives the same number) or hand out places in a list that is
// sorted by unique keys afterwards, so the same input gives the same bits on every run.
//
//   k_rpn_select   one workgroup per image.  The level's slots smallest of the image's A * Hf * Wf (logit, index) keys, read
//                  in memory order (coalesced), by gsr_block's select, gather and sort (the early end is every case without
//                  a tie across the k-th place); rank r is decoded into slot cand_offset + r.
//   k_rpn_order    one workgroup per image: the keys (score, slot) of the N slots with a level >= 0, sorted in LDS
//                  (block_sort_u64), as a list of slots in walk order and its length.
//   k_rpn_walk     one workgroup per image, the kept boxes, areas and levels in LDS.  The ordered slots are taken 64 at a
//                  time, lane l of every wave holding candidate l: wave w tests it against the kept boxes w, w + 16, ...
//                  (an LDS broadcast each) and the waves' ballots are OR-ed; the 64 x 64 block inside the chunk is one
//                  ballot per earlier candidate -- the mask of the later ones it would suppress --, resolved in order by
//                  every thread alike on uniform LDS reads; survivors are appended; the walk ends at post_topk.
#pragma once
#include <hip/hip_runtime.h>

#include "gsr_block.hip.h"
#include "gsr_rpn.h"

namespace gsr_rpn {

constexpr int RPN_THREADS = 1024;
constexpr int RPN_WAVES = RPN_THREADS / 64;
constexpr int CHUNK = 64;
constexpr int COLS_PER_WAVE = CHUNK / RPN_WAVES;     // 4

struct SelectArgs {
  Spec sp;
  const float* logits;        // [B, A, Hf, Wf]
  const float* deltas;        // [B, 4A, Hf, Wf]
  const float* cell_anchors;  // [A, 4]
  float* cand_boxes;          // [B, N, 4]
  float* cand_scores;         // [B, N]
  int32_t* cand_level;        // [B, N]
};

struct NmsArgs {
  Spec sp;
  const float* cand_boxes;    // [B, N, 4]
  const float* cand_scores;   // [B, N]
  const int32_t* cand_level;  // [B, N]
  int32_t* order;             // workspace [B, N]: slots in walk order
  int32_t* nvalid;            // workspace [B]
  float* proposals;           // [B, post_topk, 4]
  float* scores;              // [B, post_topk]
  int32_t* keep;              // [B, post_topk]
  int32_t* counts;            // [B]
};

// the key of element m (memory order: anchor a = m / HW slowest) of an image's logits; false for a NaN
__device__ __forceinline__ bool key_of(const float* lg, int m, int HW, int A, uint64_t& key) {
  const float v = lg[m];
  const int a = m / HW, p = m - a * HW;
  key = order_key(v, p * A + a);
  return !is_nan(v);
}

__global__ void __launch_bounds__(RPN_THREADS) k_rpn_select(SelectArgs ar) {
  __shared__ uint64_t s_key[MAX_SLOTS];
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_cnt;
  const Spec& sp = ar.sp;
  const int b = blockIdx.x, t = threadIdx.x;
  const int A = sp.A, HW = sp.Hf * sp.Wf, n_in = A * HW;
  const int slots = (int)level_slots(sp);                                  // <= N <= MAX_SLOTS
  const float* lg = ar.logits + (size_t)b * (size_t)n_in;

  // ---- the slots smallest keys (fewer where fewer exist), sorted
  const auto key_at = [&](int m, uint64_t& key) { return key_of(lg, m, HW, A, key); };
  int taken;
  const uint64_t thr = gsr_block::block_select_u64<RPN_THREADS>(s_hist, n_in, slots, key_at, taken);
  const int K = gsr_block::block_gather_sort_u64<RPN_THREADS>(s_key, &s_cnt, n_in, taken, thr, key_at);

  // ---- rank r -> slot cand_offset + r
  for (int r = t; r < slots; r += RPN_THREADS) {
    const size_t o = (size_t)b * (size_t)sp.N + (size_t)sp.cand_offset + (size_t)r;
    float box[4] = {0.0f, 0.0f, 0.0f, 0.0f}, score = 0.0f;
    int level = -1;
    if (r < K) {
      const int i = (int)(uint32_t)s_key[r];
      int a, x, y;
      split_index(i, A, sp.Wf, a, x, y);
      const int p = y * sp.Wf + x;
      float cell[4], anc[4], d[4], out[4];
      for (int k = 0; k < 4; ++k) {
        cell[k] = ar.cell_anchors[a * 4 + k];
        d[k] = ar.deltas[((size_t)b * (size_t)(4 * A) + (size_t)(4 * a + k)) * (size_t)HW + (size_t)p];
      }
      anchor_at<float>(cell, x, y, sp.stride, sp.shift0, anc);
      if (decode_candidate<float>(anc, d, sp.img_w, sp.img_h, sp.min_size, out)) {
        for (int k = 0; k < 4; ++k) box[k] = out[k];
        score = lg[a * HW + p];
        level = sp.level;
      }
    }
    for (int k = 0; k < 4; ++k) ar.cand_boxes[o * 4 + (size_t)k] = box[k];
    ar.cand_scores[o] = score;
    ar.cand_level[o] = level;
  }
}

__global__ void __launch_bounds__(RPN_THREADS) k_rpn_order(NmsArgs ar) {
  __shared__ uint64_t s_key[MAX_SLOTS];
  __shared__ int s_cnt;
  const Spec& sp = ar.sp;
  const int b = blockIdx.x, t = threadIdx.x, N = sp.N;
  if (t == 0) s_cnt = 0;
  __syncthreads();
  const int P = gsr_block::pow2_at_least(N > 1 ? N : 2);
  int mine = 0;
  for (int i = t; i < P; i += RPN_THREADS) {
    uint64_t key = NO_KEY;
    if (i < N) {
      const size_t o = (size_t)b * (size_t)N + (size_t)i;
      const float s = ar.cand_scores[o];
      if (ar.cand_level[o] >= 0 && !is_nan(s)) { key = order_key(s, i); ++mine; }
    }
    s_key[i] = key;
  }
  if (mine) atomicAdd(&s_cnt, mine);                                        // integers: any order gives the same number
  gsr_block::block_sort_u64<RPN_THREADS>(s_key, P);
  const int n = s_cnt;
  for (int i = t; i < N; i += RPN_THREADS) ar.order[(size_t)b * (size_t)N + (size_t)i] = i < n ? (int)(uint32_t)s_key[i] : -1;
  if (t == 0) ar.nvalid[b] = n;
}

__global__ void __launch_bounds__(RPN_THREADS) k_rpn_walk(NmsArgs ar) {
  __shared__ Box s_kbox[MAX_POST];
  __shared__ float s_karea[MAX_POST];
  __shared__ int32_t s_klvl[MAX_POST];
  __shared__ Box s_cbox[CHUNK];
  __shared__ float s_carea[CHUNK];
  __shared__ int32_t s_clvl[CHUNK], s_cslot[CHUNK];
  __shared__ uint64_t s_wmask[RPN_WAVES], s_col[CHUNK];
  const Spec& sp = ar.sp;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int N = sp.N, post = sp.post_topk;
  int n = ar.nvalid[b];
  n = n < 0 ? 0 : (n > N ? N : n);
  const int32_t* order = ar.order + (size_t)b * (size_t)N;
  int count = 0;                                                            // the same in all threads, like everything that steers the loop

  for (int base = 0; base < n && count < post; base += CHUNK) {
    if (t < CHUNK) {
      int slot = base + t < n ? order[base + t] : -1;
      slot = slot < N ? slot : -1;
      Box bx{0.0f, 0.0f, 0.0f, 0.0f};
      int lvl = -1;
      if (slot >= 0) {
        const size_t o = (size_t)b * (size_t)N + (size_t)slot;
        bx.x1 = ar.cand_boxes[o * 4]; bx.y1 = ar.cand_boxes[o * 4 + 1]; bx.x2 = ar.cand_boxes[o * 4 + 2]; bx.y2 = ar.cand_boxes[o * 4 + 3];
        lvl = ar.cand_level[o];
      }
      s_cbox[t] = bx;
      s_carea[t] = box_area(bx);
      s_clvl[t] = lvl;
      s_cslot[t] = slot;
    }
    __syncthreads();
    const Box mine = s_cbox[lane];
    const float area = s_carea[lane];
    const int lvl = s_clvl[lane];
    // against the kept boxes so far: wave w takes w, w + 16, ...
    bool sup = false;
    if (lvl >= 0)
      for (int j = wave; j < count; j += RPN_WAVES) sup = sup || suppresses(s_kbox[j], s_karea[j], s_klvl[j], mine, area, lvl, sp.iou_thr);
    const uint64_t wm = __ballot(sup);
    if (lane == 0) s_wmask[wave] = wm;
    // inside the chunk: the later candidates that candidate j would suppress
#pragma unroll
    for (int q = 0; q < COLS_PER_WAVE; ++q) {
      const int j = wave * COLS_PER_WAVE + q;
      const int jl = s_clvl[j];
      const bool s = lane > j && lvl >= 0 && jl >= 0 && suppresses(s_cbox[j], s_carea[j], jl, mine, area, lvl, sp.iou_thr);
      const uint64_t col = __ballot(s);
      if (lane == 0) s_col[j] = col;
    }
    const uint64_t valid = __ballot(lvl >= 0);                              // the same in every wave
    __syncthreads();
    uint64_t dead = 0ull;
    for (int w = 0; w < RPN_WAVES; ++w) dead |= s_wmask[w];
    uint64_t alive = valid & ~dead, kept = 0ull;
    int c = count;
    while (alive != 0ull && c < post) {
      const int j = __ffsll((unsigned long long)alive) - 1;
      kept |= 1ull << j;
      ++c;
      alive &= ~(1ull << j);
      alive &= ~s_col[j];
    }
    if (wave == 0 && ((kept >> lane) & 1ull)) {
      const int pos = count + __popcll(kept & ((1ull << lane) - 1ull));    // < post <= MAX_POST
      s_kbox[pos] = mine;
      s_karea[pos] = area;
      s_klvl[pos] = lvl;
      const int slot = s_cslot[lane];
      const size_t o = (size_t)b * (size_t)post + (size_t)pos;
      ar.proposals[o * 4] = mine.x1; ar.proposals[o * 4 + 1] = mine.y1; ar.proposals[o * 4 + 2] = mine.x2; ar.proposals[o * 4 + 3] = mine.y2;
      ar.scores[o] = ar.cand_scores[(size_t)b * (size_t)N + (size_t)slot];
      ar.keep[o] = slot;
    }
    count = c;
    __syncthreads();
  }
  for (int j = count + t; j < post; j += RPN_THREADS) {
    const size_t o = (size_t)b * (size_t)post + (size_t)j;
    for (int k = 0; k < 4; ++k) ar.proposals[o * 4 + (size_t)k] = 0.0f;
    ar.scores[o] = 0.0f;
    ar.keep[o] = -1;
  }
  if (t == 0) ar.counts[b] = count;
}

}  // namespace gsr_rpn
