// gsr_rcnn.hip.h -- kernels of the two-stage (R-CNN-style) detector stage (gsr_rcnn_sample, gsr_roi_align,
// gsr_roi_align_backward, gsr_rcnn_loss, gsr_rcnn_postprocess).  The arithmetic is gsr_rcnn.h's, the same source the host
// harness compiles.  No float atomics: every sum is a per-thread run, a wave butterfly or a fixed LDS tree and a slab of
// per-block partials that one block adds up in index order, so the same input gives the same bits on every run.
//
//   k_rcnn_sample     one workgroup per image, the R (+ M) candidates dealt over the lanes in consecutive runs: match and key
//                     into LDS, integer counts of the two kinds, the rank of a candidate within its kind by counting the
//                     (key, index) pairs before it (only for a kind whose quota bites), then a scan of the taken flags
//                     places the rows: ascending candidate index.
//   k_roi_align       one lane per output element, pw fastest, a workgroup within one RoI (its set-up is the same in all
//                     lanes): the samples of its bin in (iy, ix) order.
//   k_roi_align_bwd   a gather: a workgroup owns an 8 x 8 tile of one image's map and a chunk of channels, a lane one pixel,
//                     a wave every fourth channel of the chunk.  It walks the image's RoIs in ascending order, skips -- the
//                     same in all lanes -- those whose sample span misses the tile, builds the separable weights
//                     wy[ph][row], wx[pw][col] of the others in LDS (samples added in index order) with the masks of their
//                     non-zero bins, and every lane adds (wy * wx) * g over its bins in (ph, pw) order, divides by the
//                     RoI's sample count and adds that to its pixel.  One store per element.
//                     The per-element body of the forward (roi_pool_element) and the per-RoI step and store of the backward
//                     (roi_bwd_step, roi_bwd_store) are device functions that gsr_fpn.hip.h's kernels call too.
//   k_rcnn_count      one block: the rows with a label >= 0 (integers).
//   k_rcnn_rows       one wave per sampled row: softmax statistics (lanes stride the row, wave butterflies), the
//                     cross-entropy term and gradient, the box term and gradient; one partial pair per block.
//   k_rcnn_final      one block adds the slab in index order and writes loss[3].
//   k_rcnn_post       one workgroup per image: class, score and box of every proposal, then a scan of the candidate flags
//                     compacts them in proposal order for the NMS walk (gsr_detect.hip.h), whose kept indices
//   k_rcnn_gather     turns into dets rows.
#pragma once
#include <hip/hip_runtime.h>

#include "gsr_block.hip.h"
#include "gsr_rcnn.h"

namespace gsr_rcnn {

using gsr_block::block_scan;
using gsr_block::block_tree_sum;
using gsr_block::slab_sum;
using gsr_block::wave_softmax_stats;

constexpr int SAMP_THREADS = 1024;
constexpr int SAMP_PER = MAX_CAND / SAMP_THREADS;     // 4
constexpr int RA_THREADS = 256;
constexpr int RB_TILE = 8;                            // the backward's tile: 8 x 8 pixels = one wave
constexpr int RB_THREADS = 256;
constexpr int RB_WAVES = RB_THREADS / 64;
constexpr int RB_CHUNK = 32;                          // channels per workgroup
constexpr int RB_PER = RB_CHUNK / RB_WAVES;           // channels per lane
constexpr int ROW_THREADS = 256;
constexpr int ROW_WAVES = ROW_THREADS / 64;
constexpr int FIN_THREADS = 256;
constexpr int POST_THREADS = 1024;
constexpr int POST_PER = MAX_CAND / POST_THREADS;     // 4

// ---- the sampler --------------------------------------------------------------------------------------------------------
struct SampleArgs {
  Spec sp;
  const float* proposals;     // [B, R, 4]
  const int32_t* n_prop;      // [B] or NULL
  const float* gt_boxes;      // [B, M, 4]
  const int32_t* gt_cls;      // [B, M]
  int32_t* idx;               // [B, S]
  float* rois;                // [B, S, 4]
  int32_t* labels;            // [B, S]
  int32_t* gt_row;            // [B, S]
  int32_t* counts;            // [B, 2]
};

constexpr int32_t INFO_INVALID = -2;   // s_info: the matched row of a foreground candidate, -1 background, -2 not a candidate

__global__ void __launch_bounds__(SAMP_THREADS) k_rcnn_sample(SampleArgs ar) {
  __shared__ uint32_t s_key[MAX_CAND];
  __shared__ int32_t s_info[MAX_CAND];
  __shared__ float s_gt[MAX_ROWS * 4];
  __shared__ int32_t s_cls[MAX_ROWS];
  __shared__ int32_t s_scan[SAMP_THREADS];
  __shared__ int s_n[2];
  const Spec& sp = ar.sp;
  const int b = blockIdx.x, t = threadIdx.x;
  const int R = sp.R, M = sp.M, S = sp.S;
  const int N = R + (sp.append_gt ? M : 0);
  const int per = (N + SAMP_THREADS - 1) / SAMP_THREADS;                 // <= SAMP_PER
  int np = ar.n_prop ? ar.n_prop[b] : R;
  np = np < 0 ? 0 : (np > R ? R : np);

  if (t < M) {
    s_cls[t] = ar.gt_cls[(size_t)b * (size_t)M + (size_t)t];
    for (int k = 0; k < 4; ++k) s_gt[t * 4 + k] = ar.gt_boxes[((size_t)b * (size_t)M + (size_t)t) * 4 + (size_t)k];
  }
  if (t < 2) s_n[t] = 0;
  __syncthreads();

  const int i0 = t * per;
  int nfg_mine = 0, nbg_mine = 0;
  for (int k = 0; k < per; ++k) {
    const int i = i0 + k;
    if (i >= N) break;
    const bool valid = i < R ? i < np : present(s_cls[i - R], sp.C);
    int info = INFO_INVALID;
    if (valid) {
      float bx[4], best;
      for (int c = 0; c < 4; ++c) bx[c] = i < R ? ar.proposals[((size_t)b * (size_t)R + (size_t)i) * 4 + (size_t)c] : s_gt[(i - R) * 4 + c];
      info = match_candidate<float>(bx, s_gt, s_cls, M, sp.C, sp.fg_iou, best);
      if (info >= 0) ++nfg_mine; else ++nbg_mine;
    }
    s_info[i] = info;
    s_key[i] = sample_key(sp.seed, b, i);
  }
  if (nfg_mine) atomicAdd(&s_n[0], nfg_mine);                            // integers: any order gives the same number
  if (nbg_mine) atomicAdd(&s_n[1], nbg_mine);
  __syncthreads();
  const int nfg = s_n[0], nbg = s_n[1];
  const int n_pos = nfg < sp.max_pos ? nfg : sp.max_pos;
  const int n_neg = nbg < S - n_pos ? nbg : S - n_pos;

  unsigned taken = 0u;
  int mine = 0;
  for (int k = 0; k < per; ++k) {
    const int i = i0 + k;
    if (i >= N) break;
    const int info = s_info[i];
    if (info == INFO_INVALID) continue;
    const bool fg = info >= 0;
    const int quota = fg ? n_pos : n_neg, total = fg ? nfg : nbg;
    bool take = quota >= total;
    if (!take && quota > 0) {
      const uint32_t key = s_key[i];
      int rank = 0;
      for (int j = 0; j < N; ++j) {
        const int oj = s_info[j];
        if (oj != INFO_INVALID && (oj >= 0) == fg && key_before(s_key[j], j, key, i)) ++rank;
      }
      take = rank < quota;
    }
    if (take) { taken |= 1u << k; ++mine; }
  }
  const int incl = block_scan(s_scan, mine, SAMP_THREADS);
  const int total = s_scan[SAMP_THREADS - 1];                            // = n_pos + n_neg <= S
  int pos = incl - mine;
  for (int k = 0; k < per; ++k) {
    if (!(taken & (1u << k))) continue;
    const int i = i0 + k;
    if (pos < S) {
      const size_t o = (size_t)b * (size_t)S + (size_t)pos;
      const int row = s_info[i];
      ar.idx[o] = i;
      for (int c = 0; c < 4; ++c)
        ar.rois[o * 4 + (size_t)c] = i < R ? ar.proposals[((size_t)b * (size_t)R + (size_t)i) * 4 + (size_t)c] : s_gt[(i - R) * 4 + c];
      ar.labels[o] = row >= 0 ? s_cls[row] : sp.C;
      ar.gt_row[o] = row >= 0 ? row : -1;
    }
    ++pos;
  }
  for (int s = (total < S ? total : S) + t; s < S; s += SAMP_THREADS) {
    const size_t o = (size_t)b * (size_t)S + (size_t)s;
    ar.idx[o] = -1;
    for (int c = 0; c < 4; ++c) ar.rois[o * 4 + (size_t)c] = 0.0f;
    ar.labels[o] = -1;
    ar.gt_row[o] = -1;
  }
  if (t == 0) {
    ar.counts[(size_t)b * 2] = total < S ? total : S;
    ar.counts[(size_t)b * 2 + 1] = n_pos;
  }
}

// ---- RoIAlign -------------------------------------------------------------------------------------------------------------
struct RoiArgs {
  Spec sp;
  const float* features;      // forward: [B, Cf, Hf, Wf]
  const float* rois;          // [B, S, 4]
  const int32_t* n_roi;       // element b * n_roi_stride, or NULL: S
  int32_t n_roi_stride;
  float* pooled;              // forward: [B, S, Cf, PH, PW]
  const float* grad_pooled;   // backward
  float* grad_features;       // backward: [B, Cf, Hf, Wf]
  int32_t accumulate;
};

__device__ __forceinline__ int roi_count(const RoiArgs& ar, int b) {
  int n = ar.n_roi ? ar.n_roi[(size_t)b * (size_t)ar.n_roi_stride] : ar.sp.S;
  return n < 0 ? 0 : (n > ar.sp.S ? ar.sp.S : n);
}

// What RoIAlign needs to know of one feature map (the single-level entries build it from their Spec, the FPN pooler --
// gsr_fpn.hip.h -- from the level's members).
struct RoiMap {
  int Cf, Hf, Wf, PH, PW, sampling_ratio;
  float scale;
};

__device__ __forceinline__ RoiMap roi_map(const Spec& sp) {
  return RoiMap{sp.Cf, sp.Hf, sp.Wf, sp.PH, sp.PW, sp.sampling_ratio, sp.spatial_scale};
}

// One element of pooled: bin (ph, pw) of the finite RoI r on the channel plane f [Hf, Wf], the samples in (iy, ix) order.
__device__ __forceinline__ float roi_pool_element(const RoiMap& mp, const float* f, const float* r, int ph, int pw) {
  float sx, bx, sy, by;
  int gx, gy;
  roi_axis<float>(r[0], r[2], mp.scale, mp.PW, mp.sampling_ratio, sx, bx, gx);
  roi_axis<float>(r[1], r[3], mp.scale, mp.PH, mp.sampling_ratio, sy, by, gy);
  const int cnt = gx * gy > 1 ? gx * gy : 1;
  float acc = 0.0f;
  for (int iy = 0; iy < gy; ++iy) {
    int yl, yh;
    float hy, ly;
    const bool oky = lerp_axis<float>(sample_pos<float>(sy, by, gy, ph, iy), mp.Hf, yl, yh, hy, ly);
    for (int ix = 0; ix < gx; ++ix) {
      int xl, xh;
      float hx, lx;
      const bool okx = lerp_axis<float>(sample_pos<float>(sx, bx, gx, pw, ix), mp.Wf, xl, xh, hx, lx);
      float v = 0.0f;
      if (oky && okx) {
        GSR_FP_STRICT
        const float v1 = f[(size_t)yl * (size_t)mp.Wf + (size_t)xl], v2 = f[(size_t)yl * (size_t)mp.Wf + (size_t)xh];
        const float v3 = f[(size_t)yh * (size_t)mp.Wf + (size_t)xl], v4 = f[(size_t)yh * (size_t)mp.Wf + (size_t)xh];
        v = ((hy * hx) * v1 + (hy * lx) * v2) + (ly * hx) * v3 + (ly * lx) * v4;
      }
      {
        GSR_FP_STRICT
        acc = acc + v;
      }
    }
  }
  {
    GSR_FP_STRICT
    return acc / (float)cnt;
  }
}

__global__ void __launch_bounds__(RA_THREADS) k_roi_align(RoiArgs ar) {
  const Spec& sp = ar.sp;
  const unsigned bs = blockIdx.x;                                         // (image, RoI): the same in all lanes
  const unsigned bins = (unsigned)(sp.PH * sp.PW), per_roi = (unsigned)sp.Cf * bins;
  const unsigned i = blockIdx.y * RA_THREADS + threadIdx.x;               // (channel, ph, pw) of that RoI
  if (i >= per_roi) return;
  const int s = (int)(bs % (unsigned)sp.S), b = (int)(bs / (unsigned)sp.S);
  const int c = (int)(i / bins);
  const unsigned rem = i - (unsigned)c * bins;
  const int ph = (int)(rem / (unsigned)sp.PW), pw = (int)(rem - (unsigned)ph * (unsigned)sp.PW);
  const size_t e = (size_t)bs * (size_t)per_roi + (size_t)i;
  float out = 0.0f;
  float r[4];
  for (int k = 0; k < 4; ++k) r[k] = ar.rois[(size_t)bs * 4 + (size_t)k];
  if (s < roi_count(ar, b) && roi_finite<float>(r))
    out = roi_pool_element(roi_map(sp), ar.features + ((size_t)b * (size_t)sp.Cf + (size_t)c) * (size_t)sp.Hf * (size_t)sp.Wf, r, ph, pw);
  ar.pooled[e] = out;
}

// the weight of map cell `cell` in bin p of one axis: the samples' shares, added in sample order
__device__ __forceinline__ float axis_weight(float start, float bin, int grid, int p, int n, int cell) {
  GSR_FP_STRICT
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

// the sample span [start, start + P * bin] of one axis misses the cells c0 .. c0 + RB_TILE - 1 (a sample at y touches the
// cells floor(y) and floor(y) + 1, those below 0 and beyond n - 1 their border cell): conservative by a cell on each side
__device__ __forceinline__ bool span_misses(float start, float bin, int P, int c0) {
  const float end = start + (float)P * bin;
  const float lo = start < end ? start : end, hi = start < end ? end : start;
  return hi < (float)(c0 - 2) || lo > (float)(c0 + RB_TILE + 1);
}

// the backward's LDS: the separable weights of the RoI in hand, [cell of the tile][bin], and the bins with a non-zero weight
struct RoiBwdLds {
  float wy[RB_TILE][16], wx[RB_TILE][16];
  uint32_t my[RB_TILE], mx[RB_TILE];
};

// One RoI's step of the gather for the tile at (x0, y0) of the map mp and the channels c0 .. c0 + RB_CHUNK - 1: r its row of
// rois, g0 its [Cf, PH, PW] block of grad_pooled.  Every test up to the barriers is the same in all lanes, so the whole
// workgroup takes the barriers or none of it does.  acc[k] gains this RoI's share of channel c0 + wave + k * RB_WAVES.
__device__ __forceinline__ void roi_bwd_step(const RoiMap& mp, const float* r_in, const float* g0, int x0, int y0, int c0, RoiBwdLds& lds,
                                             float (&acc)[RB_PER]) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ty = lane >> 3, tx = lane & 7;
  const size_t bins = (size_t)mp.PH * (size_t)mp.PW;
  // the build's layout: threads 0..127 make wy (cell = t / 16, bin = t % 16), threads 128..255 wx
  const int b_cell = (t & 127) >> 4, b_bin = t & 15;
  const bool b_isx = t >= 128;
  float r[4];
  for (int k = 0; k < 4; ++k) r[k] = r_in[k];
  if (!roi_finite<float>(r)) return;
  float sx, bx, sy, by;
  int gx, gy;
  roi_axis<float>(r[0], r[2], mp.scale, mp.PW, mp.sampling_ratio, sx, bx, gx);
  roi_axis<float>(r[1], r[3], mp.scale, mp.PH, mp.sampling_ratio, sy, by, gy);
  if (gx < 1 || gy < 1) return;
  if (span_misses(sy, by, mp.PH, y0) || span_misses(sx, bx, mp.PW, x0)) return;
  __syncthreads();                                                        // the previous RoI's weights have been read
  {
    const int P = b_isx ? mp.PW : mp.PH;
    float w = 0.0f;
    if (b_bin < P)
      w = b_isx ? axis_weight(sx, bx, gx, b_bin, mp.Wf, x0 + b_cell) : axis_weight(sy, by, gy, b_bin, mp.Hf, y0 + b_cell);
    (b_isx ? lds.wx : lds.wy)[b_cell][b_bin] = w;
    const unsigned long long m = __ballot(w != 0.0f);                     // 4 cells of 16 bins per wave
    if (b_bin == 0) (b_isx ? lds.mx : lds.my)[b_cell] = (uint32_t)((m >> ((lane >> 4) * 16)) & 0xffffull);
  }
  __syncthreads();
  const uint32_t my = lds.my[ty], mx = lds.mx[tx];
  if (my == 0u || mx == 0u) return;                                       // (the step's barriers are above: every lane passed them)
  const float cnt = (float)(gx * gy);
  float part[RB_PER];
#pragma unroll
  for (int k = 0; k < RB_PER; ++k) part[k] = 0.0f;
  for (uint32_t my_ = my; my_; my_ &= my_ - 1u) {
    const int ph = __ffs((int)my_) - 1;
    const float wy = lds.wy[ty][ph];
    for (uint32_t mx_ = mx; mx_; mx_ &= mx_ - 1u) {
      GSR_FP_STRICT
      const int pw = __ffs((int)mx_) - 1;
      const float w = wy * lds.wx[tx][pw];
      const size_t o = (size_t)ph * (size_t)mp.PW + (size_t)pw;
#pragma unroll
      for (int k = 0; k < RB_PER; ++k) {
        const int c = c0 + wave + k * RB_WAVES;
        if (c < mp.Cf) part[k] = part[k] + w * g0[(size_t)c * bins + o];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < RB_PER; ++k) {
    GSR_FP_STRICT
    acc[k] = acc[k] + part[k] / cnt;
  }
}

// the tile's pixels of the channels c0 + wave + k * RB_WAVES of the plane stack g [Cf, Hf, Wf]: one store per element
__device__ __forceinline__ void roi_bwd_store(const RoiMap& mp, float* g, int x0, int y0, int c0, int accumulate, const float (&acc)[RB_PER]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y = y0 + (lane >> 3), x = x0 + (lane & 7);
  if (y < mp.Hf && x < mp.Wf) {
#pragma unroll
    for (int k = 0; k < RB_PER; ++k) {
      const int c = c0 + wave + k * RB_WAVES;
      if (c >= mp.Cf) continue;
      float* o = g + ((size_t)c * (size_t)mp.Hf + (size_t)y) * (size_t)mp.Wf + (size_t)x;
      *o = accumulate ? *o + acc[k] : acc[k];
    }
  }
}

__global__ void __launch_bounds__(RB_THREADS) k_roi_align_bwd(RoiArgs ar) {
  __shared__ RoiBwdLds lds;
  const Spec& sp = ar.sp;
  const RoiMap mp = roi_map(sp);
  const int tiles_x = (sp.Wf + RB_TILE - 1) / RB_TILE;
  const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * RB_TILE, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * RB_TILE;
  const int c0 = (int)blockIdx.y * RB_CHUNK, b = (int)blockIdx.z;
  const int n = roi_count(ar, b);
  const size_t per_roi = (size_t)sp.Cf * (size_t)sp.PH * (size_t)sp.PW;

  float acc[RB_PER];
#pragma unroll
  for (int k = 0; k < RB_PER; ++k) acc[k] = 0.0f;

  for (int s = 0; s < n; ++s) {                                           // n: the same in all lanes
    const size_t q = (size_t)b * (size_t)sp.S + (size_t)s;
    roi_bwd_step(mp, ar.rois + q * 4, ar.grad_pooled + q * per_roi, x0, y0, c0, lds, acc);
  }
  roi_bwd_store(mp, ar.grad_features + (size_t)b * (size_t)sp.Cf * (size_t)sp.Hf * (size_t)sp.Wf, x0, y0, c0, ar.accumulate, acc);
}

// ---- the box head's loss ----------------------------------------------------------------------------------------------------
struct LossArgs {
  Spec sp;
  const float* scores;        // [B, S, C + 1]
  const float* deltas;        // [B, S, 4 * C] or [B, S, 4]
  const float* rois;          // [B, S, 4]
  const int32_t* labels;      // [B, S]
  const int32_t* gt_row;      // [B, S]
  const float* gt_boxes;      // [B, M, 4]
  int32_t* nrows;             // workspace [1]
  float* slab;                // workspace [blocks of k_rcnn_rows, 2]
  float* loss;                // [3]
  float* grad_scores;         // or NULL
  float* grad_deltas;         // or NULL
};

__global__ void __launch_bounds__(FIN_THREADS) k_rcnn_count(LossArgs ar) {
  __shared__ int s_cnt[1][FIN_THREADS];
  const int t = threadIdx.x;
  const long long rows = (long long)ar.sp.B * (long long)ar.sp.S;
  int n = 0;
  for (long long i = t; i < rows; i += FIN_THREADS) n += (ar.labels[i] >= 0 && ar.labels[i] <= ar.sp.C) ? 1 : 0;
  s_cnt[0][t] = n;
  block_tree_sum(s_cnt);
  if (t == 0) ar.nrows[0] = s_cnt[0][0];
}

__device__ __forceinline__ float norm_rows(int n) { return n > 1 ? (float)n : 1.0f; }

__global__ void __launch_bounds__(ROW_THREADS) k_rcnn_rows(LossArgs ar) {
  __shared__ float s_part[ROW_WAVES][2];
  const Spec& sp = ar.sp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long rows = (long long)sp.B * (long long)sp.S;
  const long long gq = (long long)blockIdx.x * ROW_WAVES + wave;
  const int n1 = sp.C + 1;
  const int D = (sp.flags & CLASS_AGNOSTIC) ? 4 : 4 * sp.C;
  float ce = 0.0f, box = 0.0f;
  if (gq < rows) {                                                        // the same in all lanes of a wave
    GSR_FP_STRICT
    const int b = (int)(gq / sp.S);
    const float nr = norm_rows(ar.nrows[0]);
    const float kc = sp.w_cls / nr, kb = sp.w_box / nr;
    int label = ar.labels[gq];
    label = label > sp.C ? -1 : label;                                    // never past the logits, whatever the integers were
    int row = ar.gt_row[gq];
    const bool fg = label >= 0 && label < sp.C && row >= 0 && row < sp.M;
    const float* x = ar.scores + (size_t)gq * (size_t)n1;
    float* gs = ar.grad_scores ? ar.grad_scores + (size_t)gq * (size_t)n1 : nullptr;
    if (label >= 0) {
      float m, sm;
      wave_softmax_stats(x, n1, lane, m, sm);
      ce = -log_softmax<float>(x[label], m, sm);
      if (gs)
        for (int k = lane; k < n1; k += 64) gs[k] = kc * (softmax_prob<float>(x[k], m, sm) - (k == label ? 1.0f : 0.0f));
    } else if (gs) {
      for (int k = lane; k < n1; k += 64) gs[k] = 0.0f;
    }
    const int base = (sp.flags & CLASS_AGNOSTIC) ? 0 : 4 * (fg ? label : 0);
    float g4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (fg) {
      float src[4], dst[4], tg[4];
      const float w[4] = {sp.bw_x, sp.bw_y, sp.bw_w, sp.bw_h};
      for (int k = 0; k < 4; ++k) {
        src[k] = ar.rois[(size_t)gq * 4 + (size_t)k];
        dst[k] = ar.gt_boxes[((size_t)b * (size_t)sp.M + (size_t)row) * 4 + (size_t)k];
      }
      target_deltas<float>(src, dst, w, tg);
      const float* d = ar.deltas + (size_t)gq * (size_t)D + (size_t)base;
      for (int k = 0; k < 4; ++k) {
        float g;
        box = box + smooth_l1<float>(d[k] - tg[k], sp.beta, g);
        g4[k] = kb * g;
      }
    }
    if (ar.grad_deltas) {
      float* gd = ar.grad_deltas + (size_t)gq * (size_t)D;
      for (int k = lane; k < D; k += 64) {
        const int j = k - base;
        gd[k] = !fg ? 0.0f : j == 0 ? g4[0] : j == 1 ? g4[1] : j == 2 ? g4[2] : j == 3 ? g4[3] : 0.0f;
      }
    }
  }
  if (lane == 0) { s_part[wave][0] = ce; s_part[wave][1] = box; }
  __syncthreads();
  if (threadIdx.x < 2) {
    GSR_FP_STRICT
    float s = s_part[0][threadIdx.x];
    for (int w = 1; w < ROW_WAVES; ++w) s = s + s_part[w][threadIdx.x];
    ar.slab[(size_t)blockIdx.x * 2 + threadIdx.x] = s;
  }
}

__global__ void __launch_bounds__(FIN_THREADS) k_rcnn_final(LossArgs ar, unsigned nblocks) {
  GSR_FP_STRICT
  __shared__ float s_red[2][FIN_THREADS];
  const Spec& sp = ar.sp;
  const int t = threadIdx.x;
  slab_sum<2, FIN_THREADS>(ar.slab, nblocks, s_red);
  if (t == 0) {
    const float nr = norm_rows(ar.nrows[0]);
    const float cls = s_red[0][0] / nr, box = s_red[1][0] / nr;
    ar.loss[0] = cls;
    ar.loss[1] = box;
    ar.loss[2] = sp.w_cls * cls + sp.w_box * box;
  }
}

// ---- the output stage -------------------------------------------------------------------------------------------------------
struct PostArgs {
  Spec sp;
  const float* scores;        // [B, R, C + 1]
  const float* deltas;        // [B, R, 4 * C] or [B, R, 4]
  const float* proposals;     // [B, R, 4]
  const int32_t* n_prop;      // [B] or NULL
  float* boxes;               // workspace [B, R, 4]: the candidates, compacted in proposal order
  float* score;               // workspace [B, R], -inf beyond the candidates
  int32_t* cls;               // workspace [B, R]
  int32_t* ncand;             // workspace [B]
  const int32_t* keep;        // workspace [B, max_det], the NMS walk's
  const int32_t* nkept;       // workspace [B]
  float* dets;                // [B, max_det, 6]
  int32_t* counts;            // [B, 2]
};

__global__ void __launch_bounds__(POST_THREADS) k_rcnn_post(PostArgs ar) {
  __shared__ int32_t s_scan[POST_THREADS];
  const Spec& sp = ar.sp;
  const int b = blockIdx.x, t = threadIdx.x;
  const int R = sp.R, n1 = sp.C + 1;
  const int D = (sp.flags & CLASS_AGNOSTIC) ? 4 : 4 * sp.C;
  const int per = (R + POST_THREADS - 1) / POST_THREADS;                  // <= POST_PER
  int np = ar.n_prop ? ar.n_prop[b] : R;
  np = np < 0 ? 0 : (np > R ? R : np);
  const float w[4] = {sp.bw_x, sp.bw_y, sp.bw_w, sp.bw_h};
  float o_box[POST_PER][4], o_score[POST_PER];
  int o_cls[POST_PER];
  unsigned cand = 0u;
  int mine = 0;
#pragma unroll
  for (int k = 0; k < POST_PER; ++k) {
    const int i = t * per + k;
    o_score[k] = -INFINITY;
    o_cls[k] = 0;
    for (int c = 0; c < 4; ++c) o_box[k][c] = 0.0f;
    if (k >= per || i >= np) continue;
    const size_t q = (size_t)b * (size_t)R + (size_t)i;
    const float* x = ar.scores + q * (size_t)n1;
    float mx, sum, bp = -INFINITY;
    int bc = 0x7fffffff;
    softmax_stats<float>(x, n1, mx, sum);
    for (int c = 0; c < sp.C; ++c) {
      const float p = softmax_prob<float>(x[c], mx, sum);
      if (score_better<float>(p, c, bp, bc)) { bp = p; bc = c; }
    }
    if (!(bp > sp.conf_thr)) continue;                                    // a NaN score is dropped; bc < C from here on
    float roi[4], d[4];
    const size_t base = (sp.flags & CLASS_AGNOSTIC) ? 0 : (size_t)4 * (size_t)bc;
    for (int c = 0; c < 4; ++c) {
      roi[c] = ar.proposals[q * 4 + (size_t)c];
      d[c] = ar.deltas[q * (size_t)D + base + (size_t)c];
    }
    apply_deltas<float>(roi, d, w, sp.img_w, sp.img_h, o_box[k]);
    if (!roi_finite<float>(o_box[k])) continue;
    o_score[k] = bp;
    o_cls[k] = bc;
    cand |= 1u << k;
    ++mine;
  }
  const int incl = block_scan(s_scan, mine, POST_THREADS);
  const int total = s_scan[POST_THREADS - 1];
  int pos = incl - mine;
#pragma unroll
  for (int k = 0; k < POST_PER; ++k) {
    if (!(cand & (1u << k))) continue;
    const size_t o = (size_t)b * (size_t)R + (size_t)pos;
    for (int c = 0; c < 4; ++c) ar.boxes[o * 4 + (size_t)c] = o_box[k][c];
    ar.score[o] = o_score[k];
    ar.cls[o] = o_cls[k];
    ++pos;
  }
  for (int s = total + t; s < R; s += POST_THREADS) {
    const size_t o = (size_t)b * (size_t)R + (size_t)s;
    for (int c = 0; c < 4; ++c) ar.boxes[o * 4 + (size_t)c] = 0.0f;
    ar.score[o] = -INFINITY;
    ar.cls[o] = -1;
  }
  if (t == 0) {
    ar.ncand[b] = total;
    ar.counts[(size_t)b * 2 + 1] = total;
  }
}

__global__ void __launch_bounds__(256) k_rcnn_gather(PostArgs ar) {
  const Spec& sp = ar.sp;
  const int b = blockIdx.x, t = threadIdx.x;
  int kept = ar.nkept[b];
  kept = kept < 0 ? 0 : (kept > sp.max_det ? sp.max_det : kept);
  for (int j = t; j < sp.max_det; j += 256) {
    float* row = ar.dets + ((size_t)b * (size_t)sp.max_det + (size_t)j) * 6;
    int i = j < kept ? ar.keep[(size_t)b * (size_t)sp.max_det + (size_t)j] : -1;
    i = i < sp.R ? i : -1;
    if (i >= 0) {
      const size_t o = (size_t)b * (size_t)sp.R + (size_t)i;
      for (int c = 0; c < 4; ++c) row[c] = ar.boxes[o * 4 + (size_t)c];
      row[4] = ar.score[o];
      row[5] = (float)ar.cls[o];
    } else {
      for (int c = 0; c < 6; ++c) row[c] = 0.0f;
    }
  }
  if (t == 0) ar.counts[(size_t)b * 2] = kept;
}

}  // namespace gsr_rcnn
