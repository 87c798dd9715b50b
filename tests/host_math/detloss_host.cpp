// The detector loss stage in plain loops over csrc/gsr_detloss.h, the same scalar source the HIP kernels compile:
//   dlh_run_f32  float32, what gsr_detloss computes; every sum is taken in the kernels' own order (gsr_detloss.hip.h: a
//                strided run per thread, the fixed LDS tree, the slab of per-block partials added by one block), with
//                four anchors per lane where A % 4 == 0, so that what is left between this build and the kernels is the
//                two maths libraries
//   dlh_run_f64  the same code in double: tests/test_detloss_host_cpu.py differentiates its `total` by central differences
//                to check the hand-written backward against its own forward
// Build: g++ -O1 -ffp-contract=off -shared -fPIC -I <csrc> detloss_host.cpp -o libdetlosshost.so
#include <algorithm>
#include <cstdint>
#include <vector>

#include "gsr_detloss.h"

using namespace gsr_dloss;

struct HostSpec {   // GsrDetLossSpec of include/gsraster.h
  int32_t B, A, C, M, nl;
  int32_t level_h[5], level_w[5];
  float level_stride[5];
  int32_t reg_max, topk;
  float alpha, beta, w_box, w_cls, w_dfl;
  uint32_t flags;
};

// gsr_block.hip.h's block_tree_sum over v[0 .. n-1], n a power of two: stride halving, t < s; the sum ends in v[0]
template <class T>
static T tree_sum(std::vector<T>& v) {
  for (size_t s = v.size() / 2; s > 0; s >>= 1)
    for (size_t t = 0; t < s; ++t) v[t] = v[t] + v[t + s];
  return v[0];
}

// n values as a workgroup of `threads` adds them: thread t runs over t, t + threads, ... in index order, then the tree
template <class T>
static T strided_tree_sum(const T* x, size_t n, size_t threads) {
  std::vector<T> acc(threads, (T)0);
  for (size_t t = 0; t < threads; ++t)
    for (size_t i = t; i < n; i += threads) acc[t] = acc[t] + x[i];
  return tree_sum(acc);
}

constexpr int ASG_THREADS = 1024, TERM_THREADS = 256, CLS_CHUNK = 16, FIN_THREADS = 256;   // gsr_detloss.hip.h's

static bool to_spec(const HostSpec* d, Spec& sp) {
  if (!d || d->B < 1 || d->A < 1 || d->C < 1 || d->M < 1 || d->M > MAX_ROWS || d->nl < 1 || d->nl > MAX_LEVELS ||
      d->reg_max != REG_MAX || d->topk < 1 || d->topk > MAX_TOPK)
    return false;
  long long total = 0;
  for (int i = 0; i < MAX_LEVELS; ++i) {
    sp.h[i] = 1; sp.w[i] = 1; sp.stride[i] = 1.0f; sp.start[i] = 0x7fffffff;
  }
  for (int i = 0; i < d->nl; ++i) {
    sp.h[i] = d->level_h[i]; sp.w[i] = d->level_w[i]; sp.stride[i] = d->level_stride[i]; sp.start[i] = (int32_t)total;
    total += (long long)d->level_h[i] * d->level_w[i];
  }
  if (total != d->A) return false;
  sp.B = d->B; sp.A = d->A; sp.C = d->C; sp.M = d->M; sp.nl = d->nl; sp.topk = d->topk;
  sp.alpha = d->alpha; sp.beta = d->beta; sp.w_box = d->w_box; sp.w_cls = d->w_cls; sp.w_dfl = d->w_dfl;
  return true;
}

// pred [B,64+C,A], gt_boxes [B,M,4], gt_cls [B,M] -> loss[4], grad [B,64+C,A] or NULL, tgt [B,A], ts [B,A].
// ciou_a [B,A] (may be NULL): the `a` of every foreground anchor's CIoU.
// frozen: tgt, ts and ciou_a are INPUTS and the assignment is not run -- the contract differentiates nothing in the
// assignment and holds `a` constant, so this is the function of pred whose derivative grad is.
template <class T>
static int run(const HostSpec* d, const T* pred, const T* gt_boxes, const int32_t* gt_cls, T* loss, T* grad, int32_t* tgt, T* ts,
               T* ciou_a, int frozen) {
  Spec sp;
  if (!to_spec(d, sp)) return 1;
  const int B = sp.B, A = sp.A, C = sp.C, M = sp.M, K = channels(sp);
  const size_t sA = (size_t)A;
  std::vector<T> ov((size_t)M * sA), met((size_t)M * sA);
  std::vector<char> cand((size_t)M * sA);
  for (int b = 0; b < B && !frozen; ++b) {
    const T* pb = pred + (size_t)b * (size_t)K * sA;
    const T* gtb = gt_boxes + (size_t)b * (size_t)M * 4;
    const int32_t* gtc = gt_cls + (size_t)b * (size_t)M;
    int32_t* tg = tgt + (size_t)b * sA;
    T* tsb = ts + (size_t)b * sA;
    for (int a = 0; a < A; ++a) {
      float gx, gy, st;
      anchor_point(sp, a, gx, gy, st);
      const T px = (T)gx * (T)st, py = (T)gy * (T)st;
      bool any = false;
      for (int m = 0; m < M; ++m) {
        cand[(size_t)m * sA + a] = present(gtc[m], C) && is_candidate<T>(px, py, gtb + (size_t)m * 4);
        any = any || cand[(size_t)m * sA + a];
      }
      Box<T> pp = {(T)0, (T)0, (T)0, (T)0};
      if (any) {
        const Box<T> q = decode_grid<T>(pb + a, sA, (T)gx, (T)gy);
        pp.x1 = q.x1 * (T)st; pp.y1 = q.y1 * (T)st; pp.x2 = q.x2 * (T)st; pp.y2 = q.y2 * (T)st;
      }
      for (int m = 0; m < M; ++m) {
        T o = (T)0, me = (T)0;
        if (cand[(size_t)m * sA + a])
          candidate_metric<T>(gtb + (size_t)m * 4, pp, pb[(size_t)(BOX_CH + gtc[m]) * sA + a], (T)sp.alpha, (T)sp.beta, o, me);
        ov[(size_t)m * sA + a] = o;
        met[(size_t)m * sA + a] = me;
      }
      tg[a] = -1;
      tsb[a] = (T)0;
    }
    // top-k per row, then conflicts
    std::vector<int> npos((size_t)A, 0), row((size_t)A, -1);
    for (int m = 0; m < M; ++m) {
      if (!present(gtc[m], C)) continue;
      std::vector<uint64_t> keys;
      for (int a = 0; a < A; ++a)
        if (cand[(size_t)m * sA + a]) keys.push_back(order_composite<T>(met[(size_t)m * sA + a], a));
      std::sort(keys.begin(), keys.end());
      const size_t take = std::min(keys.size(), (size_t)sp.topk);
      for (size_t j = 0; j < take; ++j) {
        const int a = (int)(uint32_t)keys[j];
        npos[a] += 1;
        row[a] = m;
      }
    }
    for (int a = 0; a < A; ++a) {
      if (npos[a] == 0) continue;
      int fin = row[a];
      if (npos[a] > 1) {
        bool first = true;
        T bo = (T)0;
        for (int m = 0; m < M; ++m) {
          if (!present(gtc[m], C)) continue;
          const T o = ov[(size_t)m * sA + a];
          if (first || o > bo) { bo = o; fin = m; first = false; }
        }
      }
      tg[a] = fin;
    }
    std::vector<T> rov((size_t)M, (T)0), rmet((size_t)M, (T)0);
    for (int a = 0; a < A; ++a)
      if (tg[a] >= 0) {
        const int m = tg[a];
        rov[m] = std::max(rov[m], ov[(size_t)m * sA + a]);
        rmet[m] = std::max(rmet[m], met[(size_t)m * sA + a]);
      }
    for (int a = 0; a < A; ++a)
      if (tg[a] >= 0) tsb[a] = target_score<T>(met[(size_t)tg[a] * sA + a], rov[tg[a]], rmet[tg[a]]);
  }
  T ts_all = (T)0;                                   // k_detloss_assign's per-image sums, added in image order
  for (int b = 0; b < B; ++b) ts_all = ts_all + strided_tree_sum<T>(ts + (size_t)b * sA, sA, ASG_THREADS);
  const T tss = clamp_tss<T>(ts_all);

  // k_detloss_terms' grid: (anchor tiles, 1 + class chunks, images), V anchors per lane; a lane's partial sums
  const int V = A % 4 == 0 ? 4 : 1;
  const size_t per = (size_t)TERM_THREADS * (size_t)V, tiles = (sA + per - 1) / per;
  const size_t chunks = 1 + (size_t)((C + CLS_CHUNK - 1) / CLS_CHUNK), nblocks = tiles * chunks * (size_t)B;
  std::vector<T> l_box(nblocks * TERM_THREADS, (T)0), l_cls(nblocks * TERM_THREADS, (T)0), l_dfl(nblocks * TERM_THREADS, (T)0);
  auto lane_of = [&](int b, size_t chunk, int a) {
    const size_t tile = (size_t)a / per, t = ((size_t)a % per) / (size_t)V;
    return ((((size_t)b * chunks + chunk) * tiles + tile) * TERM_THREADS) + t;
  };
  const T fB = (T)B;
  std::vector<T> t_bce((size_t)C * sA);
  for (int b = 0; b < B; ++b) {
    for (int a = 0; a < A; ++a) {
      const size_t i = (size_t)b * sA + a;
      const T* pa = pred + (size_t)b * (size_t)K * sA + a;
      T* ga = grad ? grad + (size_t)b * (size_t)K * sA + a : nullptr;
      const int m = tgt[i];
      if (m >= 0) {
        float gx, gy, st;
        anchor_point(sp, a, gx, gy, st);
        const T w = ts[i] / tss;
        T bt, dt;
        box_dfl_anchor<T>(pa, sA, (T)gx, (T)gy, (T)st, gt_boxes + ((size_t)b * (size_t)M + (size_t)m) * 4, fB * (T)sp.w_box * w,
                          fB * (T)sp.w_dfl * w, ga, sA, bt, dt, frozen && ciou_a ? ciou_a + i : nullptr,
                          !frozen && ciou_a ? ciou_a + i : nullptr);
        const size_t ln = lane_of(b, 0, a);          // a lane takes its V anchors in index order, as this loop does
        l_box[ln] = l_box[ln] + bt * ts[i];
        l_dfl[ln] = l_dfl[ln] + dt * ts[i];
      } else if (ga) {
        for (int k = 0; k < BOX_CH; ++k) ga[(size_t)k * sA] = (T)0;
      }
      const int tc = m >= 0 ? gt_cls[(size_t)b * (size_t)M + (size_t)m] : -1;
      const T kc = fB * (T)sp.w_cls / tss;
      for (int c = 0; c < C; ++c) {
        T g;
        t_bce[(size_t)c * sA + a] = bce<T>(pa[(size_t)(BOX_CH + c) * sA], tc == c ? ts[i] : (T)0, &g);
        if (ga) ga[(size_t)(BOX_CH + c) * sA] = kc * g;
      }
    }
    // a lane of a class chunk adds class by class, and within a class its V anchors
    for (int c = 0; c < C; ++c)
      for (int a = 0; a < A; ++a) {
        const size_t ln = lane_of(b, 1 + (size_t)(c / CLS_CHUNK), a);
        l_cls[ln] = l_cls[ln] + t_bce[(size_t)c * sA + a];
      }
  }
  // every block's tree -> the slab, which k_detloss_final's one block adds
  std::vector<T> slab[3] = {std::vector<T>(nblocks), std::vector<T>(nblocks), std::vector<T>(nblocks)};
  std::vector<T>* lanes[3] = {&l_box, &l_cls, &l_dfl};
  T sums[3];
  for (int j = 0; j < 3; ++j) {
    for (size_t blk = 0; blk < nblocks; ++blk) {
      std::vector<T> v(lanes[j]->begin() + (ptrdiff_t)(blk * TERM_THREADS), lanes[j]->begin() + (ptrdiff_t)((blk + 1) * TERM_THREADS));
      slab[j][blk] = tree_sum(v);
    }
    sums[j] = strided_tree_sum<T>(slab[j].data(), nblocks, FIN_THREADS);
  }
  const T box = sums[0] / tss, cls = sums[1] / tss, dfl = sums[2] / tss;
  loss[0] = box;
  loss[1] = cls;
  loss[2] = dfl;
  loss[3] = fB * ((T)sp.w_box * box + (T)sp.w_cls * cls + (T)sp.w_dfl * dfl);
  return 0;
}

extern "C" {

int dlh_run_f32(const HostSpec* d, const float* pred, const float* gt_boxes, const int32_t* gt_cls, float* loss, float* grad,
                int32_t* tgt, float* ts, float* ciou_a, int frozen) {
  return run<float>(d, pred, gt_boxes, gt_cls, loss, grad, tgt, ts, ciou_a, frozen);
}

int dlh_run_f64(const HostSpec* d, const double* pred, const double* gt_boxes, const int32_t* gt_cls, double* loss, double* grad,
                int32_t* tgt, double* ts, double* ciou_a, int frozen) {
  return run<double>(d, pred, gt_boxes, gt_cls, loss, grad, tgt, ts, ciou_a, frozen);
}

}  // extern "C"
