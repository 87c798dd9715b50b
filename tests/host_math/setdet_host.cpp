// The set-prediction detector stage in plain loops over csrc/gsr_setdet.h, the same scalar source the HIP kernels compile:
//   sdh_run_f32   float32, what gsr_setdet_loss computes (sums taken pairwise and a row's statistics in the wave's order, so
//                 that their rounding stays at the level of the kernels' trees instead of growing with the element count)
//   sdh_run_f64   the same code in double: tests/test_setdet_host_cpu.py differentiates its `total` by central differences
//                 to check the hand-written backward against its own forward
//   sdh_post_f32  what gsr_setdet_postprocess computes
// Build: g++ -O1 -ffp-contract=off -shared -fPIC -I <csrc> setdet_host.cpp -o libsetdethost.so
// With -DSETDET_MAIN it is a program: it reads cases from the file named on its command line (per case: int32 B Q C M,
// float32 img_w img_h, then logits, boxes, gt_boxes as float32 and gt_cls as int32), runs all three entries on each and
// prints match, tgt and the losses -- what the sanitizer build runs.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gsr_setdet.h"

using namespace gsr_setdet;

struct HostSpec {   // GsrSetDetSpec of include/gsraster.h
  int32_t B, Q, C, M;
  float img_w, img_h, c_class, c_l1, c_giou, w_ce, w_l1, w_giou, eos_coef, conf_thr;
  int32_t max_det;
  uint32_t flags;
};

template <class T>
static T pairwise(const T* v, size_t n) {
  if (n <= 8) {
    T s = (T)0;
    for (size_t i = 0; i < n; ++i) s = s + v[i];
    return s;
  }
  const size_t h = n / 2;
  return pairwise(v, h) + pairwise(v + h, n - h);
}

// The statistics of one row of n logits in the order k_setdet_cost takes them (gsr_block::wave_softmax_stats): 64 lanes
// stride the row, then an xor butterfly over the lanes.  A serial sum of 1025 exponentials rounds an order of magnitude
// more than that tree; softmax_stats stays what the output stage runs, on the device as here.
template <class T>
static void wave_stats(const T* x, int n, T& mx, T& sum) {
  T a[64], o[64];
  for (int l = 0; l < 64; ++l) {
    T m = -m_inf<T>();
    for (int k = l; k < n; k += 64) m = x[k] > m ? x[k] : m;
    a[l] = m;
  }
  for (int s = 32; s >= 1; s >>= 1) {
    for (int l = 0; l < 64; ++l) o[l] = a[l ^ s] > a[l] ? a[l ^ s] : a[l];
    for (int l = 0; l < 64; ++l) a[l] = o[l];
  }
  mx = a[0];
  for (int l = 0; l < 64; ++l) {
    T t = (T)0;
    for (int k = l; k < n; k += 64) t = t + m_exp(x[k] - mx);
    a[l] = t;
  }
  for (int s = 32; s >= 1; s >>= 1) {
    for (int l = 0; l < 64; ++l) o[l] = a[l] + a[l ^ s];
    for (int l = 0; l < 64; ++l) a[l] = o[l];
  }
  sum = a[0];
}

static bool spec_ok(const HostSpec* d) {
  return d && d->B >= 1 && d->B <= 65535 && d->Q >= 1 && d->Q <= MAX_QUERIES && d->C >= 1 && d->C <= MAX_CLASSES && d->M >= 1 &&
         d->M <= MAX_ROWS && d->Q >= d->M && d->max_det >= 1 && d->max_det <= MAX_QUERIES && d->flags == 0u;
}

// logits [B,Q,C+1], boxes [B,Q,4], gt_boxes [B,M,4], gt_cls [B,M] -> loss[4], grad_logits / grad_boxes or NULL,
// match [B,M], tgt [B,Q]; cost [B,M,Q] (may be NULL): the cost matrix, zeros in absent rows.
// frozen: match and tgt are INPUTS and the match is not run -- the contract differentiates nothing in it, so this is the
// function of (logits, boxes) whose derivative the gradients are.
template <class T>
static int run(const HostSpec* d, const T* logits, const T* boxes, const T* gt_boxes, const int32_t* gt_cls, T* loss,
               T* grad_logits, T* grad_boxes, int32_t* match, int32_t* tgt, T* cost_out, int frozen) {
  if (!spec_ok(d)) return 1;
  const int B = d->B, Q = d->Q, C = d->C, M = d->M, n1 = C + 1;
  const size_t BQ = (size_t)B * (size_t)Q;
  std::vector<T> mx(BQ), sum(BQ);
  for (size_t i = 0; i < BQ; ++i) wave_stats<T>(logits + i * (size_t)n1, n1, mx[i], sum[i]);
  if (!frozen) {
    std::vector<T> cost((size_t)M * (size_t)Q), u((size_t)M + 1), v((size_t)Q + 1), minv((size_t)Q + 1);
    std::vector<int32_t> p((size_t)Q + 1), way((size_t)Q + 1), used((size_t)Q + 1);
    for (int b = 0; b < B; ++b) {
      const int32_t* cls = gt_cls + (size_t)b * (size_t)M;
      for (int m = 0; m < M; ++m) {
        T gt[4] = {(T)0, (T)0, (T)0, (T)0};
        const bool pres = present(cls[m], C);
        if (pres) gt_normalise<T>(gt_boxes + ((size_t)b * (size_t)M + (size_t)m) * 4, (T)d->img_w, (T)d->img_h, gt);
        for (int q = 0; q < Q; ++q) {
          const size_t i = (size_t)b * (size_t)Q + (size_t)q;
          T c = (T)0;
          if (pres)
            c = pair_cost<T>(softmax_prob<T>(logits[i * (size_t)n1 + (size_t)cls[m]], mx[i], sum[i]), boxes + i * 4, gt, (T)d->c_class,
                             (T)d->c_l1, (T)d->c_giou);
          cost[(size_t)m * (size_t)Q + (size_t)q] = c;
          if (cost_out) cost_out[((size_t)b * (size_t)M + (size_t)m) * (size_t)Q + (size_t)q] = c;
        }
      }
      match_rows<T>(cost.data(), cls, M, Q, C, u.data(), v.data(), minv.data(), p.data(), way.data(), used.data(),
                    match + (size_t)b * (size_t)M, tgt + (size_t)b * (size_t)Q);
    }
  }
  long long matched = 0;
  for (size_t i = 0; i < BQ; ++i) matched += tgt[i] >= 0 && tgt[i] < M ? 1 : 0;
  const T nb = norm_boxes<T>(matched), wsum = norm_ce<T>(matched, (long long)BQ, (T)d->eos_coef);
  const T kce = (T)d->w_ce / wsum, kl1 = (T)d->w_l1 / nb, kg = (T)d->w_giou / nb;
  std::vector<T> t_ce(BQ, (T)0), t_l1(BQ, (T)0), t_g(BQ, (T)0);
  for (int b = 0; b < B; ++b)
    for (int q = 0; q < Q; ++q) {
      const size_t i = (size_t)b * (size_t)Q + (size_t)q;
      int tg = tgt[i];
      tg = tg >= 0 && tg < M ? tg : -1;
      int tc = tg >= 0 ? gt_cls[(size_t)b * (size_t)M + (size_t)tg] : C;
      tc = present(tc, C) ? tc : C;
      const T wt = tc == C ? (T)d->eos_coef : (T)1;
      const T* x = logits + i * (size_t)n1;
      t_ce[i] = wt * -log_softmax<T>(x[tc], mx[i], sum[i]);
      if (grad_logits)
        for (int c = 0; c < n1; ++c)
          grad_logits[i * (size_t)n1 + (size_t)c] = (kce * wt) * (softmax_prob<T>(x[c], mx[i], sum[i]) - (c == tc ? (T)1 : (T)0));
      T* gb = grad_boxes ? grad_boxes + i * 4 : nullptr;
      if (tg >= 0) {
        T gt[4];
        gt_normalise<T>(gt_boxes + ((size_t)b * (size_t)M + (size_t)tg) * 4, (T)d->img_w, (T)d->img_h, gt);
        pair_terms<T>(boxes + i * 4, gt, kl1, kg, gb, t_l1[i], t_g[i]);
      } else if (gb) {
        for (int k = 0; k < 4; ++k) gb[k] = (T)0;
      }
    }
  const T ce = pairwise<T>(t_ce.data(), BQ) / wsum, l1 = pairwise<T>(t_l1.data(), BQ) / nb, gi = pairwise<T>(t_g.data(), BQ) / nb;
  loss[0] = ce;
  loss[1] = l1;
  loss[2] = gi;
  loss[3] = (T)d->w_ce * ce + (T)d->w_l1 * l1 + (T)d->w_giou * gi;
  return 0;
}

template <class T>
static int post(const HostSpec* d, const T* logits, const T* boxes, T* dets, int32_t* counts) {
  if (!spec_ok(d)) return 1;
  const int B = d->B, Q = d->Q, C = d->C, n1 = C + 1;
  for (int b = 0; b < B; ++b) {
    T* out = dets + (size_t)b * (size_t)d->max_det * 6;
    for (int i = 0; i < d->max_det * 6; ++i) out[i] = (T)0;
    int above = 0;
    for (int q = 0; q < Q; ++q) {
      const size_t i = (size_t)b * (size_t)Q + (size_t)q;
      const T* x = logits + i * (size_t)n1;
      T mx, sum;
      softmax_stats<T>(x, n1, mx, sum);
      T bp = -m_inf<T>();
      int bc = 0x7fffffff;
      for (int c = 0; c < C; ++c) {
        const T p = softmax_prob<T>(x[c], mx, sum);
        if (score_better<T>(p, c, bp, bc)) { bp = p; bc = c; }
      }
      if (!(bp > (T)d->conf_thr)) continue;
      if (above < d->max_det) {
        T* row = out + (size_t)above * 6;
        out_box<T>(boxes + i * 4, (T)d->img_w, (T)d->img_h, row);
        row[4] = bp;
        row[5] = (T)(bc < C ? bc : 0);
      }
      ++above;
    }
    counts[(size_t)b * 2] = above < d->max_det ? above : d->max_det;
    counts[(size_t)b * 2 + 1] = above;
  }
  return 0;
}

extern "C" {

int sdh_run_f32(const HostSpec* d, const float* logits, const float* boxes, const float* gt_boxes, const int32_t* gt_cls, float* loss,
                float* grad_logits, float* grad_boxes, int32_t* match, int32_t* tgt, float* cost, int frozen) {
  return run<float>(d, logits, boxes, gt_boxes, gt_cls, loss, grad_logits, grad_boxes, match, tgt, cost, frozen);
}

int sdh_run_f64(const HostSpec* d, const double* logits, const double* boxes, const double* gt_boxes, const int32_t* gt_cls,
                double* loss, double* grad_logits, double* grad_boxes, int32_t* match, int32_t* tgt, double* cost, int frozen) {
  return run<double>(d, logits, boxes, gt_boxes, gt_cls, loss, grad_logits, grad_boxes, match, tgt, cost, frozen);
}

int sdh_post_f32(const HostSpec* d, const float* logits, const float* boxes, float* dets, int32_t* counts) {
  return post<float>(d, logits, boxes, dets, counts);
}

}  // extern "C"

#ifdef SETDET_MAIN
template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[4];
  int k = 0;
  while (fread(hdr, sizeof(int32_t), 4, f) == 4) {
    float wh[2];
    if (fread(wh, sizeof(float), 2, f) != 2) return 3;
    HostSpec d = {hdr[0], hdr[1], hdr[2], hdr[3], wh[0], wh[1], 1.0f, 5.0f, 2.0f, 1.0f, 5.0f, 2.0f, 0.1f, 0.7f, hdr[1], 0u};
    if (!spec_ok(&d)) return 3;
    const size_t BQ = (size_t)d.B * (size_t)d.Q, BM = (size_t)d.B * (size_t)d.M, n1 = (size_t)d.C + 1;
    std::vector<float> logits, boxes, gtb;
    std::vector<int32_t> gtc;
    if (!read_n(f, logits, BQ * n1) || !read_n(f, boxes, BQ * 4) || !read_n(f, gtb, BM * 4) || !read_n(f, gtc, BM)) return 3;
    std::vector<float> gl(BQ * n1), gbx(BQ * 4), dets(BQ * 6), cost(BM * (size_t)d.Q);
    std::vector<int32_t> match(BM), tgt(BQ), counts((size_t)d.B * 2);
    float loss[4];
    if (sdh_run_f32(&d, logits.data(), boxes.data(), gtb.data(), gtc.data(), loss, gl.data(), gbx.data(), match.data(), tgt.data(),
                    cost.data(), 0))
      return 4;
    std::vector<double> l64(logits.begin(), logits.end()), b64(boxes.begin(), boxes.end()), g64(gtb.begin(), gtb.end());
    std::vector<double> gl64(BQ * n1), gb64(BQ * 4);
    std::vector<int32_t> match64(BM), tgt64(BQ);
    double loss64[4];
    if (sdh_run_f64(&d, l64.data(), b64.data(), g64.data(), gtc.data(), loss64, gl64.data(), gb64.data(), match64.data(), tgt64.data(),
                    nullptr, 0))
      return 4;
    if (sdh_post_f32(&d, logits.data(), boxes.data(), dets.data(), counts.data())) return 4;
    printf("case %d match", k);
    for (size_t i = 0; i < BM; ++i) printf(" %d", match[i]);
    printf("\ncase %d match64", k);
    for (size_t i = 0; i < BM; ++i) printf(" %d", match64[i]);
    printf("\ncase %d loss %.9g %.9g %.9g %.9g loss64 %.17g %.17g %.17g %.17g kept", k, loss[0], loss[1], loss[2], loss[3], loss64[0],
           loss64[1], loss64[2], loss64[3]);
    for (int b = 0; b < d.B; ++b) printf(" %d", counts[(size_t)b * 2]);
    printf("\n");
    ++k;
  }
  fclose(f);
  printf("cases %d\n", k);
  return 0;
}
#endif
