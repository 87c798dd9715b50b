// The fused Adam step on the CPU, from csrc/gsr_adam.h -- the scalar source the HIP kernel compiles -- in plain loops.
//   ah_step_multi     gsr_adam_step_multi's arguments without the stream; the same refusals (return 1), the same result
//   ah_bias           step_size and sqrt_bc2 of a step count, as the entry point forms them
//   ah_expon_lr       the position schedule
//   ah_span, ah_blocks, ah_tensor_of_block, ah_row_of    the launch arithmetic, for the tests
// Build: g++ -O1 -ffp-contract=off -shared -fPIC -I <csrc> adam_host.cpp -o libadamhost.so
// With -DADAM_MAIN: a program that reads calls from a file (int32 count; per call int32 n, has_mask; int64 step, row_begin,
// row_end; per tensor int64 rows, int32 cols, float lr, b1, b2, eps, int32 shift; the mask bytes if any; then per tensor x, g,
// m, v of rows * cols floats each), runs each with buffers exactly as large as the shapes say (shift: the tensor starts
// that many floats into its buffer), and prints one line per call -- for a build with -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gsr_adam.h"

using namespace gsr;

extern "C" int ah_step_multi(int32_t n, float* const* x, const float* const* g, float* const* m, float* const* v, const int64_t* rows,
                             const int32_t* cols, const float* lr, const float* beta1, const float* beta2, const float* eps, int64_t step,
                             const uint8_t* row_mask, int64_t row_begin, int64_t row_end) {
  if (n < 1 || n > ADAM_MAX_TENSORS || step < 1) return 1;
  if (!x || !g || !m || !v || !rows || !cols || !lr || !beta1 || !beta2 || !eps) return 1;
  const bool selected = row_mask != nullptr || row_begin != 0 || row_end != -1;
  for (int t = 0; t < n; ++t) {
    if (rows[t] < 0 || cols[t] < 1 || cols[t] > ADAM_MAX_COLS) return 1;
    if (rows[t] > 0 && (!x[t] || !g[t] || !m[t] || !v[t])) return 1;
    if (selected && rows[t] != rows[0]) return 1;
    if (!std::isfinite(lr[t]) || !std::isfinite(beta1[t]) || !std::isfinite(beta2[t]) || !std::isfinite(eps[t])) return 1;
    if (!(beta1[t] >= 0.f && beta1[t] < 1.f) || !(beta2[t] >= 0.f && beta2[t] < 1.f) || eps[t] < 0.f) return 1;
  }
  unsigned long long rb = 0, re = 0;
  if (selected) {
    if (row_end == -1) row_end = rows[0];
    if (row_begin < 0 || row_begin > row_end || row_end > rows[0]) return 1;
    rb = (unsigned long long)row_begin; re = (unsigned long long)row_end;
  }
  for (int t = 0; t < n; ++t) {
    float ss, sb;
    adam_bias_corrections((double)lr[t], (double)beta1[t], (double)beta2[t], (long long)step, &ss, &sb);
    const unsigned long long ne = (unsigned long long)rows[t] * (unsigned long long)cols[t];
    for (unsigned long long e = 0; e < ne; ++e) {
      if (selected && !adam_row_live(adam_row_of(e, cols[t]), row_mask, rb, re)) continue;
      adam_update(x[t][e], g[t][e], m[t][e], v[t][e], ss, sb, beta1[t], beta2[t], eps[t]);
    }
  }
  return 0;
}

extern "C" void ah_bias(double lr, double b1, double b2, int64_t t, float* step_size, float* sqrt_bc2) {
  adam_bias_corrections(lr, b1, b2, (long long)t, step_size, sqrt_bc2);
}
extern "C" double ah_expon_lr(int64_t step, double lr_init, double lr_final, int64_t delay_steps, double delay_mult, int64_t max_steps) {
  return expon_lr((long long)step, lr_init, lr_final, (long long)delay_steps, delay_mult, (long long)max_steps);
}
extern "C" int32_t ah_span() { return ADAM_SPAN; }
extern "C" uint64_t ah_blocks(uint64_t n) { return adam_blocks(n); }
extern "C" int32_t ah_tensor_of_block(const uint32_t* first, int32_t n, uint32_t b) { return adam_tensor_of_block(first, n, b); }
extern "C" uint64_t ah_row_of(uint64_t e, int32_t cols) { return adam_row_of(e, cols); }

#ifdef ADAM_MAIN
static uint32_t fnv(uint32_t h, const float* p, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t w;
    __builtin_memcpy(&w, &p[i], 4);
    for (int b = 0; b < 4; ++b) { h ^= (w >> (8 * b)) & 0xffu; h *= 16777619u; }
  }
  return h;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t ncalls = 0;
  if (fread(&ncalls, sizeof(ncalls), 1, f) != 1) return 2;
  for (int32_t k = 0; k < ncalls; ++k) {
    int32_t hd[2];
    int64_t sr[3];
    if (fread(hd, sizeof(int32_t), 2, f) != 2 || fread(sr, sizeof(int64_t), 3, f) != 3) return 2;
    const int n = hd[0];
    if (n < 1 || n > ADAM_MAX_TENSORS) return 2;
    int64_t rows[ADAM_MAX_TENSORS];
    int32_t cols[ADAM_MAX_TENSORS], shift[ADAM_MAX_TENSORS];
    float lr[ADAM_MAX_TENSORS], b1[ADAM_MAX_TENSORS], b2[ADAM_MAX_TENSORS], eps[ADAM_MAX_TENSORS];
    for (int t = 0; t < n; ++t) {
      float p[4];
      if (fread(&rows[t], 8, 1, f) != 1 || fread(&cols[t], 4, 1, f) != 1 || fread(p, 4, 4, f) != 4 || fread(&shift[t], 4, 1, f) != 1) return 2;
      lr[t] = p[0]; b1[t] = p[1]; b2[t] = p[2]; eps[t] = p[3];
      if (rows[t] < 0 || cols[t] < 1 || shift[t] < 0 || shift[t] > 3) return 2;
    }
    std::vector<uint8_t> mask;
    if (hd[1]) {
      mask.resize((size_t)rows[0]);
      if (!mask.empty() && fread(mask.data(), 1, mask.size(), f) != mask.size()) return 2;
    }
    std::vector<std::vector<float>> buf(4 * (size_t)n);
    float* px[ADAM_MAX_TENSORS]; const float* pg[ADAM_MAX_TENSORS]; float* pm[ADAM_MAX_TENSORS]; float* pv[ADAM_MAX_TENSORS];
    for (int t = 0; t < n; ++t) {
      const size_t ne = (size_t)rows[t] * (size_t)cols[t];
      for (int s = 0; s < 4; ++s) {
        std::vector<float>& b = buf[4 * (size_t)t + s];
        b.resize(ne + (size_t)shift[t]);
        if (ne && fread(b.data() + shift[t], 4, ne, f) != ne) return 2;
      }
      px[t] = ne ? buf[4 * t].data() + shift[t] : nullptr;
      pg[t] = ne ? buf[4 * t + 1].data() + shift[t] : nullptr;
      pm[t] = ne ? buf[4 * t + 2].data() + shift[t] : nullptr;
      pv[t] = ne ? buf[4 * t + 3].data() + shift[t] : nullptr;
    }
    if (ah_step_multi(n, px, pg, pm, pv, rows, cols, lr, b1, b2, eps, sr[0], hd[1] ? mask.data() : nullptr, sr[1], sr[2])) return 3;
    uint32_t h = 2166136261u;     // FNV-1a over the bits of x, m, v of every tensor: the test compares it with the library's
    for (int t = 0; t < n; ++t) {
      const size_t ne = (size_t)rows[t] * (size_t)cols[t];
      if (!ne) continue;
      h = fnv(h, px[t], ne); h = fnv(h, pm[t], ne); h = fnv(h, pv[t], ne);
    }
    printf("call %d tensors %d step %lld hash %u\n", k, n, (long long)sr[0], h);
  }
  fclose(f);
  // the launch arithmetic at its edges: every block of a table with empty tensors first, in the middle and last
  const uint32_t first[ADAM_MAX_TENSORS + 1] = {0, 0, 3, 3, 3, 7, 8, 8, 8};
  int sum = 0;
  for (uint32_t b = 0; b < 8; ++b) sum += adam_tensor_of_block(first, 8, b);
  printf("calls %d lookup %d\n", ncalls, sum);
  return 0;
}
#endif
