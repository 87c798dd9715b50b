// The projected-gradient step on the CPU, from csrc/gsr_pgd.h -- the scalar source the HIP kernels compile -- in plain
// loops: the sum of squares of the gradient in double (or the one handed in, as gsr_pgd_step_normed takes it), then the
// step row by row.
//   ph_step           x[rows, cols] in place; l2 = 0 / 1; sumsq = NULL or one double
//   ph_rows_per_wave, ph_sumsq_blocks, ph_tensor_of_block   the launch arithmetic of gsr_api.hip, for the tests
// Build: g++ -O1 -ffp-contract=off -shared -fPIC -I <csrc> pgd_host.cpp -o libpgdhost.so
// With -DPGD_MAIN: a program that reads cases from a file (int32 count; per case int32 rows, cols, l2, has_sumsq, float
// alpha, eps, double sumsq, then x, grad, x0 of rows * cols floats each), runs each with buffers exactly as large as
// the shapes say, and prints one line per case -- for a build with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gsr_pgd.h"

using namespace gsr;

extern "C" int ph_step(float* x, const float* g, const float* x0, int64_t rows, int32_t cols, float alpha, float eps,
                       int32_t l2, const double* sumsq) {
  if (rows < 0 || cols < 1 || cols > PGD_MAX_COLS) return 1;
  if (rows == 0) return 0;
  if (!x || !g || !x0) return 1;
  const size_t n = (size_t)rows * (size_t)cols;
  if (!l2) {
    for (size_t i = 0; i < n; ++i) x[i] = pgd_linf_update(x[i], g[i], x0[i], alpha, eps);
    return 0;
  }
  double t = 0.0;
  if (sumsq) t = *sumsq;
  else for (size_t i = 0; i < n; ++i) t += (double)g[i] * (double)g[i];
  const float scale = pgd_l2_scale(t, alpha);
  float d[PGD_MAX_COLS];
  for (int64_t r = 0; r < rows; ++r) {
    const size_t b = (size_t)r * (size_t)cols;
    float ss = 0.f;
    for (int c = 0; c < cols; ++c) {
      d[c] = pgd_l2_move(x[b + c], g[b + c], scale) - x0[b + c];
      ss = pgd_row_accum(d[c], ss);
    }
    const float f = pgd_row_factor(sqrtf(ss), eps);
    for (int c = 0; c < cols; ++c) x[b + c] = pgd_l2_result(d[c], f, x0[b + c]);
  }
  return 0;
}

extern "C" int32_t ph_rows_per_wave(int32_t cols) { return pgd_rows_per_wave(cols); }
extern "C" int32_t ph_sumsq_blocks(uint64_t n) { return pgd_sumsq_blocks((size_t)n); }
extern "C" int32_t ph_tensor_of_block(const uint32_t* first, int32_t n, uint32_t b) { return pgd_tensor_of_block(first, n, b); }

#ifdef PGD_MAIN
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t ncases = 0;
  if (fread(&ncases, sizeof(ncases), 1, f) != 1) return 2;
  for (int32_t k = 0; k < ncases; ++k) {
    int32_t hd[4];
    float ae[2];
    double ss = 0.0;
    if (fread(hd, sizeof(int32_t), 4, f) != 4 || fread(ae, sizeof(float), 2, f) != 2 || fread(&ss, sizeof(ss), 1, f) != 1) return 2;
    if (hd[0] < 0 || hd[1] < 1) return 2;
    const size_t n = (size_t)hd[0] * (size_t)hd[1];
    std::vector<float> x(n), g(n), x0(n);
    if (n && (fread(x.data(), 4, n, f) != n || fread(g.data(), 4, n, f) != n || fread(x0.data(), 4, n, f) != n)) return 2;
    if (ph_step(x.data(), g.data(), x0.data(), hd[0], hd[1], ae[0], ae[1], hd[2], hd[3] ? &ss : nullptr)) return 3;
    uint32_t h = 2166136261u;   // FNV-1a over the result bits: the test compares it with the library's
    for (size_t i = 0; i < n; ++i) {
      uint32_t w;
      __builtin_memcpy(&w, &x[i], 4);
      for (int b = 0; b < 4; ++b) { h ^= (w >> (8 * b)) & 0xffu; h *= 16777619u; }
    }
    printf("case %d rows %d cols %d l2 %d hash %u\n", k, hd[0], hd[1], hd[2], h);
  }
  fclose(f);
  // the launch arithmetic at its edges: every block of a table with empty tensors first, in the middle and last
  const uint32_t first[PGD_MAX_TENSORS + 1] = {0, 0, 3, 3, 3, 7, 8, 8, 8};
  int sum = 0;
  for (uint32_t b = 0; b < 8; ++b) sum += pgd_tensor_of_block(first, 8, b);
  printf("cases %d lookup %d\n", ncases, sum);
  return 0;
}
#endif
