// gsr_knn_dist2 on the CPU, from csrc/gsr_knn.h -- the scalar source the HIP kernels compile -- in plain loops that mirror
// the device pipeline step by step: bounding box (fminf / fmaxf, so a NaN coordinate is dropped as in k_knn_bbox), the
// grid, one key per point, a stable sort by key (the radix sort is stable; no pass runs for a single cell, where the
// identity permutation is written by hand as gsr_api.hip does), the cells' ranges, and the search of every point.
//   kh_dist2   out[P], how every point finished (KNN_FIN_* of gsr_knn.h), and the grid's dims
// Build: g++ -O1 -ffp-contract=off -shared -fPIC -I <csrc> knn_host.cpp -o libknnhost.so
// With -DKNN_MAIN: a program that reads cases from a file (int32 count; per case int32 P, then P * 3 floats), runs each
// with buffers exactly as large as the shapes say, and prints one line per case -- for a build with
// -fsanitize=address,undefined.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "gsr_knn.h"

using namespace gsr;

struct Range { uint32_t x, y; };

static uint32_t ceil_log2(uint32_t v) {
  uint32_t b = 0;
  while ((1ull << b) < v) ++b;
  return b;
}

extern "C" int kh_dist2(const float* pts, int32_t P, float* out, int32_t* finish, int32_t* dims) {
  if (P < 0 || (P > 0 && (!pts || !out || !finish)) || !dims) return 1;
  dims[0] = dims[1] = dims[2] = 0;
  if (P == 0) return 0;
  const size_t n = (size_t)P;
  float bb[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (size_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) { bb[a] = fminf(bb[a], pts[3 * i + a]); bb[3 + a] = fmaxf(bb[3 + a], pts[3 * i + a]); }
  const KnnGrid g = knn_make_grid(bb, P);
  dims[0] = g.dx; dims[1] = g.dy; dims[2] = g.dz;
  const uint32_t ncells = (uint32_t)g.dx * g.dy * g.dz;
  std::vector<uint32_t> keys(n), idx(n), skeys(n);
  for (size_t i = 0; i < n; ++i) keys[i] = knn_cell_key(pts, (int)i, g);
  if (ceil_log2(ncells) == 0) {   // a single cell: no sort pass, the identity permutation by hand
    for (size_t i = 0; i < n; ++i) idx[i] = (uint32_t)i;
  } else {
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    idx = order;
  }
  for (size_t i = 0; i < n; ++i) skeys[i] = keys[idx[i]];
  std::vector<Range> cell_range((size_t)ncells, Range{0u, 0u});
  for (size_t i = 0; i < n; ++i) {
    const uint32_t c = skeys[i];
    if (i == 0 || skeys[i - 1] != c) cell_range[c].x = (uint32_t)i;
    if (i == n - 1 || skeys[i + 1] != c) cell_range[c].y = (uint32_t)i + 1;
  }
  for (size_t s = 0; s < n; ++s) {
    int fin = -1;
    knn_search_point((int)s, pts, P, g, idx.data(), cell_range.data(), out, &fin);
    finish[idx[s]] = fin;
  }
  return 0;
}

#ifdef KNN_MAIN
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t ncases = 0;
  if (fread(&ncases, sizeof(ncases), 1, f) != 1) return 2;
  for (int32_t k = 0; k < ncases; ++k) {
    int32_t P = 0;
    if (fread(&P, sizeof(P), 1, f) != 1 || P < 0) return 2;
    std::vector<float> pts((size_t)P * 3), out((size_t)P);
    std::vector<int32_t> fin((size_t)P);
    if (P && fread(pts.data(), sizeof(float), pts.size(), f) != pts.size()) return 2;
    int32_t dims[3];
    if (kh_dist2(pts.data(), P, out.data(), fin.data(), dims)) return 3;
    int fallback = 0, whole = 0, shell = 0;
    uint32_t h = 2166136261u;   // FNV-1a over the result bits: the test compares it with the library's
    for (int32_t i = 0; i < P; ++i) {
      if (fin[(size_t)i] < 0) return 4;
      fallback += (fin[(size_t)i] & KNN_FIN_FALLBACK) != 0;
      whole += (fin[(size_t)i] & KNN_FIN_WHOLE_GRID) != 0;
      shell = std::max(shell, fin[(size_t)i] & KNN_FIN_SHELL);
      uint32_t w;
      __builtin_memcpy(&w, &out[(size_t)i], 4);
      for (int b = 0; b < 4; ++b) { h ^= (w >> (8 * b)) & 0xffu; h *= 16777619u; }
    }
    printf("case %d P %d dims %d %d %d fallback %d whole %d shell %d hash %u\n", k, P, dims[0], dims[1], dims[2], fallback, whole,
           shell, h);
  }
  fclose(f);
  printf("cases %d\n", ncases);
  return 0;
}
#endif
