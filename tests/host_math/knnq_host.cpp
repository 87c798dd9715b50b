// gsr_knn_query and gsr_knn_gather_mean on the CPU, from csrc/gsr_knnq.h -- the scalar source the HIP kernels compile -- in
// plain loops that mirror the device pipeline step by step: the references' bounding box (fminf / fmaxf, so a NaN
// coordinate is dropped as in k_knn_bbox), the grid, one key per reference, a stable sort by key (identity for a single
// cell), the cells' ranges, the cell-sorted copy of the references, and the search of every query.
//   kq_query        out_idx [Q,k], out_d2 [Q,k], how every query finished (KNN_FIN_* / KNNQ_FIN_*), and the grid's dims
//   kq_gather_mean  one tensor [R,cols] -> [Q,cols] through idx [Q,k], element by element with knnq_mean
// Build: g++ -O1 -ffp-contract=off -shared -fPIC -I <csrc> knnq_host.cpp -o libknnqhost.so
// With -DKNNQ_MAIN: a stand-alone program over a file of cases, for a build under the sanitizers (see its comment below).
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "gsr_knnq.h"

using namespace gsr;

struct Range { uint32_t x, y; };

static uint32_t ceil_log2(uint32_t v) {
  uint32_t b = 0;
  while ((1ull << b) < v) ++b;
  return b;
}

template <int K>
static void run_queries(const std::vector<KnnqRef>& staged, int R, const KnnGrid& g, const std::vector<Range>& cell_range,
                        const float* qry, int Q, bool exclude, const float bb[6], int32_t* out_idx, float* out_d2,
                        int32_t* finish) {
  for (int q = 0; q < Q; ++q) {
    KnnqBest<K> best;
    int fin = -1;
    const float* p = qry + 3 * (size_t)q;
    knnq_search_point<K>(p[0], p[1], p[2], exclude ? q : -1, staged.data(), R, g, cell_range.data(), best, &fin);
    bool outside = false;
    for (int a = 0; a < 3; ++a) outside = outside || p[a] < bb[a] || p[a] > bb[3 + a];
    if (outside && !(fin & KNNQ_FIN_NONFINITE)) fin |= KNNQ_FIN_OUTSIDE;
    finish[q] = fin;
    for (int j = 0; j < K; ++j) {
      out_idx[(size_t)q * K + j] = best.i[j];
      if (out_d2) out_d2[(size_t)q * K + j] = (float)best.d[j];
    }
  }
}

extern "C" int kq_query(const float* ref, int32_t R, const float* qry, int32_t Q, int32_t k, uint32_t flags, int32_t* out_idx,
                        float* out_d2, int32_t* finish, int32_t* dims) {
  if (k < 1 || k > KNNQ_MAX_K || R < 0 || Q < 0 || (flags & ~KNNQ_EXCLUDE_SAME_INDEX) || !dims) return 1;
  if ((flags & KNNQ_EXCLUDE_SAME_INDEX) && Q != R) return 1;
  if ((R > 0 && !ref) || (Q > 0 && (!qry || !out_idx || !finish))) return 1;
  dims[0] = dims[1] = dims[2] = 0;
  if (Q == 0) return 0;
  if (R == 0) {
    for (size_t i = 0; i < (size_t)Q * (size_t)k; ++i) { out_idx[i] = -1; if (out_d2) out_d2[i] = INFINITY; }
    for (int q = 0; q < Q; ++q) finish[q] = 0;
    return 0;
  }
  const size_t n = (size_t)R;
  float bb[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (size_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) { bb[a] = fminf(bb[a], ref[3 * i + a]); bb[3 + a] = fmaxf(bb[3 + a], ref[3 * i + a]); }
  const KnnGrid g = knn_make_grid(bb, R);
  dims[0] = g.dx; dims[1] = g.dy; dims[2] = g.dz;
  const uint32_t ncells = (uint32_t)g.dx * g.dy * g.dz;
  std::vector<uint32_t> keys(n), idx(n);
  for (size_t i = 0; i < n; ++i) keys[i] = knn_cell_key(ref, (int)i, g);
  std::iota(idx.begin(), idx.end(), 0u);
  if (ceil_log2(ncells) != 0)
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  std::vector<Range> cell_range((size_t)ncells, Range{0u, 0u});
  std::vector<KnnqRef> staged(n);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t o = idx[i], c = keys[o];
    if (i == 0 || keys[idx[i - 1]] != c) cell_range[c].x = (uint32_t)i;
    if (i == n - 1 || keys[idx[i + 1]] != c) cell_range[c].y = (uint32_t)i + 1;
    staged[i].x = ref[3 * (size_t)o]; staged[i].y = ref[3 * (size_t)o + 1]; staged[i].z = ref[3 * (size_t)o + 2];
    staged[i].idx = (int32_t)o;
  }
  const bool ex = (flags & KNNQ_EXCLUDE_SAME_INDEX) != 0;
  switch (k) {
    case 1: run_queries<1>(staged, R, g, cell_range, qry, Q, ex, bb, out_idx, out_d2, finish); break;
    case 2: run_queries<2>(staged, R, g, cell_range, qry, Q, ex, bb, out_idx, out_d2, finish); break;
    case 3: run_queries<3>(staged, R, g, cell_range, qry, Q, ex, bb, out_idx, out_d2, finish); break;
    case 4: run_queries<4>(staged, R, g, cell_range, qry, Q, ex, bb, out_idx, out_d2, finish); break;
    case 5: run_queries<5>(staged, R, g, cell_range, qry, Q, ex, bb, out_idx, out_d2, finish); break;
    case 6: run_queries<6>(staged, R, g, cell_range, qry, Q, ex, bb, out_idx, out_d2, finish); break;
    case 7: run_queries<7>(staged, R, g, cell_range, qry, Q, ex, bb, out_idx, out_d2, finish); break;
    default: run_queries<8>(staged, R, g, cell_range, qry, Q, ex, bb, out_idx, out_d2, finish); break;
  }
  return 0;
}

#ifdef KNNQ_MAIN
// A program that reads cases from a file (int32 count; per case int32 R, Q, k, flags, then R * 3 and Q * 3 floats), runs each
// with buffers exactly as large as the shapes say, gathers a [R,3] tensor (the references themselves) through the result, and
// prints one line per case -- for a build with -fsanitize=address,undefined.
#include <cstdio>
extern "C" int kq_gather_mean(const int32_t* idx, int32_t Q, int32_t k, int32_t R, const float* src, int32_t cols, float* dst);

static uint32_t fnv1a(uint32_t h, const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 16777619u; }
  return h;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t ncases = 0;
  if (fread(&ncases, sizeof(ncases), 1, f) != 1) return 2;
  for (int32_t c = 0; c < ncases; ++c) {
    int32_t h4[4];
    if (fread(h4, sizeof(int32_t), 4, f) != 4 || h4[0] < 0 || h4[1] < 0) return 2;
    const int32_t R = h4[0], Q = h4[1], k = h4[2];
    std::vector<float> ref((size_t)R * 3), qry((size_t)Q * 3);
    if (R && fread(ref.data(), sizeof(float), ref.size(), f) != ref.size()) return 2;
    if (Q && fread(qry.data(), sizeof(float), qry.size(), f) != qry.size()) return 2;
    std::vector<int32_t> idx((size_t)Q * k), fin((size_t)Q);
    std::vector<float> d2((size_t)Q * k), mean((size_t)Q * 3);
    int32_t dims[3];
    if (kq_query(R ? ref.data() : nullptr, R, Q ? qry.data() : nullptr, Q, k, (uint32_t)h4[3], Q ? idx.data() : nullptr,
                 Q ? d2.data() : nullptr, Q ? fin.data() : nullptr, dims)) return 3;
    if (kq_gather_mean(Q ? idx.data() : nullptr, Q, k, R, R ? ref.data() : nullptr, 3, Q ? mean.data() : nullptr)) return 3;
    uint32_t h = 2166136261u;   // FNV-1a over the result bytes: the test compares it with the library's
    h = fnv1a(h, idx.data(), idx.size() * 4);
    h = fnv1a(h, d2.data(), d2.size() * 4);
    h = fnv1a(h, fin.data(), fin.size() * 4);
    printf("case %d R %d Q %d k %d dims %d %d %d hash %u\n", c, R, Q, k, dims[0], dims[1], dims[2], h);
  }
  fclose(f);
  printf("cases %d\n", ncases);
  return 0;
}
#endif

extern "C" int kq_gather_mean(const int32_t* idx, int32_t Q, int32_t k, int32_t R, const float* src, int32_t cols, float* dst) {
  if (k < 1 || k > KNNQ_MAX_K || R < 0 || Q < 0 || cols < 1 || cols > KNNQ_MAX_COLS) return 1;
  if (Q > 0 && (!idx || !dst || (R > 0 && !src))) return 1;
  for (int q = 0; q < Q; ++q)
    for (int c = 0; c < cols; ++c) dst[(size_t)q * cols + c] = knnq_mean(idx + (size_t)q * k, k, R, src, cols, c);
  return 0;
}
