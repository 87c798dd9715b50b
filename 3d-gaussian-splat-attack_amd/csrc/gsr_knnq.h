// gsr_knnq.h -- the scalar side of the exact k-nearest-neighbour QUERY with indices between two point sets
// (gsr_knn_query, gsr_knn_gather_mean, include/gsraster.h): the distance, the k sorted slots, the search of one query point
// and the mean of one gathered element.  It stands on the grid of gsr_knn.h (KnnGrid, knn_make_grid, knn_cell_coord,
// knn_cell_key), which it uses unchanged.
//
// One source, compiled twice: by hipcc into the kernels of gsr_knnq.hip.h and by g++ into a host harness
// (tests/host_math/knnq_host.cpp) that runs the whole pipeline on the CPU and reports how every query finished.  Unlike
// gsr_knn.h the two builds give the SAME BITS: every function that rounds is GSR_FP_STRICT (no contraction).
//
// The contract (include/gsraster.h repeats it):
//   * Distance.  d2 = (dx*dx + dy*dy) + dz*dz in DOUBLE from the float32 coordinates, every difference formed in double,
//     evaluated in exactly that order without contraction: g++, hipcc and numpy float64 give the same bits.  Double is
//     chosen for exactness -- the order of two references must not depend on a float32 rounding of coordinates at a large
//     offset, and a test can then ask for equality -- not for speed: nobody has measured fp64 throughput in this search.
//   * Order.  A query's neighbours are the k smallest references under the total order (d2 ascending, reference index
//     ascending), written in that order.  Ties are decided, so the result does not depend on the order of the scan.
//   * Non-finite values.  A d2 that is NaN or +inf is never a neighbour; a query with a non-finite coordinate has no
//     neighbours; a non-finite reference is invisible to every query.  (Squares of finite floats cannot overflow a double.)
//   * Missing neighbours (R < k, the excluded reference, non-finite references): index -1 and d2 = +inf, behind the present.
//   * KNNQ_EXCLUDE_SAME_INDEX (flag bit 0): query i never takes reference i -- the self-query, which needs Q == R.
//   * knnq_mean: one output element is (((v0 + v1) + v2) ...) / m in float32 over the m present neighbours in rank order,
//     0 when m == 0.  An index outside 0 .. R-1 counts as missing and is never followed.
//
// Why the search is exact.  After shell r every reference binned inside the (2r+1)^3 block of cells around the query's
// (clamped) cell has been offered to the slots.  A reference binned OUTSIDE the block lies beyond one of the block's faces
// that is not a face of the grid, so along that axis it is at least `gap` away from the query, gap = the distance from the
// query's own coordinate to that face (0 when the face is on the wrong side of the query).  The binning rounds in float32:
// fl(fl(v - min) * inv) against an integer is off by at most 2^-22 of the grid's extent along the axis, and the gap is
// formed in double, so gap * 0.9999 - extent * 2^-20 (never below 0) is a true lower bound `safe` of that reference's
// distance.  The search stops when slot[k-1].d2 < safe^2, STRICTLY: every unscanned reference then has d2 >= safe^2 >
// slot[k-1].d2 >= the d2 of every kept one, so it follows all of them under (d2, index) whatever its index is.  With <=
// an unscanned reference at exactly the k-th distance and a lower index would have been missed.  A query outside the
// references' bounding box has a clamped cell; the bound holds for it unchanged (its gaps only grow), it pays with more
// shells or with the full sweep.  A query that has not stopped after KNN_MAX_SHELL shells takes the full sweep.
//
// Known limit, not measured (as in gsr_knn.h): the grid is uniform over the references' bounding box.  One far reference
// or one infinite coordinate collapses it to a few cells and the search turns quadratic in the references that share a
// cell.  Results stay exact; nobody has measured the run time of such a cloud.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gsr_knn.h"    // KnnGrid, knn_make_grid, knn_cell_coord, knn_cell_key, KNN_MAX_SHELL, KNN_FIN_*
#include "gsr_math.h"   // GSR_HD, GSR_FP_STRICT

namespace gsr {

constexpr int KNNQ_MAX_K = 8;
constexpr uint32_t KNNQ_EXCLUDE_SAME_INDEX = 1u;
constexpr int KNNQ_MAX_TENSORS = 8;      // gsr_knn_gather_mean
constexpr int KNNQ_MAX_COLS = 128;       // per tensor and in total

// How a query finished: KNN_FIN_SHELL / KNN_FIN_WHOLE_GRID / KNN_FIN_FALLBACK of gsr_knn.h, and
constexpr int KNNQ_FIN_NONFINITE = 0x400;   // the query has a non-finite coordinate: no search, no neighbours
constexpr int KNNQ_FIN_OUTSIDE = 0x800;     // set by the CALLER that knows the box (the host harness): the query lies outside
                                            // the references' bounding box, so its cell was clamped

// A reference as the search reads it: the cell-sorted copy, 16 bytes per candidate.
struct alignas(16) KnnqRef { float x, y, z; int32_t idx; };

template <int K>
struct KnnqBest { double d[K]; int32_t i[K]; };

GSR_HD double knnq_dist2(float ax, float ay, float az, float bx, float by, float bz) {
  GSR_FP_STRICT
  const double dx = (double)ax - (double)bx, dy = (double)ay - (double)by, dz = (double)az - (double)bz;
  return (dx * dx + dy * dy) + dz * dz;
}

GSR_HD bool knnq_before(double d2, int32_t idx, double sd, int32_t si) { return d2 < sd || (d2 == sd && idx < si); }

template <int K>
GSR_HD void knnq_clear(KnnqBest<K>& b) {
#pragma unroll
  for (int j = 0; j < K; ++j) { b.d[j] = (double)INFINITY; b.i[j] = -1; }
}

// (d2, idx) into the K sorted slots.  Every slot index is a constant after unrolling: no register array is indexed
// dynamically.  A NaN or +inf d2 precedes nothing, an empty slot (+inf, -1) included.
template <int K>
GSR_HD void knnq_insert(KnnqBest<K>& b, double d2, int32_t idx) {
  if (!knnq_before(d2, idx, b.d[K - 1], b.i[K - 1])) return;
  bool here = true;                                     // (d2, idx) precedes slot j
#pragma unroll
  for (int j = K - 1; j >= 1; --j) {
    const bool up = knnq_before(d2, idx, b.d[j - 1], b.i[j - 1]);
    b.d[j] = up ? b.d[j - 1] : (here ? d2 : b.d[j]);
    b.i[j] = up ? b.i[j - 1] : (here ? idx : b.i[j]);
    here = up;
  }
  if (here) { b.d[0] = d2; b.i[0] = idx; }
}

GSR_HD bool knnq_finite(float v) { return fabsf(v) <= FLT_MAX; }

// lower bound of the distance to anything binned beyond a face `raw` away (see the head of this file)
GSR_HD double knnq_face_gap(double raw, double extent) {
  GSR_FP_STRICT
  const double s = raw * 0.9999 - extent * (1.0 / 1048576.0);
  return s > 0.0 ? s : 0.0;
}

// The search of one query (px, py, pz) among refs[0..R), the references in cell-sorted order.  self: the reference index the
// query must not take, -1 for none.  Range: anything with .x = start, .y = end of a cell's run in refs (uint2 in the kernel).
// finish, when given, receives how the query ended; the kernel passes nothing.
template <int K, class Range>
GSR_HD void knnq_search_point(float px, float py, float pz, int32_t self, const KnnqRef* __restrict__ refs, int R,
                              const KnnGrid& g, const Range* __restrict__ cell_range, KnnqBest<K>& best,
                              int* finish = nullptr) {
  knnq_clear(best);
  if (!(knnq_finite(px) && knnq_finite(py) && knnq_finite(pz))) {
    if (finish) *finish = KNNQ_FIN_NONFINITE;
    return;
  }
  const int cx = knn_cell_coord(px, g.minx, g.inv_cx, g.dx);    // the REFERENCE grid's cell, clamped
  const int cy = knn_cell_coord(py, g.miny, g.inv_cy, g.dy);
  const int cz = knn_cell_coord(pz, g.minz, g.inv_cz, g.dz);
  const double ex = (double)g.dx * (double)g.sx, ey = (double)g.dy * (double)g.sy, ez = (double)g.dz * (double)g.sz;
  bool done = false;
  for (int r = 0; r <= KNN_MAX_SHELL && !done; ++r) {
    for (int z = cz - r; z <= cz + r; ++z) {
      if (z < 0 || z >= g.dz) continue;
      for (int y = cy - r; y <= cy + r; ++y) {
        if (y < 0 || y >= g.dy) continue;
        const bool face = (z == cz - r) || (z == cz + r) || (y == cy - r) || (y == cy + r);
        for (int x = cx - r; x <= cx + r; x += (face ? 1 : 2 * r)) {     // interior rows: only the two end cells
          if (x >= 0 && x < g.dx) {
            const Range rg = cell_range[(z * g.dy + y) * g.dx + x];
            for (uint32_t j = rg.x; j < rg.y; ++j) {
              const KnnqRef o = refs[j];
              if (o.idx == self) continue;
              knnq_insert(best, knnq_dist2(o.x, o.y, o.z, px, py, pz), o.idx);
            }
          }
          if (r == 0) break;
        }
      }
    }
    double safe = DBL_MAX;
    if (cx - r > 0) safe = fmin(safe, knnq_face_gap((double)px - ((double)g.minx + (double)(cx - r) * (double)g.sx), ex));
    if (cx + r < g.dx - 1) safe = fmin(safe, knnq_face_gap(((double)g.minx + (double)(cx + r + 1) * (double)g.sx) - (double)px, ex));
    if (cy - r > 0) safe = fmin(safe, knnq_face_gap((double)py - ((double)g.miny + (double)(cy - r) * (double)g.sy), ey));
    if (cy + r < g.dy - 1) safe = fmin(safe, knnq_face_gap(((double)g.miny + (double)(cy + r + 1) * (double)g.sy) - (double)py, ey));
    if (cz - r > 0) safe = fmin(safe, knnq_face_gap((double)pz - ((double)g.minz + (double)(cz - r) * (double)g.sz), ez));
    if (cz + r < g.dz - 1) safe = fmin(safe, knnq_face_gap(((double)g.minz + (double)(cz + r + 1) * (double)g.sz) - (double)pz, ez));
    if (safe == DBL_MAX) {
      done = true;                      // the block covers the whole grid: nothing left to scan
      if (finish) *finish = r | KNN_FIN_WHOLE_GRID;
    } else {
      done = best.d[K - 1] < safe * safe;     // strict: see the head of this file
      if (finish && done) *finish = r;
    }
  }
  if (!done) {   // isolated query: exact answer by a full sweep (any order: the slots' order is total)
    knnq_clear(best);
    for (int j = 0; j < R; ++j) {
      const KnnqRef o = refs[j];
      if (o.idx == self) continue;
      knnq_insert(best, knnq_dist2(o.x, o.y, o.z, px, py, pz), o.idx);
    }
    if (finish) *finish = KNN_MAX_SHELL | KNN_FIN_FALLBACK;
  }
}

// One element of the gather-mean: column `col` of a [R, stride] tensor over the k indices of one query.
GSR_HD float knnq_mean(const int32_t* __restrict__ idx_row, int k, int R, const float* __restrict__ src, int stride, int col) {
  GSR_FP_STRICT
  float acc = 0.f;
  int m = 0;
  for (int r = 0; r < k; ++r) {
    const int32_t id = idx_row[r];
    if (id < 0 || id >= R) continue;                    // missing, or not an index: skipped, never followed
    const float v = src[(size_t)id * (size_t)stride + (size_t)col];
    acc = m ? acc + v : v;
    ++m;
  }
  return m ? acc / (float)m : 0.f;
}

}  // namespace gsr
