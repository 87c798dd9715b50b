// gsr_knn.h -- the scalar side of the exact 3-nearest-neighbour routine (gsr_knn_dist2, include/gsraster.h): the grid
// set-up, the cell of a point, the three-best update and the search of one point.
//
// One source, compiled twice: by hipcc into the kernels of gsr_knn.hip.h and the set-up in gsr_api.hip, and by g++ into
// a host harness (tests/host_math/knn_host.cpp) that runs the whole pipeline on the CPU and reports how every point
// finished.  Nothing here is marked GSR_FP_STRICT: the kernel may contract a*a + b*b + c*c into FMAs, the host build
// (-ffp-contract=off) does not, and the tests allow for that (tests/knn_cases.py).
//
// The contract (include/gsraster.h):
//   * out[i] = (d0 + d1 + d2) / 3 in float32, d0 <= d1 <= d2 the three smallest squared distances from point i to the
//     OTHER points (by index, so a coincident point counts with distance 0).
//   * With fewer than 4 points the missing neighbours count as FLT_MAX: +inf for P <= 2 (FLT_MAX + FLT_MAX overflows),
//     and for P = 3 whatever float32 gives for (d0 + d1 + FLT_MAX) / 3.
//   * Non-finite points.  A squared distance that is NaN or +inf is never taken as a neighbour (it is not < FLT_MAX).
//     So a point with a NaN or an infinite coordinate gets +inf itself and is invisible to every other point, whose
//     result is the one over the finite points.  A NaN coordinate does not enter the bounding box (fminf / fmaxf drop
//     it) and its cell coordinate clamps to 0; the point passes no "safe distance" test, so it ends in the sweep or
//     when its block covers the grid.  An infinite coordinate makes every extent infinite (the floor is 1e-6 of the
//     largest), so the grid is ONE cell.
//
// Known limit, not measured: the grid is uniform over the bounding box.  One far point -- a COLMAP sky point at 1000x
// the scene's extent puts the whole scene into at most 8 cells -- or one infinite coordinate (one cell) collapses it,
// and the search becomes quadratic in the points that share a cell.  Results stay exact; nobody has measured the run
// time of such a cloud.  Changing the grid policy is a change of its own.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "gsr_math.h"   // GSR_HD

namespace gsr {

struct KnnGrid {
  float minx, miny, minz;
  float inv_cx, inv_cy, inv_cz;   // 1 / cell size per axis
  float sx, sy, sz;               // cell size per axis
  int dx, dy, dz;                 // cells per axis
};

constexpr int KNN_MAX_SHELL = 10;
constexpr int KNN_MAX_DIM = 256;

// How a point finished (knn_search_point's optional out-parameter): the shell index at which it stopped in the low
// byte, plus one of the two flags.  Neither flag: the "safe distance" test passed at that shell.
constexpr int KNN_FIN_SHELL = 0xff;
constexpr int KNN_FIN_WHOLE_GRID = 0x100;   // the scanned block covered the whole grid
constexpr int KNN_FIN_FALLBACK = 0x200;     // not finished after KNN_MAX_SHELL shells: the full sweep

// Host side.  bb[0..2] = min, bb[3..5] = max of the points: about three points per cell, at most KNN_MAX_DIM cells per
// axis, every extent at least 1e-6 of the largest (1 when all points coincide).
inline KnnGrid knn_make_grid(const float bb[6], int P) {
  double ext[3], vol = 1.0, emax = 0.0;
  for (int a = 0; a < 3; ++a) { ext[a] = (double)bb[3 + a] - (double)bb[a]; emax = std::max(emax, ext[a]); }
  if (!(emax > 0.0)) emax = 1.0;                       // all points coincide
  for (int a = 0; a < 3; ++a) { ext[a] = std::max(ext[a], 1e-6 * emax); vol *= ext[a]; }
  const double cell = std::cbrt(vol * 3.0 / (double)P);
  KnnGrid g;
  int dims[3];
  float inv[3], size[3];
  for (int a = 0; a < 3; ++a) {
    dims[a] = (int)std::min((double)KNN_MAX_DIM, std::max(1.0, std::ceil(ext[a] / cell)));
    const double c = ext[a] / dims[a];
    inv[a] = (float)(1.0 / c);
    size[a] = (float)c;
  }
  g.minx = bb[0]; g.miny = bb[1]; g.minz = bb[2];
  g.inv_cx = inv[0]; g.inv_cy = inv[1]; g.inv_cz = inv[2];
  g.sx = size[0]; g.sy = size[1]; g.sz = size[2]; g.dx = dims[0]; g.dy = dims[1]; g.dz = dims[2];
  return g;
}

GSR_HD int knn_cell_coord(float v, float mn, float inv, int d) {
  const int c = (int)((v - mn) * inv);
  return c < 0 ? 0 : (c >= d ? d - 1 : c);
}

GSR_HD uint32_t knn_cell_key(const float* __restrict__ pts, int i, const KnnGrid& g) {
  const int cx = knn_cell_coord(pts[3 * i], g.minx, g.inv_cx, g.dx);
  const int cy = knn_cell_coord(pts[3 * i + 1], g.miny, g.inv_cy, g.dy);
  const int cz = knn_cell_coord(pts[3 * i + 2], g.minz, g.inv_cz, g.dz);
  return (uint32_t)((cz * g.dy + cy) * g.dx + cx);
}

GSR_HD void knn_update(float d2, float best[3]) {
  if (d2 < best[2]) {
    if (d2 < best[1]) {
      best[2] = best[1];
      if (d2 < best[0]) { best[1] = best[0]; best[0] = d2; } else best[1] = d2;
    } else best[2] = d2;
  }
}

// The search of the point at position s of the cell-sorted order.  Range: anything with .x = start, .y = end of a cell's
// run in sorted_idx (uint2 in the kernel).  Writes out[sorted_idx[s]].  finish, when given, receives how the point ended
// (KNN_FIN_*); the kernel passes nothing.
template <class Range>
GSR_HD void knn_search_point(int s, const float* __restrict__ pts, int P, const KnnGrid& g,
                             const uint32_t* __restrict__ sorted_idx, const Range* __restrict__ cell_range,
                             float* __restrict__ out, int* finish = nullptr) {
  const uint32_t me = sorted_idx[s];
  const float px = pts[3 * me], py = pts[3 * me + 1], pz = pts[3 * me + 2];
  const int cx = knn_cell_coord(px, g.minx, g.inv_cx, g.dx);
  const int cy = knn_cell_coord(py, g.miny, g.inv_cy, g.dy);
  const int cz = knn_cell_coord(pz, g.minz, g.inv_cz, g.dz);
  float best[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
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
              const uint32_t o = sorted_idx[j];
              if (o == me) continue;
              const float ddx = pts[3 * o] - px, ddy = pts[3 * o + 1] - py, ddz = pts[3 * o + 2] - pz;
              knn_update(ddx * ddx + ddy * ddy + ddz * ddz, best);
            }
          }
          if (r == 0) break;
        }
      }
    }
    // distance from the point to the nearest face of the scanned (2r+1)^3 block that is not a face of the grid:
    // every point binned outside the block is at least that far away (shaved for the rounding of the binning)
    float safe = FLT_MAX;
    if (cx - r > 0) safe = fminf(safe, px - (g.minx + (float)(cx - r) * g.sx));
    if (cx + r < g.dx - 1) safe = fminf(safe, (g.minx + (float)(cx + r + 1) * g.sx) - px);
    if (cy - r > 0) safe = fminf(safe, py - (g.miny + (float)(cy - r) * g.sy));
    if (cy + r < g.dy - 1) safe = fminf(safe, (g.miny + (float)(cy + r + 1) * g.sy) - py);
    if (cz - r > 0) safe = fminf(safe, pz - (g.minz + (float)(cz - r) * g.sz));
    if (cz + r < g.dz - 1) safe = fminf(safe, (g.minz + (float)(cz + r + 1) * g.sz) - pz);
    if (safe == FLT_MAX) {
      done = true;                      // the block covers the whole grid: nothing left to scan
      if (finish) *finish = r | KNN_FIN_WHOLE_GRID;
    } else {
      safe = fmaxf(0.f, safe * 0.9999f);
      done = best[2] <= safe * safe;
      if (finish && done) *finish = r;
    }
  }
  if (!done) {   // isolated point: exact answer by a full sweep
    best[0] = best[1] = best[2] = FLT_MAX;
    for (int o = 0; o < P; ++o) {
      if ((uint32_t)o == me) continue;
      const float ddx = pts[3 * o] - px, ddy = pts[3 * o + 1] - py, ddz = pts[3 * o + 2] - pz;
      knn_update(ddx * ddx + ddy * ddy + ddz * ddz, best);
    }
    if (finish) *finish = KNN_MAX_SHELL | KNN_FIN_FALLBACK;
  }
  out[me] = (best[0] + best[1] + best[2]) / 3.0f;
}

}  // namespace gsr
