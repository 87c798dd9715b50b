// gsr_hull.h -- 3-D convex hull of a point set as outward facet planes: quickhull in double, host only, plain C++17.
//
// The groups set-up (gsplat_attack/groups.py) selects every Gaussian inside the convex hull of a classified object's
// positions.  The reference builds that hull with scipy's Delaunay (Qhull) over the filtered points and tests all P
// positions with find_simplex on the host (scratch/edit_object_removal.py:59-63).  Here the hull is built once on the
// host as a list of planes (n, c) -- unit outward normal, offset -- and the inclusion test runs on the device
// (k_points_in_hull, gsr_groups.hip.h): a point x is inside iff  n_f . x - c_f <= tau  for every facet f.
//
// Semantics (groups mode):
//   - tau = 1e-9 * D, D the diagonal of the input points' bounding box;
//   - fewer than 4 points, or points that all lie within tau of a point, a line or a plane: DEGENERATE, 0 facets
//     (Qhull raises there);
//   - before it returns, every input point is checked against every plane within tau; a failure returns
//     HULL_CHECK_FAILED and no planes.
// Kept free of HIP so that a g++ build tests it on the host (tests/host_math/hull_harness.cpp).
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

namespace gsr_hull {

struct Plane {
  double nx, ny, nz, c;    // unit outward normal, offset: the point x is on the inner side iff n . x - c <= tau
};

enum Status { HULL_OK = 0, HULL_DEGENERATE = 1, HULL_CHECK_FAILED = 2, HULL_INTERNAL = 3 };

// The one evaluation order every consumer uses (the device kernel too): ((nx*x + ny*y) + nz*z) - c, every operation
// rounded on its own (no fused multiply-add), so that host and device verdicts agree bit for bit.
inline double plane_dist(const Plane& p, double x, double y, double z) {
  double s = p.nx * x;
  s = s + p.ny * y;
  s = s + p.nz * z;
  return s - p.c;
}

struct Result {
  int status = HULL_INTERNAL;
  std::vector<Plane> planes;
  double bbox[6] = {0, 0, 0, 0, 0, 0};   // min xyz, max xyz of the input points
  double diag = 0.0;                     // D
  double tau = 0.0;                      // 1e-9 * D
  double worst = 0.0;                    // max over points and planes of plane_dist (the self-check's measure)
};

namespace detail {

struct Face {
  int v[3];
  int nb[3];                  // neighbour across the edge (v[i], v[(i + 1) % 3])
  Plane pl;
  std::vector<int> outside;   // points strictly outside this face, not yet on the hull
  int far = -1;
  double far_d = 0.0;
  bool alive = true;
};

struct Builder {
  const double* p;
  int64_t M;
  double eps;
  std::vector<Face> faces;

  const double* pt(int i) const { return p + 3 * (int64_t)i; }
  double dist(const Face& f, int i) const { const double* q = pt(i); return plane_dist(f.pl, q[0], q[1], q[2]); }

  // plane through a, b, c with the normal (b - a) x (c - a); false if the triangle has no area
  bool plane_of(int a, int b, int c, Plane& out) const {
    const double *A = pt(a), *B = pt(b), *C = pt(c);
    const double ux = B[0] - A[0], uy = B[1] - A[1], uz = B[2] - A[2];
    const double vx = C[0] - A[0], vy = C[1] - A[1], vz = C[2] - A[2];
    double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double len = std::sqrt(nx * nx + ny * ny + nz * nz);
    if (!(len > 0.0) || !std::isfinite(len)) return false;
    nx /= len; ny /= len; nz /= len;
    out.nx = nx; out.ny = ny; out.nz = nz; out.c = 0.0;
    // the offset as the mean over the three vertices: the plane passes as close to all of them as rounding allows
    out.c = (plane_dist(out, A[0], A[1], A[2]) + plane_dist(out, B[0], B[1], B[2]) + plane_dist(out, C[0], C[1], C[2])) / 3.0;
    return true;
  }

  int add_face(int a, int b, int c) {
    Face f;
    f.v[0] = a; f.v[1] = b; f.v[2] = c;
    f.nb[0] = f.nb[1] = f.nb[2] = -1;
    if (!plane_of(a, b, c, f.pl)) return -1;
    faces.push_back(std::move(f));
    return (int)faces.size() - 1;
  }

  void assign(int i, const int* cand, int n) {
    for (int k = 0; k < n; ++k) {
      Face& f = faces[cand[k]];
      const double d = dist(f, i);
      if (d > eps) {
        f.outside.push_back(i);
        if (d > f.far_d) { f.far_d = d; f.far = i; }
        return;
      }
    }
  }
};

inline int edge_index(const Face& f, int a, int b) {
  for (int i = 0; i < 3; ++i)
    if (f.v[i] == a && f.v[(i + 1) % 3] == b) return i;
  return -1;
}

}  // namespace detail

// pts: M points, xyz interleaved (double).  The result's planes are the hull's facets (triangles; coplanar facets are
// not merged).
inline Result convex_hull(const double* pts, int64_t M) {
  using namespace detail;
  Result r;
  if (M <= 0 || !pts) { r.status = HULL_DEGENERATE; return r; }
  if (M > (int64_t)0x3fffffff) { r.status = HULL_INTERNAL; return r; }
  double rmax = 0.0;
  for (int a = 0; a < 3; ++a) { r.bbox[a] = DBL_MAX; r.bbox[3 + a] = -DBL_MAX; }
  int ext[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t i = 0; i < M; ++i)
    for (int a = 0; a < 3; ++a) {
      const double v = pts[3 * i + a];
      if (!std::isfinite(v)) { r.status = HULL_INTERNAL; return r; }
      if (v < r.bbox[a]) { r.bbox[a] = v; ext[a] = (int)i; }
      if (v > r.bbox[3 + a]) { r.bbox[3 + a] = v; ext[3 + a] = (int)i; }
      rmax = std::max(rmax, std::fabs(v));
    }
  const double dx = r.bbox[3] - r.bbox[0], dy = r.bbox[4] - r.bbox[1], dz = r.bbox[5] - r.bbox[2];
  r.diag = std::sqrt(dx * dx + dy * dy + dz * dz);
  r.tau = 1e-9 * r.diag;
  if (M < 4 || !(r.diag > 0.0)) { r.status = HULL_DEGENERATE; return r; }
  const double tau = r.tau;

  Builder B;
  B.p = pts;
  B.M = M;
  // "strictly outside" during the construction: far above rounding noise of a plane evaluation at these coordinates, far
  // below tau
  B.eps = std::max(1e-12 * r.diag, 64.0 * DBL_EPSILON * rmax);
  if (!(B.eps < 0.1 * tau)) { r.status = HULL_INTERNAL; return r; }   // coordinates too far from the origin for the size

  // ---- initial simplex ------------------------------------------------------------------------------------------
  auto d2 = [&](int i, int j) {
    const double *a = B.pt(i), *b = B.pt(j);
    const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
    return x * x + y * y + z * z;
  };
  int i0 = ext[0], i1 = ext[3];
  double best = -1.0;
  for (int a = 0; a < 6; ++a)
    for (int b = a + 1; b < 6; ++b)
      if (d2(ext[a], ext[b]) > best) { best = d2(ext[a], ext[b]); i0 = ext[a]; i1 = ext[b]; }
  if (!(std::sqrt(best) > tau)) { r.status = HULL_DEGENERATE; return r; }
  const double* P0 = B.pt(i0);
  const double* P1 = B.pt(i1);
  double ux = P1[0] - P0[0], uy = P1[1] - P0[1], uz = P1[2] - P0[2];
  {
    const double l = std::sqrt(ux * ux + uy * uy + uz * uz);
    ux /= l; uy /= l; uz /= l;
  }
  int i2 = -1;
  best = -1.0;
  for (int64_t i = 0; i < M; ++i) {
    const double* q = B.pt((int)i);
    const double x = q[0] - P0[0], y = q[1] - P0[1], z = q[2] - P0[2];
    const double cx = y * uz - z * uy, cy = z * ux - x * uz, cz = x * uy - y * ux;
    const double d = cx * cx + cy * cy + cz * cz;
    if (d > best) { best = d; i2 = (int)i; }
  }
  if (!(std::sqrt(best) > tau)) { r.status = HULL_DEGENERATE; return r; }
  Plane base;
  if (!B.plane_of(i0, i1, i2, base)) { r.status = HULL_DEGENERATE; return r; }
  int i3 = -1;
  best = -1.0;
  for (int64_t i = 0; i < M; ++i) {
    const double* q = B.pt((int)i);
    const double d = std::fabs(plane_dist(base, q[0], q[1], q[2]));
    if (d > best) { best = d; i3 = (int)i; }
  }
  if (!(best > tau)) { r.status = HULL_DEGENERATE; return r; }
  {
    const double* q = B.pt(i3);
    if (plane_dist(base, q[0], q[1], q[2]) > 0.0) std::swap(i1, i2);   // the apex below the base's plane
  }
  // base (a, b, c) facing away from the apex d; side faces (b, a, d), (c, b, d), (a, c, d)
  const int tet[4][3] = {{i0, i1, i2}, {i1, i0, i3}, {i2, i1, i3}, {i0, i2, i3}};
  for (int f = 0; f < 4; ++f)
    if (B.add_face(tet[f][0], tet[f][1], tet[f][2]) != f) { r.status = HULL_DEGENERATE; return r; }
  for (int f = 0; f < 4; ++f)
    for (int e = 0; e < 3; ++e) {
      const int a = B.faces[f].v[e], b = B.faces[f].v[(e + 1) % 3];
      for (int g = 0; g < 4; ++g)
        if (g != f && edge_index(B.faces[g], b, a) >= 0) B.faces[f].nb[e] = g;
      if (B.faces[f].nb[e] < 0) { r.status = HULL_INTERNAL; return r; }
    }
  const int tv[4] = {i0, i1, i2, i3};
  for (int f = 0; f < 4; ++f)                      // each face has the opposite vertex on its inner side
    for (int k = 0; k < 4; ++k)
      if (B.dist(B.faces[f], tv[k]) > B.eps) { r.status = HULL_INTERNAL; return r; }
  {
    const int cand[4] = {0, 1, 2, 3};
    for (int64_t i = 0; i < M; ++i)
      if ((int)i != i0 && (int)i != i1 && (int)i != i2 && (int)i != i3) B.assign((int)i, cand, 4);
  }

  // ---- expansion ------------------------------------------------------------------------------------------------
  std::vector<int> todo = {0, 1, 2, 3};
  std::vector<int> stamp_vis, stamp_seen, start_of((size_t)M, -1), start_stamp((size_t)M, -1);
  std::vector<int> visible, queue, newf, pool;
  struct Hz { int a, b, outer, outer_e; };
  std::vector<Hz> horizon;
  int iter = 0;
  while (!todo.empty()) {
    const int f0 = todo.back();
    todo.pop_back();
    if (!B.faces[f0].alive || B.faces[f0].outside.empty()) continue;
    ++iter;
    const int eye = B.faces[f0].far;
    stamp_vis.resize(B.faces.size(), 0);
    stamp_seen.resize(B.faces.size(), 0);
    // visible faces: the connected region around f0 that has the eye point strictly outside
    visible.clear(); horizon.clear(); queue.clear();
    queue.push_back(f0);
    stamp_vis[f0] = iter; stamp_seen[f0] = iter;
    for (size_t qi = 0; qi < queue.size(); ++qi) {
      const int g = queue[qi];
      visible.push_back(g);
      for (int e = 0; e < 3; ++e) {
        const int h = B.faces[g].nb[e];
        if (stamp_seen[h] != iter) {
          stamp_seen[h] = iter;
          if (B.dist(B.faces[h], eye) > B.eps) { stamp_vis[h] = iter; queue.push_back(h); }
        }
        if (stamp_vis[h] != iter) {
          const int a = B.faces[g].v[e], b = B.faces[g].v[(e + 1) % 3];
          const int oe = edge_index(B.faces[h], b, a);
          if (oe < 0) { r.status = HULL_INTERNAL; return r; }
          horizon.push_back({a, b, h, oe});
        }
      }
    }
    // the horizon must be one closed loop of edges: every vertex starts exactly one edge
    if (horizon.size() < 3) { r.status = HULL_INTERNAL; return r; }
    for (size_t k = 0; k < horizon.size(); ++k) {
      const int a = horizon[k].a;
      if (start_stamp[a] == iter) { r.status = HULL_INTERNAL; return r; }
      start_stamp[a] = iter;
      start_of[a] = (int)k;
    }
    newf.clear();
    for (const Hz& hz : horizon) {
      const int nf = B.add_face(hz.a, hz.b, eye);
      if (nf < 0) { r.status = HULL_INTERNAL; return r; }
      B.faces[nf].nb[0] = hz.outer;
      B.faces[hz.outer].nb[hz.outer_e] = nf;
      newf.push_back(nf);
    }
    for (size_t k = 0; k < horizon.size(); ++k) {
      const int b = horizon[k].b;
      if (start_stamp[b] != iter) { r.status = HULL_INTERNAL; return r; }
      const int m = newf[(size_t)start_of[b]];
      B.faces[newf[k]].nb[1] = m;       // across (b, eye)
      B.faces[m].nb[2] = newf[k];       // across (eye, b)
    }
    // the visible faces go; their outside points move to the new faces or are inside now
    pool.clear();
    for (int g : visible) {
      Face& F = B.faces[g];
      F.alive = false;
      pool.insert(pool.end(), F.outside.begin(), F.outside.end());
      std::vector<int>().swap(F.outside);
    }
    for (int i : pool)
      if (i != eye) B.assign(i, newf.data(), (int)newf.size());
    for (int nf : newf)
      if (!B.faces[nf].outside.empty()) todo.push_back(nf);
  }

  for (const Face& F : B.faces)
    if (F.alive) r.planes.push_back(F.pl);

  // ---- self-check: every input point on the inner side of every plane within tau ---------------------------------
  // A point strictly inside the initial simplex is a convex combination of its four vertices, which are input points
  // themselves: an affine plane_dist is at most the largest of theirs there, so such points need no test of their own.
  const Face* T = B.faces.data();
  const std::vector<Plane>& pl = r.planes;
  unsigned nth = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (M < 65536) nth = 1;
  std::vector<double> worst(nth, -DBL_MAX);
  auto check = [&](unsigned t) {
    const int64_t lo = M * (int64_t)t / nth, hi = M * (int64_t)(t + 1) / nth;
    double w = -DBL_MAX;
    for (int64_t i = lo; i < hi; ++i) {
      const double* q = pts + 3 * i;
      bool inner = true;
      for (int f = 0; f < 4 && inner; ++f) inner = plane_dist(T[f].pl, q[0], q[1], q[2]) < -B.eps;
      if (inner && i != i0 && i != i1 && i != i2 && i != i3) continue;
      for (const Plane& P : pl) w = std::max(w, plane_dist(P, q[0], q[1], q[2]));
    }
    worst[t] = w;
  };
  if (nth == 1) check(0);
  else {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nth; ++t) th.emplace_back(check, t);
    for (std::thread& x : th) x.join();
  }
  r.worst = *std::max_element(worst.begin(), worst.end());
  if (pl.size() < 4 || !(r.worst <= tau)) {
    r.planes.clear();
    r.status = HULL_CHECK_FAILED;
    return r;
  }
  r.status = HULL_OK;
  return r;
}

}  // namespace gsr_hull
