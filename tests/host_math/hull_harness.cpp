// TEST HARNESS ONLY (built by tests/test_groups_hull_cpu.py with g++): the convex hull of csrc/gsr_hull.h -- the same
// header libgsraster.so's gsr_convex_hull_planes compiles -- as a small C library, and with -DHULL_MAIN as a program
// that runs the hull over a fixed set of clouds (for a build with -fsanitize=address,undefined).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "gsr_hull.h"

extern "C" {

// -> status (gsr_hull::Status); planes [max_facets, 4] (nx, ny, nz, c); out6 = bbox; info3 = (D, tau, worst)
int hh_convex_hull(const double* pts, int64_t M, double* planes, int64_t max_facets, int64_t* nfacets, double* bbox,
                   double* info3) {
  gsr_hull::Result r = gsr_hull::convex_hull(pts, M);
  *nfacets = (int64_t)r.planes.size();
  for (int a = 0; a < 6; ++a) bbox[a] = r.bbox[a];
  info3[0] = r.diag; info3[1] = r.tau; info3[2] = r.worst;
  if ((int64_t)r.planes.size() > max_facets) return -1;
  for (size_t f = 0; f < r.planes.size(); ++f) {
    planes[4 * f] = r.planes[f].nx; planes[4 * f + 1] = r.planes[f].ny;
    planes[4 * f + 2] = r.planes[f].nz; planes[4 * f + 3] = r.planes[f].c;
  }
  return r.status;
}

}  // extern "C"

#ifdef HULL_MAIN
int main() {
  std::mt19937_64 rng(12345);
  std::normal_distribution<double> nd(0.0, 1.0);
  std::uniform_real_distribution<double> ud(-1.0, 1.0);
  int bad = 0;
  const int64_t sizes[] = {4, 5, 10, 100, 1000, 20000};
  for (int64_t M : sizes)
    for (int kind = 0; kind < 3; ++kind) {
      std::vector<double> p((size_t)(3 * M));
      for (int64_t i = 0; i < M; ++i) {
        for (int a = 0; a < 3; ++a) p[3 * i + a] = kind == 0 ? nd(rng) : ud(rng);
        if (kind == 2) p[3 * i + (i % 3)] = (i & 1) ? 1.0 : -1.0;      // on the surface of a cube
        if (kind == 2 && i % 7 == 0 && i > 0) for (int a = 0; a < 3; ++a) p[3 * i + a] = p[3 * (i - 1) + a];   // duplicates
      }
      gsr_hull::Result r = gsr_hull::convex_hull(p.data(), M);
      const bool ok = r.status == gsr_hull::HULL_OK || (M < 8 && r.status == gsr_hull::HULL_DEGENERATE);
      std::printf("M=%lld kind=%d status=%d facets=%zu worst/tau=%.3g\n", (long long)M, kind, r.status, r.planes.size(),
                  r.tau > 0 ? r.worst / r.tau : 0.0);
      if (!ok) ++bad;
    }
  // degenerate inputs: coplanar, collinear, three points, one point repeated
  std::vector<double> flat;
  for (int i = 0; i < 50; ++i) { flat.push_back(ud(rng)); flat.push_back(ud(rng)); flat.push_back(0.25); }
  if (gsr_hull::convex_hull(flat.data(), 50).status != gsr_hull::HULL_DEGENERATE) ++bad;
  std::vector<double> line;
  for (int i = 0; i < 50; ++i) { const double t = ud(rng); line.push_back(t); line.push_back(2 * t); line.push_back(-t); }
  if (gsr_hull::convex_hull(line.data(), 50).status != gsr_hull::HULL_DEGENERATE) ++bad;
  if (gsr_hull::convex_hull(flat.data(), 3).status != gsr_hull::HULL_DEGENERATE) ++bad;
  std::vector<double> same(3 * 40, 0.5);
  if (gsr_hull::convex_hull(same.data(), 40).status != gsr_hull::HULL_DEGENERATE) ++bad;
  std::printf("%s\n", bad ? "FAIL" : "OK");
  return bad ? 1 : 0;
}
#endif
