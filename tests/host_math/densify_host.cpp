// Adaptive density control on the CPU, from csrc/gsr_densify.h -- the scalar source the HIP kernels compile -- in plain loops.
//   dh_stats        gsr_densify_stats' arguments without the stream
//   dh_plan         gsr_densify_plan without workspace and stream: code [P] and the three exclusive offsets [P + 1] go to the caller
//   dh_apply        gsr_densify_apply over those arrays; the same refusals (return 1), the same result
//   dh_thresholds, dh_normal, dh_uniform, dh_rotation, dh_span   the scalars, for the tests
// Build: g++ -O1 -ffp-contract=off -shared -fPIC -I <csrc> densify_host.cpp -o libdensifyhost.so
// With -DDENSIFY_MAIN: a program that reads calls from a file (int32 count; per call int64 P; int32 N, flags, n, has_normals,
// has_mask, seed; float64 max_grad, min_opacity, extent, percent_dense, max_screen; accum, denom, max_radii [P]; scaling [P,3];
// opacity [P]; rotation [P,4]; normals [P,N,3] if any; mask [P] if any; per tensor int32 cols, role, has_state, then src and,
// with state, m and v of P * cols floats), runs each with buffers exactly as large as the shapes say, and prints one line per
// call -- for a build with -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gsr_densify.h"

using namespace gsr;

extern "C" int dh_stats(const float* grad, const int32_t* radii, const uint8_t* filter, int32_t B, int64_t P, float* accum, float* denom,
                        float* max_radii) {
  if (B < 0 || P < 0 || P > DENS_MAX_ROWS) return 1;
  if (B == 0 || P == 0) return 0;
  if (!grad || !accum || !denom || (!radii && !filter) || (max_radii && !radii)) return 1;
  for (int64_t i = 0; i < P; ++i)
    for (int b = 0; b < B; ++b) {
      const size_t k = (size_t)b * (size_t)P + (size_t)i;
      const bool on = filter ? filter[k] != 0 : radii[k] > 0;
      if (!on) continue;
      dens_stat_update(accum[i], denom[i], grad[3 * k], grad[3 * k + 1]);
      if (radii && max_radii) max_radii[i] = dens_max_radius(max_radii[i], radii[k]);
    }
  return 0;
}

extern "C" int dh_thresholds(double max_grad, double min_opacity, double extent, double percent_dense, double max_screen, int32_t N,
                             uint32_t flags, float* out6) {
  DensParams p;
  const int rc = dens_thresholds(max_grad, min_opacity, extent, percent_dense, max_screen, N, flags, &p);
  if (rc == 0 && out6) { out6[0] = p.max_grad; out6[1] = p.t_dense; out6[2] = p.t_world; out6[3] = p.t_opac; out6[4] = p.c; out6[5] = p.max_screen; }
  return rc;
}

// -> 0, or 1 for a refusal; code [P], off_* [P + 1] (off[P] = the total), counts [3]
extern "C" int dh_plan(const float* accum, const float* denom, const float* scaling, const float* opacity, const float* max_radii, int64_t P,
                       double max_grad, double min_opacity, double extent, double percent_dense, double max_screen, int32_t N, uint32_t flags,
                       uint8_t* code, uint32_t* off_keep, uint32_t* off_clone, uint32_t* off_split, int64_t* counts) {
  if (P < 0 || P > DENS_MAX_ROWS || !counts) return 1;
  if (flags & ~(DENS_WORLD_PRUNE | DENS_SCREEN_PRUNE)) return 1;
  DensParams p;
  if (dens_thresholds(max_grad, min_opacity, extent, percent_dense, max_screen, N, flags, &p)) return 1;
  counts[0] = counts[1] = counts[2] = 0;
  if (P == 0) return 0;
  if (!accum || !denom || !scaling || !opacity || !code || !off_keep || !off_clone || !off_split) return 1;
  if ((flags & DENS_SCREEN_PRUNE) && !max_radii) return 1;
  uint32_t k = 0, c = 0, s = 0;
  for (int64_t i = 0; i < P; ++i) {
    const float g = dens_mean_grad(accum[i], denom[i]);
    const float smax = dens_max3(scaling[3 * i], scaling[3 * i + 1], scaling[3 * i + 2]);
    const int cd = dens_classify(g, smax, opacity[i], (flags & DENS_SCREEN_PRUNE) ? max_radii[i] : 0.f, p);
    code[i] = (uint8_t)cd;
    off_keep[i] = k; off_clone[i] = c; off_split[i] = s;
    k += (cd & DENS_KEEP) ? 1u : 0u; c += (cd & DENS_CLONE) ? 1u : 0u; s += (cd & DENS_KIDS) ? 1u : 0u;
  }
  off_keep[P] = k; off_clone[P] = c; off_split[P] = s;
  counts[0] = k; counts[1] = c; counts[2] = s;
  return 0;
}

static bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && na && nb && a0 < b0 + nb && b0 < a0 + na;
}

extern "C" int dh_apply(const uint8_t* code, const uint32_t* off_keep, const uint32_t* off_clone, const uint32_t* off_split, int64_t P,
                        const int64_t* counts, int32_t n, const float* const* src, float* const* dst, const float* const* m_src,
                        const float* const* v_src, float* const* m_dst, float* const* v_dst, const int32_t* cols, const int32_t* roles,
                        const float* rotation, int32_t N, uint32_t seed, const float* normals, const uint8_t* mask_in, uint8_t* mask_out,
                        int32_t* origin, int32_t* kind) {
  if (N < 1 || N > DENS_MAX_N || n < 0 || n > DENS_MAX_TENSORS || P < 0 || P > DENS_MAX_ROWS) return 1;
  if (!counts || (n > 0 && (!src || !dst || !cols || !roles))) return 1;
  if ((m_src || v_src || m_dst || v_dst) && !(m_src && v_src && m_dst && v_dst)) return 1;
  if ((origin != nullptr) != (kind != nullptr) || (mask_in && !mask_out)) return 1;
  for (int k = 0; k < 3; ++k) if (counts[k] < 0 || counts[k] > P) return 1;
  const long long Pn = (long long)counts[0] + counts[1] + (long long)N * counts[2];
  if (Pn > DENS_MAX_ROWS) return 1;
  int t_xyz = -1, t_scale = -1;
  for (int t = 0; t < n; ++t) {
    if (cols[t] < 1 || cols[t] > DENS_MAX_COLS || roles[t] < 0 || roles[t] > 2) return 1;
    if (roles[t] != DENS_COPY && cols[t] != 3) return 1;
    if (roles[t] == DENS_XYZ) { if (t_xyz >= 0) return 1; t_xyz = t; }
    if (roles[t] == DENS_SCALE) { if (t_scale >= 0) return 1; t_scale = t; }
    if ((P > 0 && !src[t]) || (Pn > 0 && !dst[t])) return 1;
  }
  if (counts[2] > 0 && t_xyz >= 0 && (t_scale < 0 || !rotation)) return 1;
  for (int s = 0; s < n; ++s)
    for (int d = 0; d < n; ++d) {
      const void* ss[3] = {src[s], m_src ? m_src[s] : nullptr, v_src ? v_src[s] : nullptr};
      const void* dd[3] = {dst[d], m_dst ? m_dst[d] : nullptr, v_dst ? v_dst[d] : nullptr};
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
          if (overlap(ss[i], (size_t)P * cols[s] * 4, dd[j], (size_t)Pn * cols[d] * 4)) return 1;
    }
  if (Pn == 0 || P == 0) return 0;
  if (!code || !off_keep || !off_clone || !off_split) return 1;
  const unsigned nk = (unsigned)counts[0], nc = (unsigned)counts[1], ns = (unsigned)counts[2];
  const float c = (float)log(0.8 * (double)N);
  for (int64_t r = 0; r < P; ++r) {
    const int cd = code[r];
    if (cd == 0) continue;
    for (int what = 0; what < 2 + N; ++what) {     // keep, clone, child 0 .. N - 1
      unsigned d;
      int kd;
      if (what == 0) { if (!(cd & DENS_KEEP)) continue; d = dens_row_keep(off_keep[r]); kd = DENS_KIND_KEEP; }
      else if (what == 1) { if (!(cd & DENS_CLONE)) continue; d = dens_row_clone(off_clone[r], nk); kd = DENS_KIND_CLONE; }
      else { if (!(cd & DENS_KIDS)) continue; d = dens_row_child(off_split[r], what - 2, nk, nc, ns); kd = DENS_KIND_CHILD + what - 2; }
      if (mask_out) mask_out[d] = what == 0 ? (uint8_t)(mask_in ? mask_in[r] != 0 : 1) : (uint8_t)1;
      if (origin) { origin[d] = (int32_t)r; kind[d] = kd; }
      for (int t = 0; t < n; ++t) {
        const bool state = m_src && m_src[t];
        for (int col = 0; col < cols[t]; ++col) {
          const size_t se = (size_t)r * cols[t] + col, de = (size_t)d * cols[t] + col;
          float val = src[t][se];
          if (what >= 2 && roles[t] == DENS_SCALE) val = dens_child_scale(val, c);
          if (what >= 2 && roles[t] == DENS_XYZ) {
            const int j = what - 2;
            float z[3];
            for (int a = 0; a < 3; ++a) z[a] = normals ? normals[((size_t)r * N + j) * 3 + a] : dens_normal(seed, (uint32_t)r, j, a);
            val = dens_child_axis(val, rotation + 4 * r, src[t_scale] + 3 * r, z, col);
          }
          dst[t][de] = val;
          if (state) { m_dst[t][de] = what == 0 ? m_src[t][se] : 0.f; v_dst[t][de] = what == 0 ? v_src[t][se] : 0.f; }
        }
      }
    }
  }
  return 0;
}

extern "C" float dh_normal(uint32_t seed, uint32_t row, int32_t child, int32_t axis) { return dens_normal(seed, row, child, axis); }
extern "C" void dh_normals(uint32_t seed, uint32_t row0, int64_t rows, int32_t N, float* out) {
  for (int64_t r = 0; r < rows; ++r)
    for (int j = 0; j < N; ++j)
      for (int a = 0; a < 3; ++a) out[((size_t)r * N + j) * 3 + a] = dens_normal(seed, row0 + (uint32_t)r, j, a);
}
extern "C" float dh_uniform(uint32_t seed, uint32_t row, int32_t child, int32_t pair, int32_t which) { return dens_uniform(seed, row, child, pair, which); }
extern "C" void dh_rotation(const float* q, float* R) { dens_build_rotation(q, R); }
extern "C" int32_t dh_span() { return DENS_SPAN; }

#ifdef DENSIFY_MAIN
static uint32_t fnv(uint32_t h, const void* p, size_t bytes) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < bytes; ++i) { h ^= b[i]; h *= 16777619u; }
  return h;
}
template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t ncalls = 0;
  if (fread(&ncalls, 4, 1, f) != 1) return 2;
  for (int32_t k = 0; k < ncalls; ++k) {
    int64_t P;
    int32_t hd[6];
    double par[5];
    if (fread(&P, 8, 1, f) != 1 || fread(hd, 4, 6, f) != 6 || fread(par, 8, 5, f) != 5) return 2;
    const int N = hd[0], n = hd[2];
    const uint32_t flags = (uint32_t)hd[1], seed = (uint32_t)hd[5];
    if (P < 0 || N < 1 || N > DENS_MAX_N || n < 0 || n > DENS_MAX_TENSORS) return 2;
    const size_t p = (size_t)P;
    std::vector<float> accum, denom, radii, scaling, opacity, rotation, normals;
    std::vector<uint8_t> mask;
    if (!rd(f, accum, p) || !rd(f, denom, p) || !rd(f, radii, p) || !rd(f, scaling, 3 * p) || !rd(f, opacity, p) || !rd(f, rotation, 4 * p)) return 2;
    if (hd[3] && !rd(f, normals, p * N * 3)) return 2;
    if (hd[4] && !rd(f, mask, p)) return 2;
    std::vector<std::vector<float>> s(n), m(n), v(n), ds(n), dm(n), dv(n);
    int32_t cols[DENS_MAX_TENSORS], roles[DENS_MAX_TENSORS], state[DENS_MAX_TENSORS];
    for (int t = 0; t < n; ++t) {
      int32_t h3[3];
      if (fread(h3, 4, 3, f) != 3 || h3[0] < 1 || h3[0] > DENS_MAX_COLS) return 2;
      cols[t] = h3[0]; roles[t] = h3[1]; state[t] = h3[2];
      if (!rd(f, s[t], p * cols[t])) return 2;
      if (state[t] && (!rd(f, m[t], p * cols[t]) || !rd(f, v[t], p * cols[t]))) return 2;
    }
    std::vector<uint8_t> code(p);
    std::vector<uint32_t> ok(p + 1), oc(p + 1), os(p + 1);
    int64_t counts[3];
    if (dh_plan(accum.data(), denom.data(), scaling.data(), opacity.data(), radii.data(), P, par[0], par[1], par[2], par[3], par[4], N, flags,
                code.data(), ok.data(), oc.data(), os.data(), counts)) return 3;
    const size_t pn = (size_t)(counts[0] + counts[1] + (int64_t)N * counts[2]);
    const float *ps[DENS_MAX_TENSORS], *pm[DENS_MAX_TENSORS], *pv[DENS_MAX_TENSORS];
    float *qs[DENS_MAX_TENSORS], *qm[DENS_MAX_TENSORS], *qv[DENS_MAX_TENSORS];
    for (int t = 0; t < n; ++t) {
      ds[t].assign(pn * cols[t], -7.25f);
      if (state[t]) { dm[t].assign(pn * cols[t], -7.25f); dv[t].assign(pn * cols[t], -7.25f); }
      ps[t] = s[t].data(); qs[t] = ds[t].data();
      pm[t] = state[t] ? m[t].data() : nullptr; pv[t] = state[t] ? v[t].data() : nullptr;
      qm[t] = state[t] ? dm[t].data() : nullptr; qv[t] = state[t] ? dv[t].data() : nullptr;
    }
    std::vector<uint8_t> mo(pn);
    std::vector<int32_t> org(pn), knd(pn);
    if (dh_apply(code.data(), ok.data(), oc.data(), os.data(), P, counts, n, ps, qs, pm, pv, qm, qv, cols, roles, rotation.data(), N, seed,
                 hd[3] ? normals.data() : nullptr, hd[4] ? mask.data() : nullptr, mo.data(), org.data(), knd.data())) return 3;
    uint32_t h = 2166136261u;     // FNV-1a over every output: the test compares it with the library's
    for (int t = 0; t < n; ++t) {
      h = fnv(h, ds[t].data(), ds[t].size() * 4);
      if (state[t]) { h = fnv(h, dm[t].data(), dm[t].size() * 4); h = fnv(h, dv[t].data(), dv[t].size() * 4); }
    }
    h = fnv(h, mo.data(), mo.size()); h = fnv(h, org.data(), org.size() * 4); h = fnv(h, knd.data(), knd.size() * 4);
    printf("call %d rows %lld counts %lld %lld %lld hash %u\n", k, (long long)P, (long long)counts[0], (long long)counts[1], (long long)counts[2], h);
  }
  fclose(f);
  printf("calls %d\n", ncalls);
  return 0;
}
#endif
