// gsr_densify.h -- the scalar side of adaptive density control (gsr_densify_stats / gsr_densify_plan / gsr_densify_apply of
// include/gsraster.h; reference scene/gaussian_model.py:591-712): the statistic's update, the thresholds, the class of a row,
// the rows a row yields, build_rotation, a child's position and scale, the keyed normal and the launch arithmetic of the move.
//
// One source, compiled twice: by hipcc into the kernels of gsr_densify.hip.h and the entry points in gsr_api.hip, and by g++
// into a host harness (tests/host_math/densify_host.cpp) that runs the stage in plain loops.  Every rounding function is
// GSR_FP_STRICT (no contraction), so both builds give the same bits wherever no transcendental takes part.
//
// The reference's densify_and_prune is five passes (clone, postfix, split, prune of the parents, postfix, prune tests, prune)
// whose result is a pure function of the state before the call: densification_postfix zeroes max_radii2D for ALL rows before
// the prune mask is formed, so its screen-size test never fires (only max scale > 0.1 extent acts when max_screen_size is
// truthy), and clones enter the split pass with a padded gradient of 0, so only original rows split.  Per original row, with
// g = accum / denom (NaN -> 0), hot = g >= max_grad, smax = max of the row's three raw (log) scales, o = the raw (logit) opacity:
//   split  = hot && smax >  t_dense
//   clone  = hot && smax <= t_dense && !pruned(smax, o)         a copy of the raw rows, zero moments
//   keep   = !split && !pruned(smax, o) [&& !(radius > max_screen) with DENS_SCREEN_PRUNE]   itself, moments carried
//   kids   = split && !pruned(smax - c, o)                       N children, zero moments; the parent goes
//   pruned(s, o) = o < t_opac || (DENS_WORLD_PRUNE && s > t_world)
// Output order, the reference's: kept originals in row order, kept clones in parent order, children j-major (child j of the
// k-th kept split parent at n_keep + n_clone + j * n_split + k: repeat(N, 1)'s order).
//
// Every decision is a float comparison of a RAW value with a threshold in the log domain, formed on the host in double and
// rounded once (dens_thresholds): t_dense = log(percent_dense extent), t_world = log(0.1 extent), t_opac = logit(min_opacity),
// c = log(0.8 N).  No exp, log or sigmoid takes part in a decision, so the device's decisions are bit for bit the host
// build's; they differ from the reference's (which compares exp(raw) and sigmoid(raw)) only for a row within a few ulps of a
// threshold.  A child's scale is raw - c where the reference forms log(exp(raw) / (0.8 N)): the same value to an ulp or two,
// finite where exp overflows.  The only library calls left are in a child's position: expf of the scales and the keyed
// normals' logf (their sine and cosine are polynomials in single operations, dens_sincos_turn).
//
// Non-finite contract (what torch does row by row):
//   * a NaN among a row's raw scales makes smax NaN (torch.max propagates it): every comparison is false -- no clone, no split,
//     no world prune; the row is kept unless its opacity prunes it.
//   * a NaN opacity is not pruned (NaN < t is false).
//   * 0 / 0 statistics give gradient 0 (the reference's grads[grads.isnan()] = 0); an infinite mean gradient is hot.
//   * +inf raw scale: smax > every threshold, the row splits when hot and is world-pruned otherwise; -inf: clone when hot.
//   * a split row with a non-finite scale, rotation (a zero quaternion included: 0 / 0) or position gives children whose
//     positions are whatever the arithmetic gives (NaN or inf); the rasteriser culls such Gaussians.  Copies stay copies.
#pragma once
#include <math.h>
#include <cmath>
#include <stddef.h>
#include <stdint.h>

#include "gsr_adam.h"   // the walk of k_adam_step_multi: ADAM_SPAN, adam_blocks, adam_row_of, adam_tensor_of_block
#include "gsr_math.h"   // GSR_HD, GSR_FP_STRICT
#include "gsr_rcnn.h"   // mix32

namespace gsr {

constexpr int DENS_MAX_TENSORS = ADAM_MAX_TENSORS;   // 8
constexpr int DENS_MAX_COLS = ADAM_MAX_COLS;         // 48
constexpr int DENS_MAX_N = 8;                        // children of a split row
constexpr int DENS_BLOCK = ADAM_BLOCK;               // k_densify_move: a workgroup is one wave ...
constexpr int DENS_VECS = ADAM_VECS;
constexpr int DENS_SPAN = ADAM_SPAN;                 // ... and owns this many consecutive floats of one source tensor
constexpr long long DENS_MAX_ROWS = 1ll << 28;       // P and P'

// a tensor's role in the move
constexpr int DENS_COPY = 0;    // children copy the parent's row
constexpr int DENS_XYZ = 1;     // children are computed from the parent's xyz, rotation, scale and normals
constexpr int DENS_SCALE = 2;   // children get raw - c

// the class code of a row: which rows it yields
constexpr int DENS_KEEP = 1, DENS_CLONE = 2, DENS_KIDS = 4;
// kind[] of an output row: 0 keep, 1 clone, 2 + j child j
constexpr int DENS_KIND_KEEP = 0, DENS_KIND_CLONE = 1, DENS_KIND_CHILD = 2;

constexpr uint32_t DENS_WORLD_PRUNE = 1u;    // max_screen_size was truthy: prune max scale > 0.1 extent (the reference's live test)
constexpr uint32_t DENS_SCREEN_PRUNE = 2u;   // extension: prune original rows whose max_radii2D > max_screen_size

struct DensParams {
  float max_grad, t_dense, t_world, t_opac, c, max_screen;
  uint32_t flags;
  int N;
};

// span-to-tensor lookup and launch arithmetic: the Adam step's (one copy)
GSR_HD unsigned long long dens_blocks(unsigned long long n) { return adam_blocks(n); }
GSR_HD int dens_tensor_of_block(const unsigned* first, int n, unsigned b) { return adam_tensor_of_block(first, n, b); }

// ---- the statistics (reference add_densification_stats :710-712 and the max_radii2D line of its training loop) --------
// one view of one Gaussian that the filter lets through
GSR_HD void dens_stat_update(float& accum, float& denom, float gx, float gy) {
  GSR_FP_STRICT
  const float xx = gx * gx;
  const float yy = gy * gy;
  const float s = xx + yy;
  accum = accum + sqrtf(s);
  denom = denom + 1.f;
}
GSR_HD float dens_max_radius(float cur, int32_t radius) {
  const float r = (float)radius;
  return r > cur ? r : cur;          // torch.max(cur, r): cur is never NaN here unless it was given so, and then stays
}

// ---- the thresholds (host, double, rounded once) -------------------------------------------------------------------------
// -> 0, or which argument gives a threshold that is not finite: 1 max_grad, 2 extent (with percent_dense), 3 min_opacity,
// 4 N outside 1 .. DENS_MAX_N, 5 max_screen_size
inline int dens_thresholds(double max_grad, double min_opacity, double extent, double percent_dense, double max_screen_size, int N,
                           uint32_t flags, DensParams* p) {
  if (N < 1 || N > DENS_MAX_N) return 4;
  p->max_grad = (float)max_grad;
  p->t_dense = (float)log(percent_dense * extent);
  p->t_world = (float)log(0.1 * extent);
  p->t_opac = (float)log(min_opacity / (1.0 - min_opacity));
  p->c = (float)log(0.8 * (double)N);
  p->max_screen = (float)max_screen_size;
  p->flags = flags;
  p->N = N;
  if (!std::isfinite(p->max_grad)) return 1;
  if (!std::isfinite(p->t_dense) || !std::isfinite(p->t_world)) return 2;
  if (!std::isfinite(p->t_opac)) return 3;
  if (!std::isfinite(p->max_screen)) return 5;
  return 0;
}

// ---- the class of a row ----------------------------------------------------------------------------------------------------
GSR_HD float dens_mean_grad(float accum, float denom) {
  GSR_FP_STRICT
  const float g = accum / denom;
  return g != g ? 0.f : g;
}
// torch.max over the row: a NaN wins
GSR_HD float dens_max3(float a, float b, float c) {
  if (a != a || b != b || c != c) return NAN;
  const float m = a > b ? a : b;
  return m > c ? m : c;
}
GSR_HD bool dens_pruned(float s, float o, const DensParams& p) {
  return o < p.t_opac || ((p.flags & DENS_WORLD_PRUNE) != 0u && s > p.t_world);
}
// radius: the row's max_radii2D from before the call (read only with DENS_SCREEN_PRUNE)
GSR_HD int dens_classify(float g, float smax, float o, float radius, const DensParams& p) {
  GSR_FP_STRICT
  const bool hot = g >= p.max_grad;
  const bool split = hot && smax > p.t_dense;
  const bool own = dens_pruned(smax, o, p);
  const bool screen = (p.flags & DENS_SCREEN_PRUNE) != 0u && radius > p.max_screen;
  int code = 0;
  if (!split && !own && !screen) code |= DENS_KEEP;
  if (hot && smax <= p.t_dense && !own) code |= DENS_CLONE;
  if (split && !dens_pruned(smax - p.c, o, p)) code |= DENS_KIDS;
  return code;
}

// ---- the rows a row yields, from its three exclusive offsets and the totals ------------------------------------------------
GSR_HD unsigned dens_row_keep(unsigned off_keep) { return off_keep; }
GSR_HD unsigned dens_row_clone(unsigned off_clone, unsigned n_keep) { return n_keep + off_clone; }
GSR_HD unsigned dens_row_child(unsigned off_split, int j, unsigned n_keep, unsigned n_clone, unsigned n_split) {
  return n_keep + n_clone + (unsigned)j * n_split + off_split;
}

// ---- build_rotation as utils/general_utils.py:78-99 writes it: normalise, then the nine entries in that order ---------------
GSR_HD void dens_build_rotation(const float q_in[4], float R[9]) {
  GSR_FP_STRICT
  const float norm = sqrtf(q_in[0] * q_in[0] + q_in[1] * q_in[1] + q_in[2] * q_in[2] + q_in[3] * q_in[3]);
  const float r = q_in[0] / norm, x = q_in[1] / norm, y = q_in[2] / norm, z = q_in[3] / norm;
  R[0] = 1.f - 2.f * (y * y + z * z);
  R[1] = 2.f * (x * y - r * z);
  R[2] = 2.f * (x * z + r * y);
  R[3] = 2.f * (x * y + r * z);
  R[4] = 1.f - 2.f * (x * x + z * z);
  R[5] = 2.f * (y * z - r * x);
  R[6] = 2.f * (x * z - r * y);
  R[7] = 2.f * (y * z + r * x);
  R[8] = 1.f - 2.f * (x * x + y * y);
}

// ---- a child ------------------------------------------------------------------------------------------------------------------
// axis a of xyz + R(q) (z * exp(scale_raw)): torch.normal(0, std) = z std, bmm's three-term sum left to right, then + xyz
GSR_HD float dens_child_axis(const float xyz_a, const float q_in[4], const float scale_raw[3], const float z[3], int a) {
  GSR_FP_STRICT
  // row a of dens_build_rotation, entry by entry the same operations (no array indexed by a: registers, not scratch)
  const float norm = sqrtf(q_in[0] * q_in[0] + q_in[1] * q_in[1] + q_in[2] * q_in[2] + q_in[3] * q_in[3]);
  const float r = q_in[0] / norm, x = q_in[1] / norm, y = q_in[2] / norm, w = q_in[3] / norm;
  float r0, r1, r2;
  if (a == 0) {
    r0 = 1.f - 2.f * (y * y + w * w); r1 = 2.f * (x * y - r * w); r2 = 2.f * (x * w + r * y);
  } else if (a == 1) {
    r0 = 2.f * (x * y + r * w); r1 = 1.f - 2.f * (x * x + w * w); r2 = 2.f * (y * w - r * x);
  } else {
    r0 = 2.f * (x * w - r * y); r1 = 2.f * (y * w + r * x); r2 = 1.f - 2.f * (x * x + y * y);
  }
  const float v0 = z[0] * expf(scale_raw[0]);
  const float v1 = z[1] * expf(scale_raw[1]);
  const float v2 = z[2] * expf(scale_raw[2]);
  const float p0 = r0 * v0;
  const float p1 = r1 * v1;
  const float p2 = r2 * v2;
  const float s = (p0 + p1) + p2;
  return s + xyz_a;
}
GSR_HD float dens_child_scale(float scale_raw, float c) {
  GSR_FP_STRICT
  return scale_raw - c;
}

// ---- the keyed normal ------------------------------------------------------------------------------------------------------
// a uniform in (0, 1): 23 bits of mix32 over (seed, row, child, pair, which) plus a half, exact in float32
GSR_HD float dens_uniform(uint32_t seed, uint32_t row, int child, int pair, int which) {
  const uint32_t k = gsr_rcnn::mix32(gsr_rcnn::mix32(seed ^ (row * 0x9E3779B9u)) + (uint32_t)((child << 2) | (pair << 1) | which));
  return ((float)(k >> 9) + 0.5f) * (1.f / 8388608.f);
}
// sin and cos of 2 pi u for u in (0, 1), in operations that round once each, so that host and device give the same bits (the
// library sinf / cosf differ between the two, and their large-argument path costs the kernel scratch): k = the nearest quarter
// turn, f = 4u - k in [-1/2, 1/2] (exact), phi = f pi / 2 in [-pi/4, pi/4], Taylor to phi^9 (sin, truncation 1.7e-9) and
// phi^10 (cos, 1e-10), then the quarter turns.
GSR_HD void dens_sincos_turn(float u, float* s_out, float* c_out) {
  GSR_FP_STRICT
  const float t = 4.f * u;
  const float kf = floorf(t + 0.5f);
  const float f = t - kf;
  const float p = f * 1.5707963267948966f;
  const float p2 = p * p;
  const float sp = p * (1.f + p2 * (-1.6666667e-1f + p2 * (8.3333333e-3f + p2 * (-1.9841270e-4f + p2 * 2.7557319e-6f))));
  const float cp = 1.f + p2 * (-0.5f + p2 * (4.1666667e-2f + p2 * (-1.3888889e-3f + p2 * (2.4801587e-5f + p2 * -2.7557319e-7f))));
  const int k = (int)kf & 3;
  *s_out = k == 0 ? sp : (k == 1 ? cp : (k == 2 ? -sp : -cp));
  *c_out = k == 0 ? cp : (k == 1 ? -sp : (k == 2 ? -cp : sp));
}
// Box-Muller: pair 0 gives axes 0 (cos) and 1 (sin), pair 1 gives axis 2 (cos).  A function of (seed, row, child, axis) only;
// logf is the one library call.
GSR_HD float dens_normal(uint32_t seed, uint32_t row, int child, int axis) {
  GSR_FP_STRICT
  const int pair = axis >> 1;
  const float u1 = dens_uniform(seed, row, child, pair, 0);
  const float u2 = dens_uniform(seed, row, child, pair, 1);
  const float rad = sqrtf(-2.f * logf(u1));
  float sn, cs;
  dens_sincos_turn(u2, &sn, &cs);
  return rad * ((axis & 1) ? sn : cs);
}

}  // namespace gsr
