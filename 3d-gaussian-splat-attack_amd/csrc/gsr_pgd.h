// gsr_pgd.h -- the scalar side of the projected-gradient step (gsr_pgd_step, gsr_pgd_step_normed, gsr_pgd_step_multi of
// include/gsraster.h): the L-inf element update, the L2 move, the scale from a sum of squares, a row's clip factor, the
// rows a wave owns, the number of partial sums, and the tensor a workgroup of the multi launch belongs to.
//
// One source, compiled twice: by hipcc into the kernels of gsr_pgd.hip.h and the launch set-up in gsr_api.hip, and by g++
// into a host harness (tests/host_math/pgd_host.cpp) that runs the step in plain loops.  Every operation here is a
// single IEEE operation or an explicit fmaf, so both builds give the same bits from the same sum of squares.
//
// The contract (include/gsraster.h), in float32 unless said otherwise:
//   L-inf:  out = x0 + clamp((x - alpha * sign(g)) - x0, -eps, eps), sign(0) = 0.
//   L2:     nrm = sqrtf((float)sum of g^2) over the WHOLE tensor; xn = x - (alpha / nrm) * g when nrm > 0, else xn = x;
//           d = xn - x0; a row with ||d|| > eps gives x0 + d * (eps / (||d|| + 1e-7)), any other row x0 + d.
//           A row with ||d|| == eps exactly is NOT clipped.
// Non-finite and out-of-range inputs (the results of the tensor formulation, gsplat_attack/pgd.py, on the CPU):
//   * sign(NaN) = 0: a NaN gradient element does not move its x under L-inf; sign(+-inf) = +-1.
//   * L2, a NaN gradient element or a NaN sum of squares: the norm is NaN, which is not > 0: NO step for the whole
//     tensor, the NaN element included (xn = x there too: pgd_l2_move tests the element, so a NaN gradient element
//     never moves its x, whatever sum is handed in); the projection still runs.
//   * L2, an infinite gradient element or a sum of squares of +inf: the norm is +inf, alpha / nrm = 0: no step at the
//     finite elements, NaN at the infinite one (0 * inf).
//   * A NaN in x or x0 comes out NaN at that element under both rules (the L-inf clamp is written with comparisons:
//     fminf / fmaxf would drop the NaN and return x0 - eps).  Under L-inf x = +-inf gives x0 +- eps, x0 = +-inf gives
//     +-inf.
//   * L2, a row of d holding a NaN has a NaN norm, which is not > eps: the row is NOT clipped (its other elements are
//     x0 + d).  A row of d holding +-inf (x or x0 infinite) has the factor eps / inf = 0: NaN at that element, x0 at
//     the others.
//   * eps = 0 returns x0 (L2: the factor is 0 for every row with d != 0); alpha = 0 is the projection alone.
//   * Range of the L2 step.  The norm is a float32: a sum of squares that overflows it (|g| >= 1e19 on 12 elements or
//     more) gives nrm = +inf and the tensor takes NO step (x stays finite).  A sum handed in as a double
//     (gsr_pgd_step_normed) is used down to a norm of FLT_MIN (1.2e-38); below that the tensor takes no step.  A sum
//     taken by k_pgd_sumsq is float32 per thread (double across threads): squares that underflow float32
//     (|g| <= 1e-23: g^2 = 0) count as 0 -- no step when all do -- and squares that are float32 denormals (|g| below
//     about 1e-19) carry few bits, so the step's length is approximate there.  Between 1e-15 and 1e15 the step is
//     held to the float64 oracle (tests/pgd_cases.py).
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gsr_math.h"   // GSR_HD

namespace gsr {

constexpr int PGD_MAX_COLS = 48;
// Rows per wave: 64 for narrow rows; 32 for rows wider than PGD_NARROW floats, so that a wave's deltas take 6 KB of LDS
// instead of 12 and 16 waves fit a CU where 12 did (the kernel is bandwidth-bound: more waves = more loads in flight).
constexpr int PGD_NARROW = 24;
constexpr int PGD_LDS_FLOATS = 64 * PGD_NARROW > 32 * PGD_MAX_COLS ? 64 * PGD_NARROW : 32 * PGD_MAX_COLS;
constexpr int PGD_MAX_TENSORS = 8;
// k_pgd_sumsq: one partial sum per workgroup of 256 threads, 4096 floats per workgroup until the grid is capped
constexpr int PGD_SUMSQ_BLOCK_FLOATS = 4096;
constexpr int PGD_SUMSQ_MAX_BLOCKS = 1024;

GSR_HD int pgd_rows_per_wave(int cols) { return cols > PGD_NARROW ? 32 : 64; }

// workgroups of k_pgd_sumsq (= partial sums) for a tensor of n floats, n > 0
GSR_HD int pgd_sumsq_blocks(size_t n) {
  const size_t nb = (n + (size_t)(PGD_SUMSQ_BLOCK_FLOATS - 1)) / (size_t)PGD_SUMSQ_BLOCK_FLOATS;
  return (int)(nb < (size_t)PGD_SUMSQ_MAX_BLOCKS ? nb : (size_t)PGD_SUMSQ_MAX_BLOCKS);
}

// L-inf: the whole update of one element
GSR_HD float pgd_linf_update(float x, float g, float x0, float alpha, float eps) {
  const float sg = g > 0.f ? 1.f : (g < 0.f ? -1.f : 0.f);          // torch.sign; sign(NaN) = 0
  const float xn = fmaf(-alpha, sg, x);
  float d = xn - x0;
  d = d < -eps ? -eps : d;                                          // comparisons, not fmaxf / fminf: a NaN stays a NaN
  d = d > eps ? eps : d;
  return d + x0;
}

// L2: alpha / ||g|| from the sum of squares; 0 unless the norm is > 0 (so 0 for a zero and for a NaN norm: no step).
// A sum that is a normal float32 takes sqrtf((float)t), the bits the kernels have always given.  A smaller one would
// become a float32 denormal of a few bits and give a step of the wrong length: its root is taken in double, and counts
// only if it is a normal float32 itself (below that alpha / nrm overflows), else as 0.
GSR_HD float pgd_l2_scale(double t, float alpha) {
  float nrm = sqrtf((float)t);
  if (!(t >= (double)FLT_MIN)) {                 // also taken by a NaN sum: no step
    nrm = (float)sqrt(t);
    if (!(nrm >= FLT_MIN)) nrm = 0.f;
  }
  return nrm > 0.f ? alpha / nrm : 0.f;
}
// L2: the move of one element.  A NaN gradient element makes the norm NaN and the scale 0; the tensor formulation then
// takes no step at all, the NaN element included, where fmaf(-0, NaN, x) would leave a NaN: the element is tested.
GSR_HD float pgd_l2_move(float x, float g, float scale) { return g == g ? fmaf(-scale, g, x) : x; }

// L2: one more term of a row's sum of squared deltas; the row's factor from its norm; the element's result
GSR_HD float pgd_row_accum(float d, float ss) { return fmaf(d, d, ss); }
GSR_HD float pgd_row_factor(float nrm, float eps) { return nrm > eps ? eps / (nrm + 1e-7f) : 1.f; }
GSR_HD float pgd_l2_result(float d, float f, float x0) { return fmaf(d, f, x0); }

// gsr_pgd_step_multi: workgroup b belongs to the tensor t with first[t] <= b < first[t + 1] (n tensors, first[n] = the
// grid; a tensor without rows has first[t] == first[t + 1] and owns no workgroup, wherever it stands)
GSR_HD int pgd_tensor_of_block(const unsigned* first, int n, unsigned b) {
  int t = 0;
#pragma unroll
  for (int i = 1; i < PGD_MAX_TENSORS; ++i) t += (i < n && b >= first[i]) ? 1 : 0;
  return t;
}

}  // namespace gsr
