// gsr_adam.h -- the scalar side of the fused Adam step (gsr_adam_step_multi of include/gsraster.h): the update of one
// element, the bias corrections from the step count, the position schedule of the reference's fits, the span of a
// workgroup, the row of a flat element and the tensor a workgroup of the launch belongs to.
//
// One source, compiled twice: by hipcc into the kernel of gsr_adam.hip.h and the launch set-up in gsr_api.hip, and by g++
// into a host harness (tests/host_math/adam_host.cpp) that runs the step in plain loops.  Every operation of the element
// update is a single IEEE operation under GSR_FP_STRICT (no contraction), so both builds give the same bits.
//
// The update (float32), that of torch.optim.Adam without weight decay, amsgrad or maximize:
//   m'  = m + (1 - b1) * (g - m)
//   v'  = b2 * v + (1 - b2) * (g * g)
//   den = sqrtf(v') / sqrt_bc2 + eps
//   x'  = x - step_size * (m' / den)
// with step_size = lr / (1 - b1^t) and sqrt_bc2 = sqrt(1 - b2^t), formed on the HOST in double from the integer step
// count t >= 1 and rounded once to float32 (adam_bias_corrections below: the C entry point and the host harness share
// it; there is no device scalar and no read-back).
// The betas are float32 and 1 - b is formed from them: 1 - 0.999f = 0.00099998713 (exact), 1.29e-5 relative below the 0.001
// that torch rounds from its double 1 - 0.999; the weight of a new gradient in v' differs from a float32 torch run by that
// much and the step's length by about 6e-6 of itself, which the float64 oracle of tests/adam_cases.py, fed the float32
// betas, does not see.
//
// Non-finite and range contract (what torch.optim.Adam does on CPU float32 tensors, element by element):
//   * a NaN gradient element gives NaN in m', v' and x' at that element; +-inf gives m' = +-inf, v' = +inf and x' = NaN
//     (inf / inf); every other element is what it is without the bad one -- there is no reduction across elements.
//   * g = 0 with zero moments moves nothing: 0 / (0 + eps) = 0 (eps > 0; with eps = 0 it is 0 / 0 = NaN, as in torch).
//   * |g| so small that the square underflows float32 (below about 1e-21 with b2 = 0.999) leaves v' = b2 * v, from zero
//     state den = eps; m' still takes the gradient.
//   * |g| up to sqrt(FLT_MAX) = 1.84e19 keeps g * g and v' finite (1e19 gives v' = 1e35 and x moves as in torch); beyond
//     that g * g = +inf, v' = +inf, den = +inf, and x does not move (m' / inf = 0).  Here torch differs: its addcmul_
//     forms ((1 - b2) * g) * g, which stays finite up to |g| = 5.8e20 with b2 = 0.999.
//   * v at FLT_MAX stays finite under b2 < 1 and a moderate gradient; den is then about 1.8e19 / sqrt_bc2.
//   * lr = 0 (step_size = 0) updates the moments and leaves x bit for bit -- unless m' / den is NaN or inf, which 0
//     does not absorb.
//   * a NaN or infinity already in x, m or v stays at its element.
// Rows that a call's row mask or row range leaves out are not read and not written: x, m and v keep their bits, NaNs
// included.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gsr_math.h"   // GSR_HD, GSR_FP_STRICT

namespace gsr {

constexpr int ADAM_MAX_TENSORS = 8;
constexpr int ADAM_MAX_COLS = 48;
// k_adam_step_multi: a workgroup is one wave; a lane takes ADAM_VECS float4 of each stream, so a workgroup's span is
// ADAM_SPAN consecutive floats of one tensor (the unit of the row-selection skip)
constexpr int ADAM_BLOCK = 64;
constexpr int ADAM_VECS = 4;
constexpr int ADAM_SPAN = ADAM_BLOCK * ADAM_VECS * 4;

// workgroups of a tensor of n floats
GSR_HD unsigned long long adam_blocks(unsigned long long n) { return (n + (unsigned long long)(ADAM_SPAN - 1)) / (unsigned long long)ADAM_SPAN; }

// the row of flat element e of a [rows, cols] tensor
GSR_HD unsigned long long adam_row_of(unsigned long long e, int cols) { return e / (unsigned long long)cols; }

// workgroup b belongs to the tensor t with first[t] <= b < first[t + 1] (pgd_tensor_of_block's shape: a tensor without
// rows has first[t] == first[t + 1] and owns no workgroup, wherever it stands)
GSR_HD int adam_tensor_of_block(const unsigned* first, int n, unsigned b) {
  int t = 0;
#pragma unroll
  for (int i = 1; i < ADAM_MAX_TENSORS; ++i) t += (i < n && b >= first[i]) ? 1 : 0;
  return t;
}

// does row r move: inside [row_begin, row_end) and, with a mask, a non-zero byte
GSR_HD bool adam_row_live(unsigned long long r, const uint8_t* row_mask, unsigned long long row_begin, unsigned long long row_end) {
  return r >= row_begin && r < row_end && (row_mask == nullptr || row_mask[r] != 0);
}

// the update of one element, in place
GSR_HD void adam_update(float& x, float g, float& m, float& v, float step_size, float sqrt_bc2, float b1, float b2, float eps) {
  GSR_FP_STRICT
  const float w1 = 1.f - b1;
  const float w2 = 1.f - b2;
  const float gm = g - m;
  const float m1 = m + w1 * gm;
  const float gg = g * g;
  const float v1 = b2 * v + w2 * gg;
  const float den = sqrtf(v1) / sqrt_bc2 + eps;
  const float q = m1 / den;
  m = m1;
  v = v1;
  x = x - step_size * q;
}

// host: the two bias-correction scalars of step t >= 1, in double, rounded once
inline void adam_bias_corrections(double lr, double b1, double b2, long long t, float* step_size, float* sqrt_bc2) {
  *step_size = (float)(lr / (1.0 - pow(b1, (double)t)));
  *sqrt_bc2 = (float)sqrt(1.0 - pow(b2, (double)t));
}

// host: the position learning-rate schedule (log-linear from lr_init at step 0 to lr_final at max_steps, eased in over
// delay_steps by a sine from delay_mult); a negative step, or both rates zero, gives 0
inline double expon_lr(long long step, double lr_init, double lr_final, long long delay_steps, double delay_mult, long long max_steps) {
  if (step < 0 || (lr_init == 0.0 && lr_final == 0.0)) return 0.0;
  double delay_rate = 1.0;
  if (delay_steps > 0) {
    double c = (double)step / (double)delay_steps;
    c = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
    delay_rate = delay_mult + (1.0 - delay_mult) * sin((0.5 * 3.141592653589793) * c);
  }
  double t = (double)step / (double)max_steps;
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  const double log_lerp = exp(log(lr_init) * (1.0 - t) + log(lr_final) * t);
  return delay_rate * log_lerp;
}

}  // namespace gsr
