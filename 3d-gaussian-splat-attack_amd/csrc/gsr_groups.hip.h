// gsr_groups.hip.h -- the groups set-up's per-Gaussian selection on gfx950: object classification and convex-hull
// inclusion.
//
// The reference picks the attacked object of a Gaussian-Grouping scene (attack.py:306-315) with
//   softmax(Conv2d(16, C, 1)(_objects_dc.permute(2, 0, 1)))[ids] > thresh  .any(0)
// -- [C, P] logits and a second [C, P] copy for the softmax, 2 GB at C = 256 and P = 1 M -- and ORs in the Gaussians
// inside the convex hull of the selected ones (scipy Delaunay on the host).  Here both are one pass over the Gaussians,
// one Gaussian per lane, and write a few bytes per Gaussian:
//   k_group_classify   psel = max over the selected ids of the softmax probability, mask = psel > thresh;
//   k_points_in_hull   inside = within the hull's box and n . x - c <= tau for every facet plane (gsr_hull.h);
//                      optionally out = mask | inside.
// No atomics, no workspace: results are bitwise reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

constexpr int GROUP_MAX_CLASSES = 1024;

struct GroupSel {
  uint32_t bits[GROUP_MAX_CLASSES / 32];   // bit c set: class c is one of the selected ids
};

// One Gaussian per lane.  objects [P,16] (the [P,1,16] _objects_dc), W [C,16], b [C].  The class loop index is
// wave-uniform, so W's rows and b are read with uniform addresses (one scalar-cache line serves the whole wave).
// A logit is b[c] + sum_k W[c,k] f[k] in double, k = 0..15 in order.  Pass 1: the largest logit m over all classes and
// the largest logit s over the selected ones.  Pass 2: sum over c of exp(l_c - m).  psel = exp(s - m) / sum: softmax is
// monotone in the logit, so that is the largest selected probability and (psel > thresh) is the reference's
// (prob[ids] > thresh).any(0).
__global__ void __launch_bounds__(256) k_group_classify(const float* __restrict__ objects, int P, const float* __restrict__ W,
                                                        const float* __restrict__ b, int C, GroupSel sel, float thresh,
                                                        float* __restrict__ psel, uint8_t* __restrict__ mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const float4* fp = reinterpret_cast<const float4*>(objects + (size_t)i * 16);
  double f[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = fp[q];
    f[4 * q] = v.x; f[4 * q + 1] = v.y; f[4 * q + 2] = v.z; f[4 * q + 3] = v.w;
  }
  auto logit = [&](int c) {
    const float* w = W + (size_t)c * 16;
    double l = (double)b[c];
#pragma unroll
    for (int k = 0; k < 16; ++k) l = fma((double)w[k], f[k], l);
    return l;
  };
  double m = -INFINITY, s = -INFINITY;
  for (int c = 0; c < C; ++c) {
    const double l = logit(c);
    m = fmax(m, l);
    if ((sel.bits[c >> 5] >> (c & 31)) & 1u) s = fmax(s, l);
  }
  double sum = 0.0;
  for (int c = 0; c < C; ++c) sum += exp(logit(c) - m);
  const float p = (float)(exp(s - m) / sum);
  psel[i] = p;
  mask[i] = p > thresh ? 1 : 0;
}

// The plane evaluation of gsr_hull::plane_dist, each operation rounded on its own (hipcc contracts a*b + c into an FMA
// unless told otherwise): the device verdict is the host's bit for bit.
__device__ __forceinline__ double hull_plane_dist(const double4 p, double x, double y, double z) {
  double s = __dmul_rn(p.x, x);
  s = __dadd_rn(s, __dmul_rn(p.y, y));
  s = __dadd_rn(s, __dmul_rn(p.z, z));
  return __dsub_rn(s, p.w);
}

// One Gaussian per lane.  planes [F] = (nx, ny, nz, c), bbox = min xyz, max xyz of the hull's points (both
// wave-uniform).  Inside = within the bounding box grown by tau on every side AND n . x - c <= tau for every facet.  The
// box test goes first; the other points walk the facets until one rejects them, and the wave leaves the facet loop as
// soon as every lane of it is rejected.  out[i] = inside, or mask_in[i] | inside with mask_in given.
__global__ void __launch_bounds__(256) k_points_in_hull(const float* __restrict__ xyz, int P, const double4* __restrict__ planes,
                                                        int F, const double* __restrict__ bbox, double tau,
                                                        const uint8_t* __restrict__ mask_in, uint8_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < P;
  double x = 0.0, y = 0.0, z = 0.0;
  if (live) { x = xyz[3 * (size_t)i]; y = xyz[3 * (size_t)i + 1]; z = xyz[3 * (size_t)i + 2]; }
  bool outside = !live || F <= 0 ||
                 !(x >= bbox[0] - tau && x <= bbox[3] + tau && y >= bbox[1] - tau && y <= bbox[4] + tau &&
                   z >= bbox[2] - tau && z <= bbox[5] + tau);
  for (int f = 0; f < F; ++f) {
    if (__all(outside)) break;
    const double4 pl = planes[f];
    if (!outside && hull_plane_dist(pl, x, y, z) > tau) outside = true;
  }
  if (!live) return;
  const uint8_t in = outside ? 0 : 1;
  out[i] = mask_in ? (uint8_t)((mask_in[i] != 0) | in) : in;
}

}  // namespace gsr
