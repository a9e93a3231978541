// Wave-wide reductions of the float64 fits, in a fixed order: the 64-bit minimum on (float bits << 32 | index) keys, the float64 sum
// and the centroid of a set of atoms.  Shared by ddmi_pose_fit (k_metrics.hip) and conformer matching (k_match.hip): every caller
// adds the same lanes in the same order.
#pragma once
#include "kernels.h"

namespace ddmi {

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m, 64), lo = (unsigned)__shfl_xor((int)(unsigned)v, m, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(b >> 32), m, 64), lo = (unsigned)__shfl_xor((int)(unsigned)b, m, 64);
    v += __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
  }
  return v;
}

// one wave: c[0..2] = the centroid of the m atoms atom(j), c[3] = sum_j |atom(j) - centroid|^2
template <class Atom> __device__ __forceinline__ void fit_center(const Atom& atom, int m, int lane, double* c) {
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int j = lane; j < m; j += 64) {
    float x, y, z;
    atom(j, x, y, z);
    sx += (double)x; sy += (double)y; sz += (double)z;
  }
  const double cx = wave_sum_f64(sx) / (double)m, cy = wave_sum_f64(sy) / (double)m, cz = wave_sum_f64(sz) / (double)m;
  double g = 0.0;
  for (int j = lane; j < m; j += 64) {
    float x, y, z;
    atom(j, x, y, z);
    const double dx = (double)x - cx, dy = (double)y - cy, dz = (double)z - cz;
    g = fma(dz, dz, fma(dy, dy, fma(dx, dx, g)));
  }
  c[0] = cx; c[1] = cy; c[2] = cz; c[3] = wave_sum_f64(g);
}

}  // namespace ddmi
