// The library's counter-based generator (Philox4x32-10) and the standard-normal draw keyed on it: shared by the step noise and the
// initial poses (k_sample.hip) and by the draws of conformer matching (k_match.hip).  Every caller runs the same rounds.
#pragma once
#include "kernels.h"

namespace ddmi {

// ------------------------------------------------------------------ counter-based RNG
__device__ __forceinline__ void philox4x32(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                           unsigned* out) {
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// standard normal keyed by (seed, sample, step, component)
__device__ __forceinline__ float normal_draw(unsigned long long seed, long long sample, int step, int comp) {
  unsigned o[4];
  philox4x32((unsigned)sample, (unsigned)((unsigned long long)sample >> 32), (unsigned)step, (unsigned)comp,
             (unsigned)seed, (unsigned)(seed >> 32), o);
  const float u1 = ((float)(o[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = ((float)(o[1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

}  // namespace ddmi
