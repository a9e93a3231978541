// Cyclic Jacobi on a symmetric 4x4 in float64: the eigen-solver of Horn's quaternion problem, shared by the Kabsch step of
// conformer_update (k_sample.hip) and the minimised RMSD of ddmi_pose_fit (k_metrics.hip).  Every caller runs the same rotations in
// the same order.
#pragma once
#include "kernels.h"

namespace ddmi {

// dominant eigenvector q of a symmetric 4x4 A (row-major, destroyed) and its eigenvalue, the largest (cyclic Jacobi, float64)
__device__ inline double max_eigvec4(double* A, double* q) {
  double V[16];
  for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0;
    for (int p = 0; p < 4; ++p) for (int r = p + 1; r < 4; ++r) off += A[p * 4 + r] * A[p * 4 + r];
    if (off < 1e-30) break;
    for (int p = 0; p < 3; ++p)
      for (int r = p + 1; r < 4; ++r) {
        const double apr = A[p * 4 + r];
        if (fabs(apr) < 1e-300) continue;
        const double theta = (A[r * 4 + r] - A[p * 4 + p]) / (2.0 * apr);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) {
          const double akp = A[k * 4 + p], akr = A[k * 4 + r];
          A[k * 4 + p] = c * akp - s * akr;
          A[k * 4 + r] = s * akp + c * akr;
        }
        for (int k = 0; k < 4; ++k) {
          const double apk = A[p * 4 + k], ark = A[r * 4 + k];
          A[p * 4 + k] = c * apk - s * ark;
          A[r * 4 + k] = s * apk + c * ark;
        }
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k * 4 + p], vkr = V[k * 4 + r];
          V[k * 4 + p] = c * vkp - s * vkr;
          V[k * 4 + r] = s * vkp + c * vkr;
        }
      }
  }
  int best = 0;
  for (int i = 1; i < 4; ++i) if (A[i * 4 + i] > A[best * 4 + best]) best = i;
  for (int k = 0; k < 4; ++k) q[k] = V[k * 4 + best];
  return A[best * 4 + best];
}

// Horn's key matrix of M = sum a b^T (row-major 3x3): its dominant eigenvector (w, x, y, z) is the rotation that moves a onto b,
// its largest eigenvalue lambda gives the residual sum |a|^2 + |b|^2 - 2 lambda (spyrmsd/qcp.py:55-122 writes the same matrix for
// the transposed M, which has the same eigenvalues).
__device__ __forceinline__ void horn_key_matrix(const double* S, double* N) {
  const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
  N[0] = Sxx + Syy + Szz; N[1] = Syz - Szy; N[2] = Szx - Sxz; N[3] = Sxy - Syx;
  N[4] = Syz - Szy; N[5] = Sxx - Syy - Szz; N[6] = Sxy + Syx; N[7] = Szx + Sxz;
  N[8] = Szx - Sxz; N[9] = Sxy + Syx; N[10] = -Sxx + Syy - Szz; N[11] = Syz + Szy;
  N[12] = Sxy - Syx; N[13] = Szx + Sxz; N[14] = Syz + Szy; N[15] = -Sxx - Syy + Szz;
}
// the proper rotation of a quaternion of any non-zero length, row-major
__device__ __forceinline__ void quat_rotation(const double* q, double* Rk) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double n2 = w * w + x * x + y * y + z * z;
  const double s2 = 2.0 / n2;
  Rk[0] = 1 - s2 * (y * y + z * z); Rk[1] = s2 * (x * y - z * w); Rk[2] = s2 * (x * z + y * w);
  Rk[3] = s2 * (x * y + z * w); Rk[4] = 1 - s2 * (x * x + z * z); Rk[5] = s2 * (y * z - x * w);
  Rk[6] = s2 * (x * z - y * w); Rk[7] = s2 * (y * z + x * w); Rk[8] = 1 - s2 * (x * x + y * y);
}

}  // namespace ddmi
