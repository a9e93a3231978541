// axis_angle_to_matrix (utils/geometry.py:39-86) in float32: the rotation of every torsion step, shared by the conformer updates of
// k_sample.hip and the objective of conformer matching (k_match.hip).
#pragma once
#include "kernels.h"

namespace ddmi {

__device__ __forceinline__ void axis_angle_to_matrix(float ax, float ay, float az, float* R) {
  const float angle = sqrtf(ax * ax + ay * ay + az * az);
  const float half = 0.5f * angle;
  const float s = fabsf(angle) < 1e-6f ? 0.5f - (angle * angle) / 48.f : sinf(half) / angle;
  const float r = cosf(half), i = ax * s, j = ay * s, k = az * s;
  const float two_s = 2.0f / (r * r + i * i + j * j + k * k);
  R[0] = 1 - two_s * (j * j + k * k); R[1] = two_s * (i * j - k * r); R[2] = two_s * (i * k + j * r);
  R[3] = two_s * (i * j + k * r); R[4] = 1 - two_s * (i * i + k * k); R[5] = two_s * (j * k - i * r);
  R[6] = two_s * (i * k - j * r); R[7] = two_s * (j * k + i * r); R[8] = 1 - two_s * (i * i + j * j);
}

}  // namespace ddmi
