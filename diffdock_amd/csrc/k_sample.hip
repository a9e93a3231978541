// Reverse-diffusion step on the device (reference utils/sampling.py:117-191):
//   k_perturb           NaN guard (:117-131) + score/noise combination (:133-186) with the
//                       step's scalar coefficients computed on the host in float64 exactly as
//                       the reference's 0-dim float64 tensors are
//   k_modify_conformer  modify_conformer_batch (utils/diffusion_utils.py:60-78): rigid update
//                       (axis_angle_to_matrix, utils/geometry.py:39-86), sequential torsion
//                       updates (utils/torsion.py:75-90), Kabsch re-alignment
//                       (utils/geometry.py:246-276).  The optimal proper rotation is obtained
//                       from Horn's quaternion eigenproblem (float64 Jacobi) instead of an SVD
//                       with reflection fix: the same minimiser, no 3x3 SVD kernel needed.
#include "axis_angle.h"
#include "jacobi4.h"
#include "kernels.h"
#include "philox.h"

namespace ddmi {

// test entry points: the generator exactly as k_perturb uses it
__global__ void k_debug_philox(const unsigned* __restrict__ ctr, const unsigned* __restrict__ key, int n, unsigned* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned o[4];
  philox4x32(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], key[2 * i], key[2 * i + 1], o);
  for (int j = 0; j < 4; ++j) out[4 * i + j] = o[j];
}
__global__ void k_debug_normal(unsigned long long seed, long long sample0, int n_samples, int step, int n_comp, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n_samples * n_comp) return;
  const long long s = i / n_comp;
  out[i] = normal_draw(seed, sample0 + s, step, (int)(i - s * n_comp));
}
void launch_debug_philox(const unsigned* ctr, const unsigned* key, int n, unsigned* out, hipStream_t s) {
  hipLaunchKernelGGL(k_debug_philox, dim3(cdiv(n, 256)), dim3(256), 0, s, ctr, key, n, out);
  DDMI_CHECK_HIP(hipGetLastError());
}
void launch_debug_normal(unsigned long long seed, long long sample0, int n_samples, int step, int n_comp, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_debug_normal, dim3(cdiv((long)n_samples * n_comp, 256)), dim3(256), 0, s, seed, sample0, n_samples, step, n_comp, out);
  DDMI_CHECK_HIP(hipGetLastError());
}

__device__ __forceinline__ float mul_add_rn(float cs, float s, float cz, float z) {
#ifdef DDMI_HIPEMU
  volatile float a = cs * s, b = cz * z;
  return a + b;
#else
  return __fadd_rn(__fmul_rn(cs, s), __fmul_rn(cz, z));
#endif
}

__device__ void nan_fix(float* x, int n, float* red, int tid) {
  // eps = 0.01 * nanmean(|x|);  nan -> eps, +inf -> eps, -inf -> -eps
  float s = 0.f, c = 0.f;
  for (int i = tid; i < n; i += 256) { const float v = fabsf(x[i]); if (!(v != v)) { s += v; c += 1.f; } }
  red[tid] = s; red[256 + tid] = c;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) { red[tid] += red[tid + off]; red[256 + tid] += red[256 + tid + off]; }
    __syncthreads();
  }
  const float eps = 0.01f * (red[0] / red[256]);
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const float v = x[i];
    if (v != v) x[i] = eps;
    else if (isinf(v)) x[i] = v > 0.f ? eps : -eps;
  }
}

__global__ __launch_bounds__(256) void k_perturb(PerturbArgs a) {
  __shared__ float red[512];
  __shared__ int flag, n_nan;
  const int tid = threadIdx.x;
  if (tid == 0) { flag = 0; n_nan = 0; }
  __syncthreads();
  for (int b = tid; b < a.B; b += 256) {
    const float m = (a.tr[3 * b] + a.tr[3 * b + 1] + a.tr[3 * b + 2]) / 3.f;
    if (m != m) { flag = 1; if (a.rec_nan) atomicAdd(&n_nan, 1); }
  }
  __syncthreads();
  if (a.rec_nan && tid == 0) a.rec_nan[0] = n_nan;
  if (flag) {
    nan_fix(a.tr, 3 * a.B, red, tid);
    __syncthreads();
    nan_fix(a.rot, 3 * a.B, red, tid);
    __syncthreads();
    if (a.R > 0) nan_fix(a.tor, a.B * a.R, red, tid);
    __syncthreads();
  }
  for (int i = tid; i < 3 * a.B; i += 256) {
    const int b = i / 3, k = i - 3 * b;
    const long long sid = a.sample_ids ? a.sample_ids[b] : b;
    const float zt = a.z_tr ? a.z_tr[i] : (a.use_rng ? normal_draw(a.seed, sid, a.step, k) : 0.f);
    const float zr = a.z_rot ? a.z_rot[i] : (a.use_rng ? normal_draw(a.seed, sid, a.step, 3 + k) : 0.f);
    const float st = a.tr[i], sr = a.rot[i];
    if (a.rec_tr) a.rec_tr[i] = st;
    if (a.rec_rot) a.rec_rot[i] = sr;
    a.tr[i] = mul_add_rn(a.c_tr_s, st, a.c_tr_z, zt);
    a.rot[i] = mul_add_rn(a.c_rot_s, sr, a.c_rot_z, zr);
  }
  for (int i = tid; i < a.B * a.R; i += 256) {
    const int b = i / a.R, k = i - b * a.R;
    const long long sid = a.sample_ids ? a.sample_ids[b] : b;
    const float z = a.z_tor ? a.z_tor[i] : (a.use_rng ? normal_draw(a.seed, sid, a.step, 6 + k) : 0.f);
    const float st = a.tor[i];
    if (a.rec_tor) a.rec_tor[i] = st;
    a.tor[i] = mul_add_rn(a.c_tor_s, st, a.c_tor_z, z);
  }
}
void launch_perturb(const PerturbArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_perturb, dim3(1), dim3(256), 0, s, a);
  DDMI_CHECK_HIP(hipGetLastError());
}

// k_perturb per NaN-guard group (ddmi_set_batch_layout): workgroup g owns graphs [group_ptr[g], group_ptr[g+1]) and their
// torsions; its guard reads and fixes only those rows.  With one group of copies this is k_perturb's arithmetic and order.
__global__ __launch_bounds__(256) void k_perturb_grouped(PerturbArgs a, const int* __restrict__ group_ptr,
                                                         const int* __restrict__ tor_ptr, const int* __restrict__ tor_batch) {
  __shared__ float red[512];
  __shared__ int flag, n_nan;
  const int tid = threadIdx.x;
  const int b0 = group_ptr[blockIdx.x], b1 = group_ptr[blockIdx.x + 1];
  const int t0 = a.tor ? tor_ptr[b0] : 0, t1 = a.tor ? tor_ptr[b1] : 0;
  float* tr = a.tr + 3 * b0; float* rot = a.rot + 3 * b0;
  const int nb = b1 - b0;
  if (tid == 0) { flag = 0; n_nan = 0; }
  __syncthreads();
  for (int b = tid; b < nb; b += 256) {
    const float m = (tr[3 * b] + tr[3 * b + 1] + tr[3 * b + 2]) / 3.f;
    if (m != m) { flag = 1; if (a.rec_nan) atomicAdd(&n_nan, 1); }
  }
  __syncthreads();
  if (a.rec_nan && tid == 0) a.rec_nan[blockIdx.x] = n_nan;
  if (flag) {
    nan_fix(tr, 3 * nb, red, tid);
    __syncthreads();
    nan_fix(rot, 3 * nb, red, tid);
    __syncthreads();
    if (t1 > t0) nan_fix(a.tor + t0, t1 - t0, red, tid);
    __syncthreads();
  }
  for (int i = 3 * b0 + tid; i < 3 * b1; i += 256) {
    const int b = i / 3, k = i - 3 * b;
    const long long sid = a.sample_ids ? a.sample_ids[b] : b;
    const float zt = a.z_tr ? a.z_tr[i] : (a.use_rng ? normal_draw(a.seed, sid, a.step, k) : 0.f);
    const float zr = a.z_rot ? a.z_rot[i] : (a.use_rng ? normal_draw(a.seed, sid, a.step, 3 + k) : 0.f);
    const float st = a.tr[i], sr = a.rot[i];
    if (a.rec_tr) a.rec_tr[i] = st;
    if (a.rec_rot) a.rec_rot[i] = sr;
    a.tr[i] = mul_add_rn(a.c_tr_s, st, a.c_tr_z, zt);
    a.rot[i] = mul_add_rn(a.c_rot_s, sr, a.c_rot_z, zr);
  }
  for (int i = t0 + tid; i < t1; i += 256) {
    const int b = tor_batch[i], k = i - tor_ptr[b];
    const long long sid = a.sample_ids ? a.sample_ids[b] : b;
    const float z = a.z_tor ? a.z_tor[i] : (a.use_rng ? normal_draw(a.seed, sid, a.step, 6 + k) : 0.f);
    const float st = a.tor[i];
    if (a.rec_tor) a.rec_tor[i] = st;
    a.tor[i] = mul_add_rn(a.c_tor_s, st, a.c_tor_z, z);
  }
}
void launch_perturb_grouped(const PerturbArgs& a, int G, const int* group_ptr, const int* tor_ptr, const int* tor_batch,
                            hipStream_t s) {
  if (G <= 0) return;
  hipLaunchKernelGGL(k_perturb_grouped, dim3(G), dim3(256), 0, s, a, group_ptr, tor_ptr, tor_batch);
  DDMI_CHECK_HIP(hipGetLastError());
}

__global__ void k_fill_times(float* __restrict__ t, int B, float t_tr, float t_rot, float t_tor) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) { t[i] = t_tr; t[B + i] = t_rot; t[2 * B + i] = t_tor; }
}
// set_time of EVERY step of a sampling loop in one launch: t[k][3][B] (the times are host scalars: they ride in the kernel arguments)
__global__ void k_fill_times_all(float* __restrict__ t, int B, StepTimes st) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
  if (i < B) {
    float* __restrict__ tk = t + (size_t)k * 3 * B;
    tk[i] = st.t[3 * k]; tk[B + i] = st.t[3 * k + 1]; tk[2 * B + i] = st.t[3 * k + 2];
  }
}
void launch_fill_times_all(float* t, int B, const StepTimes& st, hipStream_t s) {
  hipLaunchKernelGGL(k_fill_times_all, dim3(cdiv(B, 256), st.steps), dim3(256), 0, s, t, B, st);
  DDMI_CHECK_HIP(hipGetLastError());
}
void launch_fill_times(float* t, int B, float t_tr, float t_rot, float t_tor, hipStream_t s) {
  hipLaunchKernelGGL(k_fill_times, dim3(cdiv(B, 256)), dim3(256), 0, s, t, B, t_tr, t_rot, t_tor);
  DDMI_CHECK_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ conformer update
// one graph (64 threads): p [Nl][3] in place; tr / rot [3] and tor [R] (or nullptr) are the graph's updates, rot_u / rot_v
// graph-local atom indices, mask_rotate its [R][Nl] block.  smem holds 6 * Nl + 16 floats.  rp: nullptr, or the graph's [Nl][3]
// block of a record row (ddmi_set_sample_record) that receives the final coordinates as well.
__device__ __forceinline__ void conformer_update(float* __restrict__ p, float* __restrict__ rp, int Nl, int R, const int* __restrict__ rot_u,
                                                 const int* __restrict__ rot_v, const unsigned char* __restrict__ mask_rotate,
                                                 const float* __restrict__ tr, const float* __restrict__ rot,
                                                 const float* __restrict__ tor, float* smem) {
  float* rigid = smem;            // [Nl][3]
  float* flex = smem + 3 * Nl;    // [Nl][3]
  float* sc = flex + 3 * Nl;      // scratch: centre(3), R(9), t(3)
  const int tid = threadIdx.x;
  for (int i = tid; i < 3 * Nl; i += 64) flex[i] = p[i];
  __syncthreads();
  if (tid == 0) {
    float cx = 0.f, cy = 0.f, cz = 0.f;
    for (int a = 0; a < Nl; ++a) { cx += flex[3 * a]; cy += flex[3 * a + 1]; cz += flex[3 * a + 2]; }
    sc[0] = cx / Nl; sc[1] = cy / Nl; sc[2] = cz / Nl;
    axis_angle_to_matrix(rot[0], rot[1], rot[2], sc + 3);
  }
  __syncthreads();
  for (int a = tid; a < Nl; a += 64) {
    const float x = flex[3 * a] - sc[0], y = flex[3 * a + 1] - sc[1], z = flex[3 * a + 2] - sc[2];
    for (int k = 0; k < 3; ++k)
      rigid[3 * a + k] = (sc[3 + 3 * k] * x + sc[4 + 3 * k] * y + sc[5 + 3 * k] * z) + tr[k] + sc[k];
  }
  __syncthreads();
  if (tor == nullptr || R == 0) {
    for (int i = tid; i < 3 * Nl; i += 64) p[i] = rigid[i];
    if (rp) for (int i = tid; i < 3 * Nl; i += 64) rp[i] = rigid[i];
    return;
  }
  for (int i = tid; i < 3 * Nl; i += 64) flex[i] = rigid[i];
  __syncthreads();
  for (int idx = 0; idx < R; ++idx) {
    const int u = rot_u[idx], v = rot_v[idx];
    const float vx = flex[3 * u] - flex[3 * v], vy = flex[3 * u + 1] - flex[3 * v + 1], vz = flex[3 * u + 2] - flex[3 * v + 2];
    const float px = flex[3 * v], py = flex[3 * v + 1], pz = flex[3 * v + 2];
    __syncthreads();
    const float nrm = sqrtf(vx * vx + vy * vy + vz * vz);
    const float th = tor[idx];
    float Rm[9];
    axis_angle_to_matrix(vx / nrm * th, vy / nrm * th, vz / nrm * th, Rm);
    for (int a = tid; a < Nl; a += 64) {
      if (!mask_rotate[(size_t)idx * Nl + a]) continue;
      const float x = flex[3 * a] - px, y = flex[3 * a + 1] - py, z = flex[3 * a + 2] - pz;
      flex[3 * a] = (Rm[0] * x + Rm[1] * y + Rm[2] * z) + px;
      flex[3 * a + 1] = (Rm[3] * x + Rm[4] * y + Rm[5] * z) + py;
      flex[3 * a + 2] = (Rm[6] * x + Rm[7] * y + Rm[8] * z) + pz;
    }
    __syncthreads();
  }
  if (tid == 0) {
    double cA[3] = {0, 0, 0}, cB[3] = {0, 0, 0};
    for (int a = 0; a < Nl; ++a)
      for (int k = 0; k < 3; ++k) { cA[k] += flex[3 * a + k]; cB[k] += rigid[3 * a + k]; }
    for (int k = 0; k < 3; ++k) { cA[k] /= Nl; cB[k] /= Nl; }
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int a = 0; a < Nl; ++a)
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) S[3 * i + j] += (flex[3 * a + i] - cA[i]) * (rigid[3 * a + j] - cB[j]);
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double N[16] = {Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx,
                    Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz,
                    Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy,
                    Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz};
    double q[4];
    max_eigvec4(N, q);
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double n2 = w * w + x * x + y * y + z * z;
    const double s2 = 2.0 / n2;
    double Rk[9] = {1 - s2 * (y * y + z * z), s2 * (x * y - z * w), s2 * (x * z + y * w),
                    s2 * (x * y + z * w), 1 - s2 * (x * x + z * z), s2 * (y * z - x * w),
                    s2 * (x * z - y * w), s2 * (y * z + x * w), 1 - s2 * (x * x + y * y)};
    for (int i = 0; i < 9; ++i) sc[3 + i] = (float)Rk[i];
    for (int i = 0; i < 3; ++i) sc[12 + i] = (float)(cB[i] - (Rk[3 * i] * cA[0] + Rk[3 * i + 1] * cA[1] + Rk[3 * i + 2] * cA[2]));
  }
  __syncthreads();
  for (int a = tid; a < Nl; a += 64) {
    const float x = flex[3 * a], y = flex[3 * a + 1], z = flex[3 * a + 2];
    float out[3];
    for (int k = 0; k < 3; ++k) out[k] = (sc[3 + 3 * k] * x + sc[4 + 3 * k] * y + sc[5 + 3 * k] * z) + sc[12 + k];
    for (int k = 0; k < 3; ++k) p[3 * a + k] = out[k];
    if (rp) for (int k = 0; k < 3; ++k) rp[3 * a + k] = out[k];
  }
}
// block (64 threads) per sample
__global__ __launch_bounds__(64) void k_modify_conformer(float* __restrict__ pos, int Nl, int R,
                                                         const int* __restrict__ rot_u, const int* __restrict__ rot_v,
                                                         const unsigned char* __restrict__ mask_rotate,
                                                         const float* __restrict__ tr, const float* __restrict__ rot,
                                                         const float* __restrict__ tor, float* __restrict__ rec_pos) {
  DDMI_DYN_SMEM(float, smem);
  const int b = blockIdx.x;
  conformer_update(pos + (size_t)b * Nl * 3, rec_pos ? rec_pos + (size_t)b * Nl * 3 : nullptr, Nl, R, rot_u, rot_v, mask_rotate, tr + 3 * b, rot + 3 * b,
                   tor ? tor + (size_t)b * R : nullptr, smem);
}
// block (64 threads) per graph of a batch of different complexes (ddmi_set_batch_layout)
__global__ __launch_bounds__(64) void k_modify_conformer_ragged(float* __restrict__ pos, const int* __restrict__ lig_ptr,
                                                                const int* __restrict__ tor_ptr, const int* __restrict__ rot_u,
                                                                const int* __restrict__ rot_v, const long long* __restrict__ mask_off,
                                                                const unsigned char* __restrict__ mask_rotate,
                                                                const float* __restrict__ tr, const float* __restrict__ rot,
                                                                const float* __restrict__ tor, float* __restrict__ rec_pos) {
  DDMI_DYN_SMEM(float, smem);
  const int b = blockIdx.x;
  const int a0 = lig_ptr[b], t0 = tor_ptr[b];
  const int R = tor ? tor_ptr[b + 1] - t0 : 0;
  conformer_update(pos + (size_t)a0 * 3, rec_pos ? rec_pos + (size_t)a0 * 3 : nullptr, lig_ptr[b + 1] - a0, R, rot_u + t0, rot_v + t0, R ? mask_rotate + mask_off[b] : nullptr,
                   tr + 3 * b, rot + 3 * b, R ? tor + t0 : nullptr, smem);
}
void launch_modify_conformer(float* pos, int B, int Nl, int R, const int* rot_u, const int* rot_v,
                             const unsigned char* mask_rotate, const float* tr, const float* rot, const float* tor,
                             float* rec_pos, hipStream_t s) {
  if (B <= 0) return;
  const size_t smem = (size_t)(6 * Nl + 16) * sizeof(float);
  hipLaunchKernelGGL(k_modify_conformer, dim3(B), dim3(64), smem, s, pos, Nl, R, rot_u, rot_v, mask_rotate, tr, rot, tor, rec_pos);
  DDMI_CHECK_HIP(hipGetLastError());
}
void launch_modify_conformer_ragged(float* pos, int B, int maxNl, const int* lig_ptr, const int* tor_ptr, const int* rot_u,
                                    const int* rot_v, const long long* mask_off, const unsigned char* mask_rotate, const float* tr,
                                    const float* rot, const float* tor, float* rec_pos, hipStream_t s) {
  if (B <= 0) return;
  const size_t smem = (size_t)(6 * maxNl + 16) * sizeof(float);
  hipLaunchKernelGGL(k_modify_conformer_ragged, dim3(B), dim3(64), smem, s, pos, lig_ptr, tor_ptr, rot_u, rot_v, mask_off,
                     mask_rotate, tr, rot, tor, rec_pos);
  DDMI_CHECK_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ initial poses
// randomize_position (utils/sampling.py:16-58) for one graph per workgroup (64 threads), in place on the graph's block of pos:
// sequential torsion rotations WITHOUT re-alignment (modify_conformer_torsion_angles, utils/torsion.py:48-72), then
// (pos - mean) R^T + centre, then the translation.  Draws the caller does not supply come from philox4x32 at step -1
// (ddmi_randomize_cfg in include/ddmi.h has the component table).  One kernel serves the batch of copies (a.lig_ptr == nullptr)
// and the ragged layout, so that a graph's arithmetic is the same instruction stream in both.  smem: 3 * Nl + 32 floats.
__global__ __launch_bounds__(64) void k_randomize_position(RandomizeArgs a) {
  DDMI_DYN_SMEM(float, smem);
  const int b = blockIdx.x, tid = threadIdx.x;
  const int a0 = a.lig_ptr ? a.lig_ptr[b] : b * a.Nl;
  const int Nl = a.lig_ptr ? a.lig_ptr[b + 1] - a0 : a.Nl;
  const int t0 = a.lig_ptr ? a.tor_ptr[b] : b * a.R;
  const int R = a.no_torsion ? 0 : (a.lig_ptr ? a.tor_ptr[b + 1] - t0 : a.R);
  const int* __restrict__ rot_u = a.rot_u + (a.lig_ptr ? t0 : 0);
  const int* __restrict__ rot_v = a.rot_v + (a.lig_ptr ? t0 : 0);
  const unsigned char* __restrict__ mask = R ? a.mask_rotate + (a.lig_ptr ? a.mask_off[b] : 0) : nullptr;
  const long long sid = a.sample_ids ? a.sample_ids[b] : b;
  float* __restrict__ p = a.pos + (size_t)a0 * 3;
  float* x = smem;            // [Nl][3]
  float* sc = smem + 3 * Nl;  // mean(3), R(9), t(3), -, normals(7), residue index(1)
  for (int i = tid; i < 3 * Nl; i += 64) x[i] = p[i];
  if (tid < 7) sc[16 + tid] = normal_draw(a.seed, sid, -1, tid);
  if (tid == 7) {
    int idx = 0;
    if (a.choose_residue) {
      unsigned o[4];
      philox4x32((unsigned)sid, (unsigned)((unsigned long long)sid >> 32), (unsigned)-1, 7u, (unsigned)a.seed, (unsigned)(a.seed >> 32), o);
      const int r0 = a.rec_ptr[b];
      idx = r0 + (int)(o[0] % (unsigned)(a.rec_ptr[b + 1] - r0));
    }
    reinterpret_cast<int*>(sc)[23] = idx;
  }
  __syncthreads();
  for (int j = 0; j < R; ++j) {
    float th;
    if (a.tor_updates) th = a.tor_updates[t0 + j];
    else {   // (2u - 1) pi with u = ((word0 >> 8) + 0.5) / 2^24: every operation below is exact up to the last product, |th| < pi
      unsigned o[4];
      philox4x32((unsigned)sid, (unsigned)((unsigned long long)sid >> 32), (unsigned)-1, (unsigned)(8 + j), (unsigned)a.seed,
                 (unsigned)(a.seed >> 32), o);
      th = ((float)((int)(o[0] >> 8) - 8388608) + 0.5f) * (3.14159265358979f / 8388608.f);
    }
    if (th == 0.f) continue;   // the reference skips an update of exactly 0 (the same decision in every thread)
    const int u = rot_u[j], v = rot_v[j];
    const float vx = x[3 * u] - x[3 * v], vy = x[3 * u + 1] - x[3 * v + 1], vz = x[3 * u + 2] - x[3 * v + 2];
    const float px = x[3 * v], py = x[3 * v + 1], pz = x[3 * v + 2];
    __syncthreads();
    const float nrm = sqrtf(vx * vx + vy * vy + vz * vz);
    float Rm[9];
    axis_angle_to_matrix(vx / nrm * th, vy / nrm * th, vz / nrm * th, Rm);
    for (int i = tid; i < Nl; i += 64) {
      if (!mask[(size_t)j * Nl + i]) continue;
      const float dx = x[3 * i] - px, dy = x[3 * i + 1] - py, dz = x[3 * i + 2] - pz;
      x[3 * i] = (Rm[0] * dx + Rm[1] * dy + Rm[2] * dz) + px;
      x[3 * i + 1] = (Rm[3] * dx + Rm[4] * dy + Rm[5] * dz) + py;
      x[3 * i + 2] = (Rm[6] * dx + Rm[7] * dy + Rm[8] * dz) + pz;
    }
    __syncthreads();
  }
  if (tid < 3) {   // molecule centre and translation, one coordinate per thread
    float s = 0.f;
    for (int i = 0; i < Nl; ++i) s += x[3 * i + tid];
    sc[tid] = s / Nl;
    float t = 0.f;
    if (!a.no_random) {
      if (a.tr_updates) t = a.tr_updates[3 * b + tid];
      else if (a.choose_residue) t = a.rec_pos[3 * (size_t)reinterpret_cast<const int*>(sc)[23] + tid] + 0.01f * sc[20 + tid];
      else t = a.tr_std * sc[20 + tid];
    }
    sc[12 + tid] = t;
  }
  if (tid == 3) {
    if (a.rotations) {
      for (int i = 0; i < 9; ++i) sc[3 + i] = a.rotations[9 * (size_t)b + i];
    } else {   // unit quaternion (w, x, y, z) -> matrix
      const float n = sqrtf(sc[16] * sc[16] + sc[17] * sc[17] + sc[18] * sc[18] + sc[19] * sc[19]);
      const float w = sc[16] / n, qx = sc[17] / n, qy = sc[18] / n, qz = sc[19] / n;
      sc[3] = 1 - 2 * (qy * qy + qz * qz); sc[4] = 2 * (qx * qy - qz * w); sc[5] = 2 * (qx * qz + qy * w);
      sc[6] = 2 * (qx * qy + qz * w); sc[7] = 1 - 2 * (qx * qx + qz * qz); sc[8] = 2 * (qy * qz - qx * w);
      sc[9] = 2 * (qx * qz - qy * w); sc[10] = 2 * (qy * qz + qx * w); sc[11] = 1 - 2 * (qx * qx + qy * qy);
    }
  }
  __syncthreads();
  for (int i = tid; i < Nl; i += 64) {
    const float dx = x[3 * i] - sc[0], dy = x[3 * i + 1] - sc[1], dz = x[3 * i + 2] - sc[2];
    for (int k = 0; k < 3; ++k)
      p[3 * i + k] = ((sc[3 + 3 * k] * dx + sc[4 + 3 * k] * dy + sc[5 + 3 * k] * dz) + a.center[3 * b + k]) + sc[12 + k];
  }
}
void launch_randomize_position(const RandomizeArgs& a, int maxNl, hipStream_t s) {
  if (a.B <= 0) return;
  const size_t smem = (size_t)(3 * maxNl + 32) * sizeof(float);
  hipLaunchKernelGGL(k_randomize_position, dim3(a.B), dim3(64), smem, s, a);
  DDMI_CHECK_HIP(hipGetLastError());
}

}  // namespace ddmi
