// Pose metrics on the device (ddmi_pose_metrics, include/ddmi.h): the symmetry-corrected RMSD of evaluate.py:474-484 (spyrmsd's
// _rmsd_isomorphic_core with minimize = center = False, spyrmsd/rmsd.py:179-203: a min over graph isomorphisms of a sum of squared
// distances), the uncorrected RMSD of evaluate.py:481, the centroid distance of :486, the minimum intra-ligand distance of
// :503-505 and the minimum distance to a caller-given point set.
//
// Two launches, no atomics:
//   k_pose_sums    one workgroup (4 waves) per (pose p, reference k, chunk c of MET_CHUNK permutations).  The kept atoms of the pose
//                  and the reference are staged in LDS, the permutation rows are streamed from global memory.  ONE WAVE owns the
//                  sum of one (p, k, s): lane l adds the atoms l, l + 64, .. in order, then the fixed butterfly of wave_sum -- the
//                  same instruction stream on the same inputs whatever P, K, S or the grid are, so the value of a triple is
//                  bit-identical in every call.  The minimum of a chunk is taken on the 64-bit word (float bits << 32 | s):
//                  non-negative floats order like their bit patterns, equal sums fall to the lowest s, a NaN sum loses to every
//                  number.  The workgroup of chunk 0 also owns the identity sum and the centroid distance of its (p, k).
//   k_pose_finish  one workgroup per pose: min over the chunks (rmsd_per_ref), then over the references in ascending k with a strict
//                  `<` (ties fall to the lowest k * S + s), and the two clearances, which are mins and so exact in any order.
// Molecules whose kept atoms do not fit the LDS budget (m > MET_LDS_ATOMS) run the same arithmetic in the same order on global memory.
#include <algorithm>

#include "jacobi4.h"
#include "kernels.h"
#include "wave_f64.h"

namespace ddmi {

constexpr int MET_WAVES = 4;

__device__ __forceinline__ int met_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
__device__ __forceinline__ float met_d2(float dx, float dy, float dz) { return fmaf(dz, dz, fmaf(dy, dy, dx * dx)); }
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}

// The kept atoms of one pose (m-space: atom j = pos[atom_index[j]]) and one reference, in LDS (STAGED) or in place.  An index outside
// its range is the caller's error; it is clamped so that it cannot read outside the arrays.
template <bool STAGED> struct MetView {
  const float* x;    // STAGED: LDS [m][3], compacted; else pos of the pose [n][3]
  const float* r;    // STAGED: LDS [m][3]; else ref of the reference [m][3]
  const int* ai; int n;
  __device__ __forceinline__ void pose(int j, float& px, float& py, float& pz) const {
    const int a = STAGED ? j : (ai ? met_clamp(ai[j], n) : j);
    px = x[3 * (size_t)a]; py = x[3 * (size_t)a + 1]; pz = x[3 * (size_t)a + 2];
  }
  __device__ __forceinline__ void refr(int j, float& px, float& py, float& pz) const {
    px = r[3 * (size_t)j]; py = r[3 * (size_t)j + 1]; pz = r[3 * (size_t)j + 2];
  }
};

// smem: MET_WAVES 64-bit words, then (STAGED) 6 m floats.
template <bool STAGED> __global__ __launch_bounds__(64 * MET_WAVES) void k_pose_sums(PoseMetricsArgs a, int p0) {
  DDMI_DYN_SMEM(unsigned long long, wk);
  float* xs = reinterpret_cast<float*>(wk + MET_WAVES);
  float* rs = xs + 3 * (size_t)a.m;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = (int)(blockIdx.x % (unsigned)a.C), k = (int)((blockIdx.x / (unsigned)a.C) % (unsigned)a.K);
  const int p = p0 + (int)(blockIdx.x / ((unsigned)a.C * (unsigned)a.K));
  const int m = a.m;
  const float* __restrict__ pos = a.pos + (size_t)p * a.n * 3;
  const float* __restrict__ ref = a.ref + (size_t)k * m * 3;
  MetView<STAGED> v{STAGED ? xs : pos, STAGED ? rs : ref, a.atom_index, a.n};
  if (STAGED) {
    for (int j = tid; j < m; j += 64 * MET_WAVES) {
      const int at = a.atom_index ? met_clamp(a.atom_index[j], a.n) : j;
      for (int d = 0; d < 3; ++d) { xs[3 * j + d] = pos[3 * (size_t)at + d]; rs[3 * j + d] = ref[3 * (size_t)j + d]; }
    }
    __syncthreads();
  }
  const int s_lo = c * MET_CHUNK, s_hi = a.S - s_lo > MET_CHUNK ? s_lo + MET_CHUNK : a.S;
  unsigned long long best = ~0ull;
  for (int s = s_lo + w; s < s_hi; s += MET_WAVES) {   // wave-uniform: every lane of the wave takes part in the butterfly
    const int* __restrict__ pr = a.perm ? a.perm + (size_t)s * m : nullptr;
    float acc = 0.f;
    for (int j = lane; j < m; j += 64) {
      float px, py, pz, qx, qy, qz;
      v.pose(j, px, py, pz);
      v.refr(pr ? met_clamp(pr[j], m) : j, qx, qy, qz);
      acc += met_d2(qx - px, qy - py, qz - pz);
    }
    acc = wave_sum(acc);
    const unsigned long long key = ((unsigned long long)__float_as_uint(acc) << 32) | (unsigned)s;
    best = key < best ? key : best;
  }
  if (lane == 0) wk[w] = best;
  if (c == 0 && w == 0) {   // identity sum (evaluate.py:481) and centroid distance (:486; mean(ref) - mean(pose) = mean(ref - pose), which does not cancel)
    float acc = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
    for (int j = lane; j < m; j += 64) {
      float px, py, pz, qx, qy, qz;
      v.pose(j, px, py, pz);
      v.refr(j, qx, qy, qz);
      const float dx = qx - px, dy = qy - py, dz = qz - pz;
      acc += met_d2(dx, dy, dz);
      sx += dx; sy += dy; sz += dz;
    }
    acc = wave_sum(acc); sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
    if (lane == 0) {
      const size_t pk = (size_t)p * a.K + k;
      a.part_plain[pk] = acc;
      a.part_cd[pk] = sqrtf(met_d2(sx / (float)m, sy / (float)m, sz / (float)m));
    }
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long b = wk[0];
    for (int i = 1; i < MET_WAVES; ++i) b = wk[i] < b ? wk[i] : b;
    a.part_key[((size_t)p * a.K + k) * a.C + c] = b;
  }
}

// smem: 2 * MET_WAVES floats, then (STAGED) 3 m floats.
template <bool STAGED> __global__ __launch_bounds__(64 * MET_WAVES) void k_pose_finish(PoseMetricsArgs a) {
  DDMI_DYN_SMEM(unsigned, red);
  float* xs = reinterpret_cast<float*>(red + 2 * MET_WAVES);
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int m = a.m, K = a.K, C = a.C;
  const float* __restrict__ pos = a.pos + (size_t)p * a.n * 3;
  MetView<STAGED> v{STAGED ? xs : pos, nullptr, a.atom_index, a.n};
  const bool clear = a.min_self || a.min_point;   // (min_point without points is written as +inf)
  if (STAGED && clear) {
    for (int j = tid; j < m; j += 64 * MET_WAVES) {
      const int at = a.atom_index ? met_clamp(a.atom_index[j], a.n) : j;
      for (int d = 0; d < 3; ++d) xs[3 * j + d] = pos[3 * (size_t)at + d];
    }
  }
  if (w == 0) {   // the RMSD outputs: min over chunks, then over references in ascending k
    unsigned bv = 0xffffffffu, bs = 0; int bk = 0;
    for (int k = 0; k < K; ++k) {
      const unsigned long long* __restrict__ pk = a.part_key + ((size_t)p * K + k) * C;
      unsigned long long key = ~0ull;
      for (int c = lane; c < C; c += 64) key = pk[c] < key ? pk[c] : key;
      key = wave_min_u64(key);
      const unsigned val = (unsigned)(key >> 32);
      if (lane == 0 && a.rmsd_per_ref) a.rmsd_per_ref[(size_t)p * K + k] = sqrtf(__uint_as_float(val) / (float)m);
      if (val < bv) { bv = val; bs = (unsigned)key; bk = k; }
    }
    unsigned pl = 0xffffffffu, cd = 0xffffffffu;
    for (int k = lane; k < K; k += 64) {
      pl = min(pl, __float_as_uint(a.part_plain[(size_t)p * K + k]));
      cd = min(cd, __float_as_uint(a.part_cd[(size_t)p * K + k]));
    }
    pl = wave_min_u32(pl); cd = wave_min_u32(cd);
    if (lane == 0) {
      if (a.rmsd) a.rmsd[p] = sqrtf(__uint_as_float(bv) / (float)m);
      if (a.best) { a.best[2 * (size_t)p] = bk; a.best[2 * (size_t)p + 1] = (int)bs; }
      if (a.rmsd_plain) a.rmsd_plain[p] = sqrtf(__uint_as_float(pl) / (float)m);
      if (a.centroid) a.centroid[p] = __uint_as_float(cd);
    }
  }
  if (!clear) return;   // (the same decision in every thread)
  __syncthreads();
  const unsigned INF = 0x7f800000u;
  unsigned self = INF, pt = INF;
  if (a.min_self)
    for (int i = tid; i < m; i += 64 * MET_WAVES) {
      float px, py, pz;
      v.pose(i, px, py, pz);
      for (int j = i + 1; j < m; ++j) {
        float qx, qy, qz;
        v.pose(j, qx, qy, qz);
        self = min(self, __float_as_uint(met_d2(qx - px, qy - py, qz - pz)));
      }
    }
  if (a.min_point && a.points)
    for (int q = tid; q < a.Q; q += 64 * MET_WAVES) {
      const float qx = a.points[3 * (size_t)q], qy = a.points[3 * (size_t)q + 1], qz = a.points[3 * (size_t)q + 2];
      for (int j = 0; j < m; ++j) {
        float px, py, pz;
        v.pose(j, px, py, pz);
        pt = min(pt, __float_as_uint(met_d2(qx - px, qy - py, qz - pz)));
      }
    }
  self = wave_min_u32(self); pt = wave_min_u32(pt);
  if (lane == 0) { red[w] = self; red[MET_WAVES + w] = pt; }
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < MET_WAVES; ++i) { self = min(self, red[i]); pt = min(pt, red[MET_WAVES + i]); }
    if (a.min_self) a.min_self[p] = sqrtf(__uint_as_float(self));
    if (a.min_point) a.min_point[p] = sqrtf(__uint_as_float(pt));
  }
}

void launch_pose_metrics(const PoseMetricsArgs& a, hipStream_t s) {
  if (a.P <= 0) return;
  const bool staged = a.m <= MET_LDS_ATOMS;
  const size_t smem1 = MET_WAVES * sizeof(unsigned long long) + (staged ? 6 * (size_t)a.m * sizeof(float) : 0);
  const size_t smem2 = 2 * MET_WAVES * sizeof(unsigned) + (staged ? 3 * (size_t)a.m * sizeof(float) : 0);
  const long per_pose = (long)a.K * a.C;
  const int step = (int)std::max(1L, std::min((long)a.P, (1L << 30) / per_pose));   // poses per launch: the grid stays below 2^31
  for (int p0 = 0; p0 < a.P; p0 += step) {
    const unsigned grid = (unsigned)(per_pose * std::min(step, a.P - p0));
    if (staged) hipLaunchKernelGGL(k_pose_sums<true>, dim3(grid), dim3(64 * MET_WAVES), smem1, s, a, p0);
    else hipLaunchKernelGGL(k_pose_sums<false>, dim3(grid), dim3(64 * MET_WAVES), smem1, s, a, p0);
    DDMI_CHECK_HIP(hipGetLastError());
  }
  if (staged) hipLaunchKernelGGL(k_pose_finish<true>, dim3(a.P), dim3(64 * MET_WAVES), smem2, s, a);
  else hipLaunchKernelGGL(k_pose_finish<false>, dim3(a.P), dim3(64 * MET_WAVES), smem2, s, a);
  DDMI_CHECK_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ ddmi_pose_fit
// The minimised symmetric RMSD (spyrmsd.rmsd.symmrmsd with minimize = True, spyrmsd/rmsd.py:179-203 and spyrmsd/qcp.py: for every
// graph isomorphism the RMSD after the optimal rigid superposition, then the min) and the transform that attains it.  For pose p,
// reference k, permutation s, with a_j = pos[p, atom_index[j]] and b_j = ref[k, perm[s, j]]:
//   ca = mean a_j, cb = mean b_j, Ga = sum |a_j - ca|^2, Gb = sum |b_j - cb|^2, M = sum (a_j - ca)(b_j - cb)^T,
//   lambda = the largest eigenvalue of Horn's key matrix of M, e = Ga + Gb - 2 lambda,
//   rmsd_min = 0 where |e| < 1e-9 (the reference's atol, qcp.py:283), else sqrt(max(e, 0) / m).
// ALL of it is float64 on the float32 inputs: e is a difference of numbers of size m r^2 and is m rmsd^2, which float32 cannot hold
// for a near-perfect conformer.  lambda comes from the cyclic Jacobi of jacobi4.h, which needs no special case where the largest
// eigenvalue is degenerate (m = 2, collinear atoms); the characteristic-polynomial Newton of QCP is not used.
// Two launches with the decomposition and the properties of the kernels above -- no atomics, no host synchronisation, scratch from
// the handle's growing pool, and the value of a triple depends on its own inputs only:
//   k_pose_fit_sums    one workgroup (4 waves) per (p, k, chunk of MET_CHUNK permutations), atoms staged in LDS as float32 or read in
//                      place as above.  Wave 0 computes (ca, Ga) and wave 1 (cb, Gb) before the loop: lane l adds the atoms l, l + 64,
//                      .. in order, then the fixed butterfly of wave_sum_f64 -- a function of the pose (the reference) alone, whatever
//                      P, K, S or the grid are.  ONE WAVE owns a triple: nine explicit-fma sums in the same lane order and the same
//                      butterfly; the sums of the wave's i-th triple stay in lane i, and the eigenvalues of its (up to 16) triples
//                      are found together, one lane each.  The chunk minimum is taken on (float bits of (float) e << 32 | s)
//                      with e clamped as above: rounding to float32 is monotone, so this is the rounding of the float64 minimum; equal
//                      keys fall to the lowest s and a NaN loses.
//   k_pose_fit_finish  one workgroup (one wave) per pose: min over the chunks, then over k ascending with a strict `<`; then M again for
//                      the winning (k, s), the dominant eigenvector q of its key matrix, the proper rotation R(q) (det = +1: QCP never
//                      reflects) and t = cb - R ca, so that R a_j + t ~ b_j; R and t are stored as float32.  m = 1 gives the identity.
//                      Where the largest eigenvalue is degenerate (m = 2, collinear atoms: any rotation about the common axis) every
//                      maximiser is a correct answer and the one returned is the one the Jacobi sweeps arrive at.
// (wave_sum_f64, wave_min_u64 and fit_center -- the centroid and the centred square sum of one set of atoms -- live in wave_f64.h)
// one wave: M [3][3] = sum_j (a_j - ca)(b_j - cb)^T with b_j = the reference atom pr[j] (pr == nullptr: j)
template <bool STAGED> __device__ __forceinline__ void fit_cross(const MetView<STAGED>& v, const int* __restrict__ pr, int m, int lane,
                                                                 const double* ca, const double* cb, double* M) {
  for (int i = 0; i < 9; ++i) M[i] = 0.0;
  for (int j = lane; j < m; j += 64) {
    float px, py, pz, qx, qy, qz;
    v.pose(j, px, py, pz);
    v.refr(pr ? met_clamp(pr[j], m) : j, qx, qy, qz);
    const double ax = (double)px - ca[0], ay = (double)py - ca[1], az = (double)pz - ca[2];
    const double bx = (double)qx - cb[0], by = (double)qy - cb[1], bz = (double)qz - cb[2];
    M[0] = fma(ax, bx, M[0]); M[1] = fma(ax, by, M[1]); M[2] = fma(ax, bz, M[2]);
    M[3] = fma(ay, bx, M[3]); M[4] = fma(ay, by, M[4]); M[5] = fma(ay, bz, M[5]);
    M[6] = fma(az, bx, M[6]); M[7] = fma(az, by, M[7]); M[8] = fma(az, bz, M[8]);
  }
  for (int i = 0; i < 9; ++i) M[i] = wave_sum_f64(M[i]);
}

// smem: MET_WAVES 64-bit words, 8 doubles (ca, Ga, cb, Gb), then (STAGED) 6 m floats.
template <bool STAGED> __global__ __launch_bounds__(64 * MET_WAVES) void k_pose_fit_sums(PoseFitArgs a, int p0) {
  DDMI_DYN_SMEM(unsigned long long, wk);
  double* cen = reinterpret_cast<double*>(wk + MET_WAVES);
  float* xs = reinterpret_cast<float*>(cen + 8);
  float* rs = xs + 3 * (size_t)a.m;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = (int)(blockIdx.x % (unsigned)a.C), k = (int)((blockIdx.x / (unsigned)a.C) % (unsigned)a.K);
  const int p = p0 + (int)(blockIdx.x / ((unsigned)a.C * (unsigned)a.K));
  const int m = a.m;
  const float* __restrict__ pos = a.pos + (size_t)p * a.n * 3;
  const float* __restrict__ ref = a.ref + (size_t)k * m * 3;
  MetView<STAGED> v{STAGED ? xs : pos, STAGED ? rs : ref, a.atom_index, a.n};
  if (STAGED) {
    for (int j = tid; j < m; j += 64 * MET_WAVES) {
      const int at = a.atom_index ? met_clamp(a.atom_index[j], a.n) : j;
      for (int d = 0; d < 3; ++d) { xs[3 * j + d] = pos[3 * (size_t)at + d]; rs[3 * j + d] = ref[3 * (size_t)j + d]; }
    }
    __syncthreads();
  }
  if (w < 2) {   // wave-uniform
    double cc[4];
    if (w == 0) fit_center([&](int j, float& x, float& y, float& z) { v.pose(j, x, y, z); }, m, lane, cc);
    else fit_center([&](int j, float& x, float& y, float& z) { v.refr(j, x, y, z); }, m, lane, cc);
    if (lane == 0) { cen[4 * w] = cc[0]; cen[4 * w + 1] = cc[1]; cen[4 * w + 2] = cc[2]; cen[4 * w + 3] = cc[3]; }
  }
  __syncthreads();
  double ca[3] = {cen[0], cen[1], cen[2]}, cb[3] = {cen[4], cen[5], cen[6]};
  const double G = cen[3] + cen[7];
  const int s_lo = c * MET_CHUNK, s_hi = a.S - s_lo > MET_CHUNK ? s_lo + MET_CHUNK : a.S;
  // The wave's triples s = s_lo + w + MET_WAVES i, i < MET_CHUNK / MET_WAVES <= 64: the sums of triple i are left in lane i, and the
  // eigenvalues of all of them are then found at once, one lane each -- the same instructions on the same sums in whichever lane.
  static_assert(MET_CHUNK <= 64 * MET_WAVES, "one lane per triple of a wave");
  double M[9], mine[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int i = 0;
  for (int s = s_lo + w; s < s_hi; s += MET_WAVES, ++i) {   // wave-uniform: every lane of the wave takes part in the butterflies
    fit_cross<STAGED>(v, a.perm ? a.perm + (size_t)s * m : nullptr, m, lane, ca, cb, M);
    for (int j = 0; j < 9; ++j) mine[j] = lane == i ? M[j] : mine[j];
  }
  unsigned long long best = ~0ull;
  if (lane < i) {
    double N[16], q[4];
    horn_key_matrix(mine, N);
    double e = G - 2.0 * max_eigvec4(N, q);
    e = fabs(e) < 1e-9 ? 0.0 : (e < 0.0 ? 0.0 : e);   // (a NaN stays a NaN)
    best = ((unsigned long long)__float_as_uint((float)e) << 32) | (unsigned)(s_lo + w + MET_WAVES * lane);
  }
  best = wave_min_u64(best);
  if (lane == 0) wk[w] = best;
  __syncthreads();
  if (tid == 0) {
    unsigned long long b = wk[0];
    for (int i = 1; i < MET_WAVES; ++i) b = wk[i] < b ? wk[i] : b;
    a.part_key[((size_t)p * a.K + k) * a.C + c] = b;
  }
}

__global__ __launch_bounds__(64) void k_pose_fit_finish(PoseFitArgs a) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const int m = a.m, K = a.K, C = a.C;
  unsigned bv = 0xffffffffu, bs = 0; int bk = 0;   // (the same in every lane: wave_min_u64 leaves the minimum in all of them)
  for (int k = 0; k < K; ++k) {
    const unsigned long long* __restrict__ pk = a.part_key + ((size_t)p * K + k) * C;
    unsigned long long key = ~0ull;
    for (int c = lane; c < C; c += 64) key = pk[c] < key ? pk[c] : key;
    key = wave_min_u64(key);
    const unsigned val = (unsigned)(key >> 32);
    if (lane == 0 && a.rmsd_min_per_ref) a.rmsd_min_per_ref[(size_t)p * K + k] = sqrtf(__uint_as_float(val) / (float)m);
    if (val < bv) { bv = val; bs = (unsigned)key; bk = k; }
  }
  if (lane == 0) {
    if (a.rmsd_min) a.rmsd_min[p] = sqrtf(__uint_as_float(bv) / (float)m);
    if (a.best_min) { a.best_min[2 * (size_t)p] = bk; a.best_min[2 * (size_t)p + 1] = (int)bs; }
  }
  if (!a.rotation && !a.translation) return;
  const int s = met_clamp((int)bs, a.S);
  MetView<false> v{a.pos + (size_t)p * a.n * 3, a.ref + (size_t)bk * m * 3, a.atom_index, a.n};
  double ca[4], cb[4], M[9];
  fit_center([&](int j, float& x, float& y, float& z) { v.pose(j, x, y, z); }, m, lane, ca);
  fit_center([&](int j, float& x, float& y, float& z) { v.refr(j, x, y, z); }, m, lane, cb);
  fit_cross<false>(v, a.perm ? a.perm + (size_t)s * m : nullptr, m, lane, ca, cb, M);
  if (lane == 0) {
    double N[16], q[4], R[9];
    horn_key_matrix(M, N);
    max_eigvec4(N, q);
    quat_rotation(q, R);
    if (a.rotation) for (int i = 0; i < 9; ++i) a.rotation[9 * (size_t)p + i] = (float)R[i];
    if (a.translation)
      for (int i = 0; i < 3; ++i) a.translation[3 * (size_t)p + i] = (float)(cb[i] - (R[3 * i] * ca[0] + R[3 * i + 1] * ca[1] + R[3 * i + 2] * ca[2]));
  }
}

void launch_pose_fit(const PoseFitArgs& a, hipStream_t s) {
  if (a.P <= 0) return;
  const bool staged = a.m <= MET_LDS_ATOMS;
  const size_t smem = MET_WAVES * sizeof(unsigned long long) + 8 * sizeof(double) + (staged ? 6 * (size_t)a.m * sizeof(float) : 0);
  const long per_pose = (long)a.K * a.C;
  const int step = (int)std::max(1L, std::min((long)a.P, (1L << 30) / per_pose));   // poses per launch: the grid stays below 2^31
  for (int p0 = 0; p0 < a.P; p0 += step) {
    const unsigned grid = (unsigned)(per_pose * std::min(step, a.P - p0));
    if (staged) hipLaunchKernelGGL(k_pose_fit_sums<true>, dim3(grid), dim3(64 * MET_WAVES), smem, s, a, p0);
    else hipLaunchKernelGGL(k_pose_fit_sums<false>, dim3(grid), dim3(64 * MET_WAVES), smem, s, a, p0);
    DDMI_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_pose_fit_finish, dim3(a.P), dim3(64), 0, s, a);
  DDMI_CHECK_HIP(hipGetLastError());
}

}  // namespace ddmi
