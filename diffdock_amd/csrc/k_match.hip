// Conformer matching on the device (ddmi_match_conformer, include/ddmi.h): the search of datasets/conformer_matching.py
// (optimize_rotatable_bonds, called from get_lig_graph_with_matching, datasets/process_mols.py:323-384) for the torsion angles that
// bring a generated conformer closest to the known pose.
//
// The objective.  For one job (start [n][3], target [n][3], R rotatable bonds) and an angle vector theta [R], E(theta) is the minimised
// RMSD between torsions(start, theta) and target:
//   torsions   the loop of utils/torsion.py:48-72 as k_randomize_position runs it: the bonds in edge order, bond j rotating the atoms of
//              its mask_rotate row about pos[v] by the axis-angle (pos[u] - pos[v]) / |..| * theta_j, in float32; an angle of exactly 0 is
//              skipped; no re-alignment (E does not change under a rigid motion).
//   RMSD       the formula of ddmi_pose_fit with the identity permutation: e = Ga + Gb - 2 lambda in float64 on the float32 coordinates
//              (fit_center of wave_f64.h, horn_key_matrix and max_eigvec4 of jacobi4.h), |e| < 1e-9 -> 0, E = sqrt(max(e, 0) / n).
//              Individuals are compared on (float) e, as k_pose_fit_sums compares; rounding and the square root are monotone.
// This restates the reference's objective with its two RDKit primitives replaced.  SetDihedralRad sets an ABSOLUTE dihedral; the angles
// here are RELATIVE to the start conformer.  Both are searched over a full period [-pi, pi] per bond, so the reachable conformers are
// the same: the box is shifted by the start conformer's dihedrals.  Which side of a bond turns does not matter after the
// superposition.  AlignMol uses the identity atom map and a proper rotation, as this fit does.
//
// The optimiser: differential evolution with scipy's strategy and the parameters of optimize_rotatable_bonds (best1bin, mutation
// (0.5, 1) dithered once per generation, recombination 0.8, population P = max(5, popsize R, n_init)).  Deliberate differences:
//   deferred updating   every trial of a generation is built from the population and the best member of the PREVIOUS generation
//                       (scipy's updating='deferred'; the reference runs 'immediate'), so a generation is P independent evaluations;
//   the zero row        without caller rows, row 0 of the initial population is all zeros (scipy has no such row): the result is never
//                       worse than the unmatched conformer;
//   no polish           no L-BFGS-B step at the end; accuracy is bought with generations.
// Generation g = 1 .. maxiter: F = U[0.5, 1); for individual i, r1 != r2, both != i, and the forced crossover index jrand;
// trial_j = best_j + F (pop[r1]_j - pop[r2]_j) where u_j < 0.8 or j = jrand, else pop[i]_j; a component outside [-pi, pi] is drawn
// again uniformly (scipy's rule); the trial replaces pop[i] when E(trial) <= E(pop[i]); after the generation the search stops when
// std(E) <= tol |mean(E)| (tol = 0 never stops early).  The draw table is in include/ddmi.h.
//
// One launch, no atomics, no host synchronisation, nothing depends on timing.  ONE WORKGROUP (MATCH_WAVES waves) per job runs every
// generation; ONE WAVE owns the evaluation of an individual and the waves take the individuals w, w + MATCH_WAVES, .. of a generation.
// Atoms are lane-strided (a = lane, lane + 64, ..); the wave's working conformer is in LDS; the float64 sums use the fixed butterfly of
// wave_sum_f64; the sums of the wave's k-th individual stay in lane k and the eigenvalues of up to 64 individuals are then found
// together, one lane each.  The population is kept twice (this generation, the next) with its energies, in LDS or in the handle's
// scratch (kernels.h has the rule and the limits); the minima are taken on (float bits << 32 | index), ties to the lower index.  A job
// reads only its own rows: its result depends on its inputs, its job id and the seed alone.
#include "axis_angle.h"
#include "jacobi4.h"
#include "kernels.h"
#include "philox.h"
#include "wave_f64.h"

namespace ddmi {

constexpr unsigned MATCH_INIT_WORD = 0xffffffffu;   // the generation word of the initial population, the individual word of F
constexpr float MATCH_BOUND = 3.14159250259399414f;  // the largest float32 below pi: the box [-pi, pi]

// (2u - 1) pi with u = ((word >> 8) + 0.5) / 2^24, the angle formula of k_randomize_position: |angle| < pi
__device__ __forceinline__ float match_angle(unsigned word) {
  return ((float)((int)(word >> 8) - 8388608) + 0.5f) * (3.14159265358979f / 8388608.f);
}
__device__ __forceinline__ void match_block(long long job_id, unsigned gen, unsigned c3, unsigned long long seed, unsigned* o) {
  philox4x32((unsigned)job_id, (unsigned)((unsigned long long)job_id >> 32), gen, c3, (unsigned)seed, (unsigned)(seed >> 32), o);
}

struct MatchJob {   // the job's staged inputs (LDS)
  const float *st, *tg;             // start, target [n][3]
  const unsigned long long* bits;   // [n]: bit j = atom turns with bond j
  const int *ru, *rv;               // [R], clamped into the job
  const double* cb;                 // centroid of target (3), Gb
  int n, R;
};

// One wave: torsions(start, th) into wk [n][3], then ca (centroid, Ga) and M = sum (a - ca)(b - cb)^T, the same in every lane.
__device__ __forceinline__ void match_eval(const MatchJob& jb, float* wk, const float* th, int lane, double* ca, double* M) {
  const int n = jb.n;
  for (int i = lane; i < 3 * n; i += 64) wk[i] = jb.st[i];
  DDMI_WAVE_SYNC();
  for (int j = 0; j < jb.R; ++j) {
    const float t = th[j];
    if (t == 0.f) continue;   // the reference skips an update of exactly 0 (the same decision in every lane)
    const int u = jb.ru[j], v = jb.rv[j];
    const float vx = wk[3 * u] - wk[3 * v], vy = wk[3 * u + 1] - wk[3 * v + 1], vz = wk[3 * u + 2] - wk[3 * v + 2];
    const float px = wk[3 * v], py = wk[3 * v + 1], pz = wk[3 * v + 2];
    DDMI_WAVE_SYNC();
    const float nrm = sqrtf(vx * vx + vy * vy + vz * vz);
    float Rm[9];
    axis_angle_to_matrix(vx / nrm * t, vy / nrm * t, vz / nrm * t, Rm);
    for (int i = lane; i < n; i += 64) {
      if (!((jb.bits[i] >> j) & 1ull)) continue;
      const float dx = wk[3 * i] - px, dy = wk[3 * i + 1] - py, dz = wk[3 * i + 2] - pz;
      wk[3 * i] = (Rm[0] * dx + Rm[1] * dy + Rm[2] * dz) + px;
      wk[3 * i + 1] = (Rm[3] * dx + Rm[4] * dy + Rm[5] * dz) + py;
      wk[3 * i + 2] = (Rm[6] * dx + Rm[7] * dy + Rm[8] * dz) + pz;
    }
    DDMI_WAVE_SYNC();
  }
  fit_center([&](int i, float& x, float& y, float& z) { x = wk[3 * i]; y = wk[3 * i + 1]; z = wk[3 * i + 2]; }, n, lane, ca);
  for (int i = 0; i < 9; ++i) M[i] = 0.0;
  for (int i = lane; i < n; i += 64) {
    const double ax = (double)wk[3 * i] - ca[0], ay = (double)wk[3 * i + 1] - ca[1], az = (double)wk[3 * i + 2] - ca[2];
    const double bx = (double)jb.tg[3 * i] - jb.cb[0], by = (double)jb.tg[3 * i + 1] - jb.cb[1], bz = (double)jb.tg[3 * i + 2] - jb.cb[2];
    M[0] = fma(ax, bx, M[0]); M[1] = fma(ax, by, M[1]); M[2] = fma(ax, bz, M[2]);
    M[3] = fma(ay, bx, M[3]); M[4] = fma(ay, by, M[4]); M[5] = fma(ay, bz, M[5]);
    M[6] = fma(az, bx, M[6]); M[7] = fma(az, by, M[7]); M[8] = fma(az, bz, M[8]);
  }
  for (int i = 0; i < 9; ++i) M[i] = wave_sum_f64(M[i]);
}

// one lane: the clamped residual e of the sums (M, Ga + Gb), rounded to float32 (a NaN stays a NaN)
__device__ __forceinline__ float match_residual(const double* M, double G) {
  double N[16], q[4];
  horn_key_matrix(M, N);
  double e = G - 2.0 * max_eigvec4(N, q);
  e = fabs(e) < 1e-9 ? 0.0 : (e < 0.0 ? 0.0 : e);
  return (float)e;
}

// smem: match_lds_bytes(n, R, P, POP_LDS) of kernels.h, in the order of the pointers below.
template <bool POP_LDS> __global__ __launch_bounds__(64 * MATCH_WAVES) void k_match(MatchArgs a) {
  DDMI_DYN_SMEM(double, cen);            // cb (3), Gb; then the final transform (12); then the partial sums of the waves (2 each)
  constexpr int W = MATCH_WAVES, T = 64 * MATCH_WAVES;
  const int job = a.job_list[blockIdx.x], tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int a0 = a.lig_ptr[job], n = a.lig_ptr[job + 1] - a0, t0 = a.tor_ptr[job], R = a.tor_ptr[job + 1] - t0;
  const int P = (int)match_population(R, a.popsize, a.n_init);
  const long long jid = a.job_ids[job];
  double* xf = cen + 4;
  double* red = cen + 16;
  unsigned long long* wkey = reinterpret_cast<unsigned long long*>(red + 2 * W);
  unsigned long long* bits = wkey + W;
  float* st = reinterpret_cast<float*>(bits + n);
  float* tg = st + 3 * n;
  float* work = tg + 3 * n + (size_t)w * 3 * n;            // this wave's conformer
  float* ang = tg + 3 * n + (size_t)W * 3 * n + 64 * w;    // this wave's angle vector
  int* ru = reinterpret_cast<int*>(tg + 3 * n + (size_t)W * 3 * n + 64 * W);
  int* rv = ru + R;
  float* pop = POP_LDS ? reinterpret_cast<float*>(rv + R) : a.pop_ws + a.pop_off[job];
  float* cur = pop;
  float* nxt = pop + (size_t)P * R;
  float* en = pop + 2 * (size_t)P * R;

  // ---- stage the job
  for (int i = tid; i < 3 * n; i += T) { st[i] = a.start[3 * (size_t)a0 + i]; tg[i] = a.target[3 * (size_t)a0 + i]; }
  for (int j = tid; j < R; j += T) {
    const int u = a.rot_u[t0 + j], v = a.rot_v[t0 + j];
    ru[j] = u < 0 ? 0 : (u >= n ? n - 1 : u);   // an index outside the job is the caller's error: it cannot read outside the arrays
    rv[j] = v < 0 ? 0 : (v >= n ? n - 1 : v);
  }
  const unsigned char* __restrict__ mask = R ? a.mask_rotate + a.mask_off[job] : nullptr;
  for (int i = tid; i < n; i += T) {
    unsigned long long b = 0;
    for (int j = 0; j < R; ++j) b |= (unsigned long long)(mask[(size_t)j * n + i] != 0) << j;
    bits[i] = b;
  }
  __syncthreads();
  if (w == 0) {   // the target's centroid and Gb, a function of the target alone
    double cc[4];
    fit_center([&](int i, float& x, float& y, float& z) { x = tg[3 * i]; y = tg[3 * i + 1]; z = tg[3 * i + 2]; }, n, lane, cc);
    if (lane == 0) { cen[0] = cc[0]; cen[1] = cc[1]; cen[2] = cc[2]; cen[3] = cc[3]; }
  }
  __syncthreads();
  const MatchJob jb{st, tg, bits, ru, rv, cen, n, R};
  const double Gb = cen[3];
  const float fn = (float)n;
  float* hist = a.best_history ? a.best_history + (size_t)job * (a.maxiter + 1) : nullptr;

  // the sums of the wave's k-th individual since the last flush stay in lane k
  double mine[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, mineG = 0.0, ca[4], M[9];
  auto keep = [&](int k) {
    for (int i = 0; i < 9; ++i) mine[i] = lane == k ? M[i] : mine[i];
    mineG = lane == k ? ca[3] + Gb : mineG;
  };

  // ---- the initial population: the caller's rows, else the zero row, then uniform draws
  {
    int k = 0, first = w;
    auto flush = [&]() {
      if (lane < k) {
        const int i = first + W * lane;
        const float ef = match_residual(mine, mineG);
        en[i] = ef;
        if (i < a.n_init && a.init_energy) a.init_energy[(size_t)job * a.n_init + i] = sqrtf(ef / fn);
      }
      first += W * k; k = 0;
    };
    for (int i = w; i < P; i += W) {   // wave-uniform
      if (lane < R) {
        float v;
        if (i < a.n_init) v = a.init_angles[(size_t)a.n_init * t0 + (size_t)i * R + lane];   // as given: the caller keeps them in the box
        else if (i == 0) v = 0.f;
        else {
          unsigned o[4];
          match_block(jid, MATCH_INIT_WORD, ((unsigned)i << 6) | (unsigned)(lane >> 2), a.seed, o);
          v = match_angle(o[lane & 3]);
        }
        cur[(size_t)i * R + lane] = v;
        ang[lane] = v;
      }
      match_eval(jb, work, ang, lane, ca, M);
      keep(k);
      if (++k == 64) flush();
    }
    flush();
  }

  // ---- the best member and the spread of the energies: the same in every thread
  unsigned best = 0; float best_e = 0.f; bool converged = false;
  auto survey = [&]() {
    __syncthreads();
    unsigned long long key = ~0ull;
    double s1 = 0.0, s2 = 0.0;
    for (int i = tid; i < P; i += T) {
      const float ef = en[i];
      const unsigned long long ki = ((unsigned long long)__float_as_uint(ef) << 32) | (unsigned)i;
      key = ki < key ? ki : key;
      const double x = sqrt((double)ef / (double)n);
      s1 += x; s2 = fma(x, x, s2);
    }
    key = wave_min_u64(key); s1 = wave_sum_f64(s1); s2 = wave_sum_f64(s2);
    if (lane == 0) { wkey[w] = key; red[2 * w] = s1; red[2 * w + 1] = s2; }
    __syncthreads();
    key = wkey[0]; s1 = red[0]; s2 = red[1];
    for (int i = 1; i < W; ++i) { key = wkey[i] < key ? wkey[i] : key; s1 += red[2 * i]; s2 += red[2 * i + 1]; }
    best = (unsigned)key; best_e = __uint_as_float((unsigned)(key >> 32));
    const double mean = s1 / (double)P, var = s2 / (double)P - mean * mean;
    converged = a.tol > 0.f && sqrt(var > 0.0 ? var : 0.0) <= (double)a.tol * fabs(mean);   // (false where an energy is not finite)
  };
  survey();
  if (tid == 0 && hist) hist[0] = sqrtf(best_e / fn);

  // ---- the generations
  int n_gen = 0;
  for (int g = 1; g <= a.maxiter && R > 0; ++g) {
    unsigned o[4];
    match_block(jid, (unsigned)g, MATCH_INIT_WORD, a.seed, o);
    const float F = 0.5f + 0.5f * ((float)(o[0] >> 8) * (1.0f / 16777216.0f));
    const float* bestrow = cur + (size_t)best * R;
    int k = 0, first = w;
    auto flush = [&]() {
      int acc = 0;
      if (lane < k) {
        const int i = first + W * lane;
        const float ef = match_residual(mine, mineG);
        acc = ef <= en[i];
        if (acc) en[i] = ef;
      }
      for (int kk = 0; kk < k; ++kk) {   // a refused trial: the member stays
        const int i = first + W * kk;
        if (!__shfl(acc, kk, 64) && lane < R) nxt[(size_t)i * R + lane] = cur[(size_t)i * R + lane];
      }
      first += W * k; k = 0;
    };
    for (int i = w; i < P; i += W) {   // wave-uniform
      match_block(jid, (unsigned)g, (unsigned)i << 6, a.seed, o);
      int r1 = (int)(o[0] % (unsigned)(P - 1)), r2 = (int)(o[1] % (unsigned)(P - 2));
      r1 += r1 >= i;
      const int lo = r1 < i ? r1 : i, hi = r1 < i ? i : r1;
      r2 += r2 >= lo; r2 += r2 >= hi;
      const int jrand = (int)(o[2] % (unsigned)R);
      if (lane < R) {
        unsigned c[4];
        match_block(jid, (unsigned)g, ((unsigned)i << 6) | (unsigned)(1 + (lane >> 2)), a.seed, c);
        const float u = ((float)(c[lane & 3] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        float v = cur[(size_t)i * R + lane];
        if (u < 0.8f || lane == jrand) v = bestrow[lane] + F * (cur[(size_t)r1 * R + lane] - cur[(size_t)r2 * R + lane]);
        if (v < -MATCH_BOUND || v > MATCH_BOUND) {
          match_block(jid, (unsigned)g, ((unsigned)i << 6) | (unsigned)(17 + (lane >> 2)), a.seed, c);
          v = match_angle(c[lane & 3]);
        }
        nxt[(size_t)i * R + lane] = v;
        ang[lane] = v;
      }
      match_eval(jb, work, ang, lane, ca, M);
      keep(k);
      if (++k == 64) flush();
    }
    flush();
    float* t = cur; cur = nxt; nxt = t;
    survey();
    n_gen = g;
    if (tid == 0 && hist) hist[g] = sqrtf(best_e / fn);
    if (converged) break;
  }
  if (tid == 0) {
    if (hist) for (int g = n_gen + 1; g <= a.maxiter; ++g) hist[g] = sqrtf(best_e / fn);
    if (a.rmsd) a.rmsd[job] = sqrtf(best_e / fn);
    if (a.n_generations) a.n_generations[job] = n_gen;
  }
  if (a.angles && tid < R) a.angles[t0 + tid] = cur[(size_t)best * R + tid];
  if (!a.pos || w != 0) return;

  // ---- the best member moved onto the target by the proper rotation and translation of its fit (wave 0)
  if (lane < R) ang[lane] = cur[(size_t)best * R + lane];
  match_eval(jb, work, ang, lane, ca, M);
  if (lane == 0) {
    double N[16], q[4], Rk[9];
    horn_key_matrix(M, N);
    max_eigvec4(N, q);
    quat_rotation(q, Rk);
    for (int i = 0; i < 9; ++i) xf[i] = Rk[i];
    for (int i = 0; i < 3; ++i) xf[9 + i] = cen[i] - (Rk[3 * i] * ca[0] + Rk[3 * i + 1] * ca[1] + Rk[3 * i + 2] * ca[2]);
  }
  DDMI_WAVE_SYNC();
  float* __restrict__ out = a.pos + 3 * (size_t)a0;
  for (int i = lane; i < n; i += 64) {
    const double x = (double)work[3 * i], y = (double)work[3 * i + 1], z = (double)work[3 * i + 2];
    for (int d = 0; d < 3; ++d) out[3 * i + d] = (float)(xf[3 * d] * x + xf[3 * d + 1] * y + xf[3 * d + 2] * z + xf[9 + d]);
  }
}

void launch_match(const MatchArgs& a, int count, bool pop_lds, size_t smem, hipStream_t s) {
  if (count <= 0) return;
  if (pop_lds) hipLaunchKernelGGL(k_match<true>, dim3(count), dim3(64 * MATCH_WAVES), smem, s, a);
  else hipLaunchKernelGGL(k_match<false>, dim3(count), dim3(64 * MATCH_WAVES), smem, s, a);
  DDMI_CHECK_HIP(hipGetLastError());
}

}  // namespace ddmi
