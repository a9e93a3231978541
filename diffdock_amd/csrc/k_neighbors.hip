// Capped neighbour lists of a ragged batch of point sets (ddmi_neighbor_graph, include/ddmi.h): the neighbour loop of
// new_extract_receptor_structure (datasets/process_mols.py:171-192 residues, :207-228 atoms) without the dense torch.cdist matrix and
// the per-row np.where / np.argsort.  For node i of set g (rows ptr[g] .. ptr[g + 1]): the other nodes of the set closer than the
// cutoff; all of them in ascending index if at most `cap`, else the cap nearest in ascending distance; the nearest other node if
// there is none.
//
// ONE WAVE owns one node and scans its set 64 candidates at a time, in two launches with an exclusive scan of the degrees between them:
//   k_neighbor_count  the in-cutoff count (lane-local counts, one wave sum) -> cnt, and the degree after the cap / fallback -> deg
//   k_neighbor_fill   the columns [offsets[i], offsets[i + 1]) of edge_index, by what cnt[i] says:
//     0           the minimum of the key (float bits of d^2 << 32 | j) over the set: non-negative floats order like their bit patterns,
//                 equal distances fall to the lower j
//     <= cap      a ballot per chunk; a hit's column is the hits before it (chunk base + lower lanes): index order, no staging
//     <= STAGE    the keys are staged in the wave's LDS list the same way, then every staged key counts the keys below it (keys are
//                 distinct: they carry j) and the ranks below cap are written at their rank: ascending (distance, index)
//     >  STAGE    the list does not hold the row: cap scans of the set, each taking the smallest in-cutoff key above the last one taken
// No atomics, no order that depends on timing; the arithmetic of a row reads nothing but its own set, so a row is bit-identical
// whatever the other sets, G and the grid are.  d^2 is (dx dx + dy dy) + dz dz with every operation rounded on its own (no fma
// contraction: the emulated build and the device agree bit for bit), from direct differences -- not |a|^2 + |b|^2 - 2 a.b, whose
// cancellation is where torch.cdist's error comes from.
#include "kernels.h"

namespace ddmi {

__device__ __forceinline__ float nbr_d2(float ax, float ay, float az, float bx, float by, float bz) {
#ifdef DDMI_HIPEMU
  volatile float dx = ax - bx, dy = ay - by, dz = az - bz;
  volatile float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  volatile float s = xx + yy;
  return s + zz;
#else
  const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
#endif
}
__device__ __forceinline__ unsigned long long nbr_wave_min(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m, 64), lo = (unsigned)__shfl_xor((int)(unsigned)v, m, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}

// the set of row i: the largest g with ptr[g] <= i (empty sets own no row and are stepped over)
struct NbrRow { int i, lo, hi; float x, y, z, c2; int cap; };
__device__ __forceinline__ NbrRow nbr_row(const NeighborArgs& a, int i) {
  int g = 0, top = a.G;
  while (top - g > 1) {
    const int mid = (g + top) >> 1;
    if (a.ptr[mid] <= i) g = mid; else top = mid;
  }
  NbrRow r;
  r.i = i; r.lo = a.ptr[g]; r.hi = a.ptr[g + 1];
  r.x = a.pos[3 * (size_t)i]; r.y = a.pos[3 * (size_t)i + 1]; r.z = a.pos[3 * (size_t)i + 2];
  r.c2 = a.c2[g]; r.cap = a.cap[g];
  return r;
}
__device__ __forceinline__ float nbr_dist(const NeighborArgs& a, const NbrRow& r, int j) {
  return nbr_d2(a.pos[3 * (size_t)j], a.pos[3 * (size_t)j + 1], a.pos[3 * (size_t)j + 2], r.x, r.y, r.z);
}
__device__ __forceinline__ unsigned long long nbr_key(float d2, int j_local) {
  return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)j_local;
}

__global__ __launch_bounds__(64 * NBR_WAVES) void k_neighbor_count(NeighborArgs a) {
  const int lane = threadIdx.x & 63, i = (int)blockIdx.x * NBR_WAVES + (int)(threadIdx.x >> 6);
  if (i >= a.N) return;   // (a whole wave)
  const NbrRow r = nbr_row(a, i);
  int c = 0;
  for (int j = r.lo + lane; j < r.hi; j += 64) c += (j != i && nbr_dist(a, r, j) < r.c2) ? 1 : 0;
  c = wave_sum_i(c);
  if (lane == 0) {
    a.cnt[i] = c;
    a.deg[i] = c > r.cap ? r.cap : (c > 0 ? c : (r.hi - r.lo > 1 ? 1 : 0));
  }
}

__device__ __forceinline__ void nbr_write(const NeighborArgs& a, long long col, int neighbour, int centre) {
  if (col < a.capacity) { a.edge[col] = neighbour; a.edge[a.capacity + col] = centre; }
}

// smem: NBR_WAVES lists of NBR_STAGE 64-bit keys
__global__ __launch_bounds__(64 * NBR_WAVES) void k_neighbor_fill(NeighborArgs a) {
  DDMI_DYN_SMEM(unsigned long long, lists);
  const int lane = threadIdx.x & 63, w = (int)(threadIdx.x >> 6), i = (int)blockIdx.x * NBR_WAVES + w;
  if (i >= a.N) return;   // (a whole wave; the kernel has no workgroup barrier)
  const NbrRow r = nbr_row(a, i);
  const int c = a.cnt[i];
  const long long off = a.offsets[i];
  if (r.hi - r.lo <= 1) return;
  const unsigned long long below = (1ull << lane) - 1ull;
  if (c == 0) {   // nobody inside the cutoff: the nearest other node
    unsigned long long best = ~0ull;
    for (int j = r.lo + lane; j < r.hi; j += 64)
      if (j != i) { const unsigned long long k = nbr_key(nbr_dist(a, r, j), j - r.lo); best = k < best ? k : best; }
    best = nbr_wave_min(best);
    if (lane == 0) nbr_write(a, off, r.lo + (int)(unsigned)best, i);
  } else if (c <= r.cap) {   // every candidate, in index order
    int base = 0;
    for (int j0 = r.lo; j0 < r.hi; j0 += 64) {   // wave-uniform trip count: every lane votes
      const int j = j0 + lane;
      const bool in = j < r.hi && j != i && nbr_dist(a, r, j) < r.c2;
      const unsigned long long mask = __ballot(in);
      if (in) nbr_write(a, off + base + __popcll(mask & below), j, i);
      base += __popcll(mask);
    }
  } else if (c <= NBR_STAGE) {   // stage the keys in index order, then rank by counting
    unsigned long long* list = lists + (size_t)w * NBR_STAGE;
    int base = 0;
    for (int j0 = r.lo; j0 < r.hi; j0 += 64) {
      const int j = j0 + lane;
      const float d2 = j < r.hi ? nbr_dist(a, r, j) : 0.f;
      const bool in = j < r.hi && j != i && d2 < r.c2;
      const unsigned long long mask = __ballot(in);
      const int slot = base + __popcll(mask & below);
      if (in && slot < NBR_STAGE) list[slot] = nbr_key(d2, j - r.lo);   // (slot < c <= NBR_STAGE: the count kernel ran the same arithmetic)
      base += __popcll(mask);
    }
    DDMI_WAVE_SYNC();
    for (int e = lane; e < c; e += 64) {
      const unsigned long long k = list[e];
      int rank = 0;
      for (int f = 0; f < c; ++f) rank += list[f] < k ? 1 : 0;
      if (rank < r.cap) nbr_write(a, off + rank, r.lo + (int)(unsigned)k, i);
    }
  } else {   // more candidates than the list holds: the smallest key above the last one taken, cap times
    unsigned long long last = 0;
    for (int t = 0; t < r.cap; ++t) {
      unsigned long long best = ~0ull;
      for (int j = r.lo + lane; j < r.hi; j += 64) {
        const float d2 = nbr_dist(a, r, j);
        if (j != i && d2 < r.c2) {
          const unsigned long long k = nbr_key(d2, j - r.lo);
          if ((t == 0 || k > last) && k < best) best = k;
        }
      }
      best = nbr_wave_min(best);
      if (lane == 0) nbr_write(a, off + t, r.lo + (int)(unsigned)best, i);
      last = best;
    }
  }
}

void launch_neighbor_count(const NeighborArgs& a, hipStream_t s) {
  if (a.N <= 0) return;
  hipLaunchKernelGGL(k_neighbor_count, dim3(cdiv(a.N, NBR_WAVES)), dim3(64 * NBR_WAVES), 0, s, a);
  DDMI_CHECK_HIP(hipGetLastError());
}
void launch_neighbor_fill(const NeighborArgs& a, hipStream_t s) {
  if (a.N <= 0) return;
  hipLaunchKernelGGL(k_neighbor_fill, dim3(cdiv(a.N, NBR_WAVES)), dim3(64 * NBR_WAVES),
                     (size_t)NBR_WAVES * NBR_STAGE * sizeof(unsigned long long), s, a);
  DDMI_CHECK_HIP(hipGetLastError());
}

}  // namespace ddmi
