// The device calls that need no complex: pose metrics and fit (evaluate.py:474-505), capped neighbour lists (process_mols.py:171-228)
// and conformer matching (datasets/conformer_matching.py).  Each owns a grow-only scratch of the handle; the per-set / per-job tables a
// call needs on the device are checked on the host and ride through a pinned staging buffer of the handle.
#include <algorithm>
#include <string>

#include "model.h"

namespace ddmi {

// A sub-array of a staged table: the same byte offset applied to the host staging and to the device copy.
template <class T> static T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }

// The fields PoseMetricsArgs and PoseFitArgs share, with C chunks of MET_CHUNK permutations per (pose, reference).
template <class Args, class Cfg> static Args pose_args(const Cfg& c, const char* entry) {
  Args a{};
  a.pos = c.pos; a.ref = c.ref; a.perm = c.perm; a.atom_index = c.atom_index;
  a.P = c.n_poses; a.n = c.n_atoms; a.m = c.n_kept; a.K = c.n_refs; a.S = c.perm ? c.n_perms : 1;
  a.C = cdiv(a.S, MET_CHUNK);
  DDMI_REQUIRE((long)a.K * a.C <= (1L << 30), DDMI_ERR_CAPACITY, std::string(entry) + ": n_refs * ceil(n_perms / 64) exceeds 2^30");
  return a;
}

// The scratch (per (pose, reference): one 64-bit word per chunk of permutations, the identity sum, the centroid distance) belongs to
// the handle: a call that needs more than any call before it allocates; every other call enqueues two kernels and returns.
void pose_metrics(Model& m, const ddmi_pose_metrics_cfg& mc, hipStream_t s) {
  PoseMetricsArgs a = pose_args<PoseMetricsArgs>(mc, "ddmi_pose_metrics");
  a.points = mc.points; a.Q = mc.points ? mc.n_points : 0;
  const size_t pk = (size_t)a.P * a.K, key_bytes = round_up((long)(pk * a.C * sizeof(unsigned long long)), 256);
  char* ws = m.metrics_ws.reserve(key_bytes + 2 * pk * sizeof(float));
  a.part_key = at<unsigned long long>(ws, 0);
  a.part_plain = at<float>(ws, key_bytes);
  a.part_cd = a.part_plain + pk;
  a.rmsd = mc.rmsd; a.best = mc.best; a.rmsd_per_ref = mc.rmsd_per_ref; a.rmsd_plain = mc.rmsd_plain;
  a.centroid = mc.centroid_distance; a.min_self = mc.min_self_distance; a.min_point = mc.min_point_distance;
  launch_pose_metrics(a, s);
}

// ddmi_pose_fit shares the scratch of ddmi_pose_metrics (one 64-bit word per (pose, reference, chunk)): calls on one stream are ordered.
void pose_fit(Model& m, const ddmi_pose_fit_cfg& fc, hipStream_t s) {
  PoseFitArgs a = pose_args<PoseFitArgs>(fc, "ddmi_pose_fit");
  a.part_key = at<unsigned long long>(m.metrics_ws.reserve((size_t)a.P * a.K * a.C * sizeof(unsigned long long)), 0);
  a.rmsd_min = fc.rmsd_min; a.best_min = fc.best_min; a.rmsd_min_per_ref = fc.rmsd_min_per_ref;
  a.rotation = fc.rotation; a.translation = fc.translation;
  launch_pose_fit(a, s);
}

// ddmi_neighbor_graph: the per-set table (ptr, cutoff squared, cap) is staged, then count -> scan -> fill.
void neighbor_graph(Model& m, const ddmi_neighbor_graph_cfg& nc, hipStream_t s) {
  const int N = nc.n_nodes, G = nc.n_sets;
  DDMI_REQUIRE(nc.ptr[0] == 0 && nc.ptr[G] == N, DDMI_ERR_ARG, "ddmi_neighbor_graph_cfg.ptr must run from 0 to n_nodes");
  // layout of the staged table, 32-bit words: ptr [G + 1], cutoff squared [G], cap [G]
  const size_t o_c2 = ((size_t)G + 1) * 4, o_cap = o_c2 + (size_t)G * 4, tab = o_cap + (size_t)G * 4;
  void* host = m.nbr_stage.host(tab);
  int32_t *h_ptr = at<int32_t>(host, 0), *h_cap = at<int32_t>(host, o_cap);
  float* h_c2 = at<float>(host, o_c2);
  long long bound = 0;
  bool capped = true;
  for (int g = 0; g < G; ++g) {
    const long long n = (long long)nc.ptr[g + 1] - nc.ptr[g];
    DDMI_REQUIRE(n >= 0, DDMI_ERR_ARG, "ddmi_neighbor_graph_cfg.ptr decreases");
    const float c = nc.set_cutoff ? nc.set_cutoff[g] : nc.cutoff;
    DDMI_REQUIRE(c > 0.f, DDMI_ERR_ARG, "ddmi_neighbor_graph_cfg: a cutoff must be positive");   // (false for NaN)
    const int cap = nc.set_max_neighbors ? nc.set_max_neighbors[g] : nc.max_neighbors;
    DDMI_REQUIRE(cap >= 0, DDMI_ERR_ARG, "ddmi_neighbor_graph_cfg: max_neighbors must not be negative");
    capped = capped && cap > 0;
    h_ptr[g] = nc.ptr[g]; h_c2[g] = c * c; h_cap[g] = cap > 0 ? cap : 1000;
    bound += n * std::min<long long>(h_cap[g], std::max<long long>(n - 1, 0));
  }
  h_ptr[G] = N;
  DDMI_REQUIRE(bound < (1LL << 31), DDMI_ERR_CAPACITY, "ddmi_neighbor_graph: the edge bound of the call reaches 2^31");
  DDMI_REQUIRE(nc.capacity >= 0 && (!nc.edge_index || !capped || nc.capacity >= bound), DDMI_ERR_ARG,
               "ddmi_neighbor_graph_cfg.capacity is below sum n_g * min(max_neighbors, n_g - 1), the edge bound of a capped call");
  const size_t tab_bytes = round_up((long)tab, 256), row_bytes = round_up((long)(((size_t)N + 1) * sizeof(int)), 256);
  char* ws = m.nbr_ws.reserve(tab_bytes + 3 * row_bytes);
  m.nbr_stage.upload(ws, tab, s);
  NeighborArgs a{};
  a.pos = nc.pos; a.N = N; a.G = G;
  a.ptr = at<const int>(ws, 0); a.c2 = at<const float>(ws, o_c2); a.cap = at<const int>(ws, o_cap);
  a.cnt = at<int>(ws, tab_bytes);
  a.deg = nc.deg ? nc.deg : at<int>(ws, tab_bytes + row_bytes);
  int* offsets = nc.offsets ? nc.offsets : at<int>(ws, tab_bytes + 2 * row_bytes);
  a.offsets = offsets;
  a.edge = reinterpret_cast<long long*>(nc.edge_index); a.capacity = nc.capacity;
  launch_neighbor_count(a, s);
  launch_exclusive_scan(a.deg, offsets, N, s);
  if (nc.n_edges) DDMI_CHECK_HIP(hipMemcpyAsync(nc.n_edges, offsets + N, sizeof(int), hipMemcpyDeviceToDevice, s));
  if (nc.edge_index) launch_neighbor_fill(a, s);
}

// ddmi_match_conformer: the per-job tables (ptrs, mask offsets, job ids, the place of a population that does not fit LDS, the job lists
// of the two launches) are staged.  Jobs whose population fits LDS run in one launch, the others in a second one with their populations
// in the handle's scratch: the same kernel arithmetic either way.
void match_conformer(Model& m, const ddmi_match_cfg& mc, hipStream_t s) {
  const int J = mc.n_jobs;
  DDMI_REQUIRE(mc.lig_ptr[0] == 0 && mc.tor_ptr[0] == 0, DDMI_ERR_ARG, "ddmi_match_cfg: lig_ptr and tor_ptr must start at 0");
  bool torsions = false;
  for (int j = 0; j < J; ++j) {
    DDMI_REQUIRE(mc.tor_ptr[j + 1] >= mc.tor_ptr[j] && mc.lig_ptr[j + 1] >= mc.lig_ptr[j], DDMI_ERR_ARG, "ddmi_match_cfg: a ptr decreases");
    DDMI_REQUIRE(mc.lig_ptr[j + 1] > mc.lig_ptr[j], DDMI_ERR_ARG, "ddmi_match_cfg: a job of 0 atoms");
    torsions = torsions || mc.tor_ptr[j + 1] > mc.tor_ptr[j];
  }
  DDMI_REQUIRE(!torsions || (mc.rot_u && mc.rot_v && mc.mask_rotate), DDMI_ERR_ARG,
               "ddmi_match_cfg: rotatable bonds need rot_u, rot_v and mask_rotate");
  // layout of the staged tables: int lig_ptr [J + 1], tor_ptr [J + 1], list_lds [J], list_ws [J] (padded to an even count); then 64-bit
  // mask_off, job_ids, pop_off [J]
  const size_t j4 = (size_t)J * 4, j8 = (size_t)J * 8;
  const size_t o_tor = j4 + 4, o_lds = 2 * o_tor, o_ws = o_lds + j4, o_off = round_up(4 * (long)J + 2, 2) * 4, o_ids = o_off + j8, o_pop = o_ids + j8;
  const size_t tab_bytes = o_pop + j8;
  void* host = m.match_stage.host(tab_bytes);
  int32_t *h_lig = at<int32_t>(host, 0), *h_tor = at<int32_t>(host, o_tor), *h_lds = at<int32_t>(host, o_lds), *h_ws = at<int32_t>(host, o_ws);
  int64_t *h_off = at<int64_t>(host, o_off), *h_ids = at<int64_t>(host, o_ids), *h_pop = at<int64_t>(host, o_pop);
  int n_lds = 0, n_ws = 0;
  size_t smem_lds = 0, smem_ws = 0, pop_words = 0;
  int64_t mask_at = 0;
  for (int j = 0; j < J; ++j) {
    const int n = mc.lig_ptr[j + 1] - mc.lig_ptr[j], R = mc.tor_ptr[j + 1] - mc.tor_ptr[j];
    DDMI_REQUIRE(n <= MATCH_MAX_ATOMS && R <= MATCH_MAX_TORSIONS, DDMI_ERR_CAPACITY,
                 "ddmi_match_conformer: job " + std::to_string(j) + " has " + std::to_string(n) + " atoms and " + std::to_string(R) +
                     " rotatable bonds; the limits are " + std::to_string(MATCH_MAX_ATOMS) + " and " + std::to_string(MATCH_MAX_TORSIONS));
    const long P = match_population(R, mc.popsize, mc.n_init);
    DDMI_REQUIRE(P <= MATCH_MAX_POP, DDMI_ERR_CAPACITY, "ddmi_match_conformer: a population above 2^20 members");
    h_lig[j] = mc.lig_ptr[j]; h_tor[j] = mc.tor_ptr[j];
    h_off[j] = mc.mask_off ? mc.mask_off[j] : mask_at;
    mask_at += (int64_t)R * n;
    h_ids[j] = mc.job_ids ? mc.job_ids[j] : j;
    const size_t need = match_lds_bytes(n, R, P, true);
    if (need <= (size_t)MATCH_LDS_BYTES) {
      h_pop[j] = 0; h_lds[n_lds++] = j; smem_lds = std::max(smem_lds, need);
    } else {
      h_pop[j] = (int64_t)pop_words; pop_words += match_pop_words(P, R);
      h_ws[n_ws++] = j; smem_ws = std::max(smem_ws, match_lds_bytes(n, R, P, false));
    }
  }
  h_lig[J] = mc.lig_ptr[J]; h_tor[J] = mc.tor_ptr[J];
  const size_t tab_dev = round_up((long)tab_bytes, 256);
  char* ws = m.match_ws.reserve(tab_dev + pop_words * sizeof(float));
  m.match_stage.upload(ws, tab_bytes, s);
  MatchArgs a{};
  a.lig_ptr = at<const int>(ws, 0); a.tor_ptr = at<const int>(ws, o_tor);
  a.mask_off = at<const long long>(ws, o_off); a.job_ids = at<const long long>(ws, o_ids); a.pop_off = at<const long long>(ws, o_pop);
  a.start = mc.start; a.target = mc.target; a.rot_u = mc.rot_u; a.rot_v = mc.rot_v; a.mask_rotate = mc.mask_rotate;
  a.init_angles = mc.init_angles; a.n_init = mc.n_init; a.popsize = mc.popsize; a.maxiter = mc.maxiter; a.tol = mc.tol; a.seed = mc.seed;
  a.pop_ws = at<float>(ws, tab_dev);
  a.angles = mc.angles; a.rmsd = mc.rmsd; a.pos = mc.pos; a.init_energy = mc.init_energy; a.best_history = mc.best_history;
  a.n_generations = mc.n_generations;
  a.job_list = at<const int>(ws, o_lds);
  launch_match(a, n_lds, true, smem_lds, s);
  a.job_list = at<const int>(ws, o_ws);
  launch_match(a, n_ws, false, smem_ws, s);
}

}  // namespace ddmi
