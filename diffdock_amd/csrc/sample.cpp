// The reverse-diffusion loop on the device (reference sampling() utils/sampling.py:96-191): conformer update, score / noise
// combination of a step, and the step loop around forward().
#include <cmath>
#include <cstdlib>
#include <string>

#include "cx.h"

namespace ddmi {

void modify_conformer(Model& m, float* lig_pos, const float* tr, const float* rot, const float* tor, hipStream_t s,
                      float* rec_pos) {
  DDMI_REQUIRE(m.has_complex, DDMI_ERR_STATE, "ddmi_set_complex must precede ddmi_modify_conformer");
  Cx& c = *m.cx;
  if (c.layout) {
    launch_modify_conformer_ragged(lig_pos, c.B, c.maxNl, c.lig_ptr, c.tor_ptr, c.rot_lu, c.rot_lv, c.mask_off, c.mask_all, tr, rot,
                                   c.nT > 0 ? tor : nullptr, rec_pos, s);
    return;
  }
  DDMI_REQUIRE(c.uniform && c.Nl_one > 0, DDMI_ERR_STATE,
               "modify_conformer needs a batch of copies of one complex (utils/diffusion_utils.py:60-64)");
  const bool torsion = tor != nullptr && c.R_one > 0;
  DDMI_REQUIRE(!torsion || c.mask_rotate, DDMI_ERR_STATE, "mask_rotate was not provided to ddmi_set_complex");
  launch_modify_conformer(lig_pos, c.B, c.Nl_one, torsion ? c.R_one : 0, c.rot_u, c.rot_v, c.mask_rotate, tr, rot,
                          torsion ? tor : nullptr, rec_pos, s);
}

void set_sample_record(Model& m, const ddmi_sample_record* r) {
  if (!r) {
    if (m.cx) m.cx->rec_on = false;
    return;
  }
  DDMI_REQUIRE(r->struct_size == sizeof(ddmi_sample_record), DDMI_ERR_ARG, "ddmi_sample_record.struct_size does not match this library");
  DDMI_REQUIRE(r->capacity_steps >= 1, DDMI_ERR_ARG, "ddmi_sample_record.capacity_steps must be positive");
  DDMI_REQUIRE(m.has_complex, DDMI_ERR_STATE, "ddmi_set_complex must precede ddmi_set_sample_record");
  m.cx->rec = *r;
  m.cx->rec_on = true;
}

// Sample ids of the batch (keys of the counter-based generator) on the device: staged through a pinned host buffer, so
// the caller's array is consumed before this returns and nothing waits for the stream (the event only guards the reuse of
// the staging buffer by a later call).
static const long long* upload_sample_ids(Model& m, const int64_t* ids, hipStream_t s) {
  Cx& c = *m.cx;
  if (!ids) return nullptr;
  if (!c.s_ids) {
    c.s_ids = m.cpool.alloc<long long>(c.B);
    DDMI_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&c.s_ids_host), (size_t)c.B * 8));
    DDMI_CHECK_HIP(hipEventCreate(&c.s_ids_ev));
  } else {
    DDMI_CHECK_HIP(hipEventSynchronize(c.s_ids_ev));
  }
  for (int b = 0; b < c.B; ++b) c.s_ids_host[b] = ids[b];
  DDMI_CHECK_HIP(hipMemcpyAsync(c.s_ids, c.s_ids_host, (size_t)c.B * 8, hipMemcpyHostToDevice, s));
  DDMI_CHECK_HIP(hipEventRecord(c.s_ids_ev, s));
  return c.s_ids;
}

// Step k of utils/sampling.py:117-186 on score arrays (in place): NaN guard, then score and noise coefficients evaluated on
// the host in float64 exactly as the reference's 0-dim float64 tensors are.
// rec: the record whose row k receives the guarded scores and the NaN counts (the ddmi_sample loop), or nullptr.
static void perturb_step(Model& m, float* tr, float* rot, float* tor, const ddmi_sample_cfg& sc, int k,
                         const long long* ids_dev, hipStream_t s, const ddmi_sample_record* rec = nullptr) {
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int steps = sc.inference_steps, B = c.B;
  const bool torsion = tor != nullptr && !cfg.no_torsion && c.nT > 0;
  const bool last = k == steps - 1;
  const double t_tr = sc.tr_schedule[k], t_rot = sc.rot_schedule[k], t_tor = sc.tor_schedule[k];
  const double dt_tr = last ? t_tr : t_tr - sc.tr_schedule[k + 1];
  const double dt_rot = last ? t_rot : t_rot - sc.rot_schedule[k + 1];
  const double dt_tor = last ? t_tor : t_tor - sc.tor_schedule[k + 1];
  const double s_tr = std::pow((double)cfg.tr_sigma_min, 1 - t_tr) * std::pow((double)cfg.tr_sigma_max, t_tr);
  const double s_rot = std::pow((double)cfg.rot_sigma_min, 1 - t_rot) * std::pow((double)cfg.rot_sigma_max, t_rot);
  const double s_tor = std::pow((double)cfg.tor_sigma_min, 1 - t_tor) * std::pow((double)cfg.tor_sigma_max, t_tor);
  const bool zero_noise = sc.no_random || (sc.no_final_step_noise && last) || sc.ode;
  auto coeffs = [&](double sigma, double smin, double smax, double dt, int i, float& cs, float& cz) {
    const double g = sigma * std::sqrt(2.0 * std::log(smax / smin));
    double a = sc.ode ? 0.5 * g * g * dt : g * g * dt;
    double z = g * std::sqrt(dt);
    if (sc.temp_sampling[i] != 1.0) {
      const double T = sc.temp_sampling[i], psi = sc.temp_psi[i], sdat = sc.temp_sigma_data[i];
      const double sigma_data = std::exp(sdat * std::log(smax) + (1 - sdat) * std::log(smin));
      const double lambda = (sigma_data + sigma) / (sigma_data + sigma / T);
      a = g * g * dt * (lambda + T * psi / 2);
      z = g * std::sqrt(dt * (1 + psi));
    }
    cs = (float)a;
    cz = zero_noise ? 0.f : (float)z;
  };
  PerturbArgs p{};
  p.B = B; p.R = torsion ? c.nT / B : 0; p.tr = tr; p.rot = rot; p.tor = tor;
  coeffs(s_tr, cfg.tr_sigma_min, cfg.tr_sigma_max, dt_tr, 0, p.c_tr_s, p.c_tr_z);
  coeffs(s_rot, cfg.rot_sigma_min, cfg.rot_sigma_max, dt_rot, 1, p.c_rot_s, p.c_rot_z);
  coeffs(s_tor, cfg.tor_sigma_min, cfg.tor_sigma_max, dt_tor, 2, p.c_tor_s, p.c_tor_z);
  if (!zero_noise) {
    p.z_tr = sc.z_tr ? sc.z_tr + (size_t)k * B * 3 : nullptr;
    p.z_rot = sc.z_rot ? sc.z_rot + (size_t)k * B * 3 : nullptr;
    p.z_tor = sc.z_tor ? sc.z_tor + (size_t)k * c.nT : nullptr;
    p.use_rng = 1;
  }
  p.seed = sc.seed; p.sample_ids = ids_dev; p.step = k;
  if (rec) {
    if (rec->tr) p.rec_tr = rec->tr + (size_t)k * B * 3;
    if (rec->rot) p.rec_rot = rec->rot + (size_t)k * B * 3;
    if (rec->tor && torsion) p.rec_tor = rec->tor + (size_t)k * c.nT;
    if (rec->nan_count) p.rec_nan = rec->nan_count + (size_t)k * (c.layout ? c.G : 1);
  }
  if (c.layout) launch_perturb_grouped(p, c.G, c.grp_ptr, c.tor_ptr, c.tor_batch, s);
  else launch_perturb(p, s);
}

static void check_sample_cfg(Model& m, const ddmi_sample_cfg& sc) {
  DDMI_REQUIRE(sc.inference_steps > 0 && sc.tr_schedule && sc.rot_schedule && sc.tor_schedule, DDMI_ERR_ARG, "bad schedule");
  DDMI_REQUIRE(m.cx->uniform || m.cx->layout, DDMI_ERR_STATE,
               "the step loop needs a batch of copies of one complex, or ddmi_set_batch_layout for a batch of several");
}

void perturb(Model& m, float* tr, float* rot, float* tor, const ddmi_sample_cfg& sc, int k, hipStream_t s) {
  DDMI_REQUIRE(m.has_complex, DDMI_ERR_STATE, "ddmi_set_complex must precede ddmi_perturb");
  check_sample_cfg(m, sc);
  DDMI_REQUIRE(k >= 0 && k < sc.inference_steps, DDMI_ERR_ARG, "step index out of range");
  perturb_step(m, tr, rot, tor, sc, k, upload_sample_ids(m, sc.sample_ids, s), s);
}

void randomize_position(Model& m, float* lig_pos, const ddmi_randomize_cfg& rc, hipStream_t s) {
  DDMI_REQUIRE(m.has_complex, DDMI_ERR_STATE, "ddmi_set_complex must precede ddmi_randomize_position");
  Cx& c = *m.cx;
  DDMI_REQUIRE(c.layout || (c.uniform && c.Nl_one > 0), DDMI_ERR_STATE,
               "randomize_position needs a batch of copies of one complex, or ddmi_set_batch_layout for a batch of several");
  const bool torsion = !rc.no_torsion && c.nT > 0;
  DDMI_REQUIRE(!torsion || (c.layout ? c.mask_all != nullptr : c.mask_rotate != nullptr), DDMI_ERR_STATE,
               "the batch has rotatable bonds and mask_rotate was not provided to ddmi_set_complex");
  // the centres ride through a pinned staging buffer as the sample ids do: consumed before this returns, nothing waits for the stream
  if (!c.rp_center) {
    c.rp_center = m.cpool.alloc<float>((size_t)3 * c.B);
    DDMI_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&c.rp_center_host), (size_t)3 * c.B * sizeof(float)));
    DDMI_CHECK_HIP(hipEventCreate(&c.rp_ev));
  } else {
    DDMI_CHECK_HIP(hipEventSynchronize(c.rp_ev));
  }
  for (int i = 0; i < 3 * c.B; ++i) c.rp_center_host[i] = rc.center[i];
  DDMI_CHECK_HIP(hipMemcpyAsync(c.rp_center, c.rp_center_host, (size_t)3 * c.B * sizeof(float), hipMemcpyHostToDevice, s));
  DDMI_CHECK_HIP(hipEventRecord(c.rp_ev, s));
  RandomizeArgs a{};
  a.pos = lig_pos; a.B = c.B;
  if (c.layout) {
    a.lig_ptr = c.lig_ptr; a.tor_ptr = c.tor_ptr; a.rot_u = c.rot_lu; a.rot_v = c.rot_lv; a.mask_off = c.mask_off; a.mask_rotate = c.mask_all;
  } else {
    a.Nl = c.Nl_one; a.R = c.R_one; a.rot_u = c.rot_u; a.rot_v = c.rot_v; a.mask_rotate = c.mask_rotate;
  }
  a.rec_ptr = c.rec_ptr; a.rec_pos = c.rec_pos; a.center = c.rp_center;
  a.no_torsion = !torsion; a.no_random = rc.no_random != 0; a.choose_residue = rc.choose_residue != 0; a.tr_std = rc.tr_std;
  a.seed = rc.seed; a.sample_ids = upload_sample_ids(m, rc.sample_ids, s);
  a.tor_updates = rc.tor_updates; a.rotations = rc.rotations; a.tr_updates = rc.tr_updates;
  launch_randomize_position(a, c.layout ? c.maxNl : c.Nl_one, s);
}

// The scratch (per (pose, reference): one 64-bit word per chunk of permutations, the identity sum, the centroid distance) belongs to
// the handle and only grows: a call that needs more than any call before it allocates (hipFree waits for the device, so kernels of an
// earlier call still in flight keep their memory); every other call enqueues two kernels and returns.
static void metrics_scratch(Model& m, size_t bytes) {
  if (bytes <= m.metrics_ws_bytes) return;
  m.mpool.release();
  m.metrics_ws = nullptr; m.metrics_ws_bytes = 0;
  m.metrics_ws = m.mpool.alloc_bytes(bytes);
  m.metrics_ws_bytes = bytes;
}

void pose_metrics(Model& m, const ddmi_pose_metrics_cfg& mc, hipStream_t s) {
  PoseMetricsArgs a{};
  a.pos = mc.pos; a.ref = mc.ref; a.perm = mc.perm; a.atom_index = mc.atom_index; a.points = mc.points;
  a.P = mc.n_poses; a.n = mc.n_atoms; a.m = mc.n_kept; a.K = mc.n_refs; a.S = mc.perm ? mc.n_perms : 1; a.Q = mc.points ? mc.n_points : 0;
  a.C = cdiv(a.S, MET_CHUNK);
  DDMI_REQUIRE((long)a.K * a.C <= (1L << 30), DDMI_ERR_CAPACITY, "ddmi_pose_metrics: n_refs * ceil(n_perms / 64) exceeds 2^30");
  const size_t pk = (size_t)a.P * a.K, key_bytes = round_up((long)(pk * a.C * sizeof(unsigned long long)), 256);
  const size_t bytes = key_bytes + 2 * pk * sizeof(float);
  metrics_scratch(m, bytes);
  a.part_key = reinterpret_cast<unsigned long long*>(m.metrics_ws);
  a.part_plain = reinterpret_cast<float*>(reinterpret_cast<char*>(m.metrics_ws) + key_bytes);
  a.part_cd = a.part_plain + pk;
  a.rmsd = mc.rmsd; a.best = mc.best; a.rmsd_per_ref = mc.rmsd_per_ref; a.rmsd_plain = mc.rmsd_plain;
  a.centroid = mc.centroid_distance; a.min_self = mc.min_self_distance; a.min_point = mc.min_point_distance;
  launch_pose_metrics(a, s);
}

// ddmi_pose_fit shares the scratch of ddmi_pose_metrics (one 64-bit word per (pose, reference, chunk)): calls on one stream are ordered.
void pose_fit(Model& m, const ddmi_pose_fit_cfg& fc, hipStream_t s) {
  PoseFitArgs a{};
  a.pos = fc.pos; a.ref = fc.ref; a.perm = fc.perm; a.atom_index = fc.atom_index;
  a.P = fc.n_poses; a.n = fc.n_atoms; a.m = fc.n_kept; a.K = fc.n_refs; a.S = fc.perm ? fc.n_perms : 1;
  a.C = cdiv(a.S, MET_CHUNK);
  DDMI_REQUIRE((long)a.K * a.C <= (1L << 30), DDMI_ERR_CAPACITY, "ddmi_pose_fit: n_refs * ceil(n_perms / 64) exceeds 2^30");
  metrics_scratch(m, (size_t)a.P * a.K * a.C * sizeof(unsigned long long));
  a.part_key = reinterpret_cast<unsigned long long*>(m.metrics_ws);
  a.rmsd_min = fc.rmsd_min; a.best_min = fc.best_min; a.rmsd_min_per_ref = fc.rmsd_min_per_ref;
  a.rotation = fc.rotation; a.translation = fc.translation;
  launch_pose_fit(a, s);
}

// ddmi_neighbor_graph: the per-set table (ptr, cutoff squared, cap) is checked on the host and rides through a pinned staging buffer as
// the centres of randomize_position do -- consumed before this returns, nothing waits for the stream; then count -> scan -> fill.
void neighbor_graph(Model& m, const ddmi_neighbor_graph_cfg& nc, hipStream_t s) {
  const int N = nc.n_nodes, G = nc.n_sets;
  DDMI_REQUIRE(nc.ptr[0] == 0 && nc.ptr[G] == N, DDMI_ERR_ARG, "ddmi_neighbor_graph_cfg.ptr must run from 0 to n_nodes");
  const size_t words = 3 * (size_t)G + 1;
  if (words > m.nbr_host_words) {
    if (m.nbr_ev) DDMI_CHECK_HIP(hipEventSynchronize(m.nbr_ev));
    else DDMI_CHECK_HIP(hipEventCreate(&m.nbr_ev));
    if (m.nbr_host) { (void)hipHostFree(m.nbr_host); m.nbr_host = nullptr; m.nbr_host_words = 0; }
    DDMI_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&m.nbr_host), words * sizeof(int32_t)));
    m.nbr_host_words = words;
  } else {
    DDMI_CHECK_HIP(hipEventSynchronize(m.nbr_ev));
  }
  int32_t* h_ptr = m.nbr_host;
  float* h_c2 = reinterpret_cast<float*>(m.nbr_host + G + 1);
  int32_t* h_cap = m.nbr_host + 2 * (size_t)G + 1;
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
  const size_t tab_bytes = round_up((long)(words * sizeof(int32_t)), 256), row_bytes = round_up((long)(((size_t)N + 1) * sizeof(int)), 256);
  const size_t bytes = tab_bytes + 3 * row_bytes;
  if (bytes > m.nbr_ws_bytes) {   // (hipFree waits for the device: kernels of an earlier call keep their memory)
    m.npool.release();
    m.nbr_ws = nullptr; m.nbr_ws_bytes = 0;
    m.nbr_ws = m.npool.alloc_bytes(bytes);
    m.nbr_ws_bytes = bytes;
  }
  char* ws = reinterpret_cast<char*>(m.nbr_ws);
  DDMI_CHECK_HIP(hipMemcpyAsync(ws, m.nbr_host, words * sizeof(int32_t), hipMemcpyHostToDevice, s));
  DDMI_CHECK_HIP(hipEventRecord(m.nbr_ev, s));
  NeighborArgs a{};
  a.pos = nc.pos; a.N = N; a.G = G;
  a.ptr = reinterpret_cast<const int*>(ws);
  a.c2 = reinterpret_cast<const float*>(ws) + G + 1;
  a.cap = reinterpret_cast<const int*>(ws) + 2 * (size_t)G + 1;
  a.cnt = reinterpret_cast<int*>(ws + tab_bytes);
  a.deg = nc.deg ? nc.deg : reinterpret_cast<int*>(ws + tab_bytes + row_bytes);
  int* offsets = nc.offsets ? nc.offsets : reinterpret_cast<int*>(ws + tab_bytes + 2 * row_bytes);
  a.offsets = offsets;
  a.edge = reinterpret_cast<long long*>(nc.edge_index); a.capacity = nc.capacity;
  launch_neighbor_count(a, s);
  launch_exclusive_scan(a.deg, offsets, N, s);
  if (nc.n_edges) DDMI_CHECK_HIP(hipMemcpyAsync(nc.n_edges, offsets + N, sizeof(int), hipMemcpyDeviceToDevice, s));
  if (nc.edge_index) launch_neighbor_fill(a, s);
}

// ddmi_match_conformer: the per-job tables (ptrs, mask offsets, job ids, the place of a population that does not fit LDS, the job lists
// of the two launches) are checked on the host and ride through a pinned staging buffer as the table of neighbor_graph does -- consumed
// before this returns, nothing waits for the stream.  Jobs whose population fits LDS run in one launch, the others in a second one with
// their populations in the handle's scratch: the same kernel arithmetic either way.
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
  // layout of the staged tables: int lig_ptr [J + 1], tor_ptr [J + 1], list_lds [J], list_ws [J]; then 64-bit mask_off, job_ids, pop_off [J]
  const size_t ints = round_up(4 * (size_t)J + 2, 2), tab_bytes = ints * sizeof(int32_t) + 3 * (size_t)J * sizeof(int64_t);
  if (tab_bytes > m.match_host_bytes) {
    if (m.match_ev) DDMI_CHECK_HIP(hipEventSynchronize(m.match_ev));
    else DDMI_CHECK_HIP(hipEventCreate(&m.match_ev));
    if (m.match_host) { (void)hipHostFree(m.match_host); m.match_host = nullptr; m.match_host_bytes = 0; }
    DDMI_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&m.match_host), tab_bytes));
    m.match_host_bytes = tab_bytes;
  } else {
    DDMI_CHECK_HIP(hipEventSynchronize(m.match_ev));
  }
  int32_t* h_lig = reinterpret_cast<int32_t*>(m.match_host);
  int32_t *h_tor = h_lig + J + 1, *h_lds = h_tor + J + 1, *h_ws = h_lds + J;
  int64_t* h_off = reinterpret_cast<int64_t*>(m.match_host + ints * sizeof(int32_t));
  int64_t *h_ids = h_off + J, *h_pop = h_ids + J;
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
  const size_t tab_dev = round_up((long)tab_bytes, 256), bytes = tab_dev + pop_words * sizeof(float);
  if (bytes > m.match_ws_bytes) {   // (hipFree waits for the device: kernels of an earlier call keep their memory)
    m.xpool.release();
    m.match_ws = nullptr; m.match_ws_bytes = 0;
    m.match_ws = m.xpool.alloc_bytes(bytes);
    m.match_ws_bytes = bytes;
  }
  char* ws = reinterpret_cast<char*>(m.match_ws);
  DDMI_CHECK_HIP(hipMemcpyAsync(ws, m.match_host, tab_bytes, hipMemcpyHostToDevice, s));
  DDMI_CHECK_HIP(hipEventRecord(m.match_ev, s));
  MatchArgs a{};
  a.lig_ptr = reinterpret_cast<const int*>(ws); a.tor_ptr = a.lig_ptr + J + 1;
  a.mask_off = reinterpret_cast<const long long*>(ws + ints * sizeof(int32_t)); a.job_ids = a.mask_off + J; a.pop_off = a.job_ids + J;
  a.start = mc.start; a.target = mc.target; a.rot_u = mc.rot_u; a.rot_v = mc.rot_v; a.mask_rotate = mc.mask_rotate;
  a.init_angles = mc.init_angles; a.n_init = mc.n_init; a.popsize = mc.popsize; a.maxiter = mc.maxiter; a.tol = mc.tol; a.seed = mc.seed;
  a.pop_ws = reinterpret_cast<float*>(ws + tab_dev);
  a.angles = mc.angles; a.rmsd = mc.rmsd; a.pos = mc.pos; a.init_energy = mc.init_energy; a.best_history = mc.best_history;
  a.n_generations = mc.n_generations;
  a.job_list = a.tor_ptr + J + 1;
  launch_match(a, n_lds, true, smem_lds, s);
  a.job_list += J;
  launch_match(a, n_ws, false, smem_ws, s);
}

void sample(Model& m, float* lig_pos, const ddmi_sample_cfg& sc, hipStream_t s) {
  DDMI_REQUIRE(m.has_complex, DDMI_ERR_STATE, "ddmi_set_complex must precede ddmi_sample");
  check_sample_cfg(m, sc);
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int steps = sc.inference_steps, B = c.B;
  const bool torsion = !cfg.no_torsion && c.nT > 0;
  const ddmi_sample_record* rec = c.rec_on ? &c.rec : nullptr;
  DDMI_REQUIRE(!rec || rec->capacity_steps >= steps, DDMI_ERR_ARG,
               "ddmi_sample_record.capacity_steps = " + std::to_string(rec ? rec->capacity_steps : 0) + " < inference_steps = " + std::to_string(steps));
  struct CropGuard {   // the per-step crop must not outlive the loop, also when a step throws
    Model& m; double saved;
    ~CropGuard() { m.crop_cutoff = saved; }
  } crop_guard{m, m.crop_cutoff};
  if (!c.s_t) c.s_t = m.cpool.alloc<float>((size_t)3 * B * STEP_TIMES_MAX);
  const long long* ids_dev = upload_sample_ids(m, sc.sample_ids, s);
  const bool times_once = steps <= STEP_TIMES_MAX;   // set_time of every step in ONE launch in front of the loop (one launch less per forward)
  if (times_once) {
    StepTimes st{};
    st.steps = steps;
    for (int k = 0; k < steps; ++k) { st.t[3 * k] = (float)sc.tr_schedule[k]; st.t[3 * k + 1] = (float)sc.rot_schedule[k]; st.t[3 * k + 2] = (float)sc.tor_schedule[k]; }
    launch_fill_times_all(c.s_t, B, st, s);
  }
  for (int k = 0; k < steps; ++k) {
    const double t_tr = sc.tr_schedule[k], t_rot = sc.rot_schedule[k], t_tor = sc.tor_schedule[k];
    const double s_tr = std::pow((double)cfg.tr_sigma_min, 1 - t_tr) * std::pow((double)cfg.tr_sigma_max, t_tr);
    float* tk = times_once ? c.s_t + (size_t)k * 3 * B : c.s_t;
    if (!times_once) launch_fill_times(tk, B, (float)t_tr, (float)t_rot, (float)t_tor, s);   // set_time for this step
    m.crop_cutoff = sc.use_crop ? s_tr * 3.0 + sc.crop_beyond : 0.0;   // sampling.py:107
    // (Measured and dropped in round 4, profiles/r04_e7_ab.txt: the forward captured once as a HIP graph -- every launch argument
    // of a forward is the same in every step -- and replayed per step.  A dependent-kernel boundary costs the same inside a graph
    // as between eager launches on this stack, and the replay's fixed cost is not hidden: 146.3 -> 145.4 poses/s at 40 poses,
    // 102.2 -> 100.5 at 5.)
    {
      struct UniformT {   // every graph of the step has the same t (fill_times above): forward may share pose-invariant work
        Model& m;
        explicit UniformT(Model& mm) : m(mm) { m.uniform_t = true; }
        ~UniformT() { m.uniform_t = false; }
      } uniform_t{m};
      forward(m, lig_pos, tk, tk + B, tk + 2 * B, c.s_tr, c.s_rot, torsion ? c.s_tor : nullptr, s);
    }
    perturb_step(m, c.s_tr, c.s_rot, torsion ? c.s_tor : nullptr, sc, k, ids_dev, s, rec);
#ifdef DDMI_PROFILING   // timing-only ablation builds produce garbage scores: DDMI_FREEZE_POSE keeps the graphs fixed (never in the shipped library)
    static const bool freeze = getenv("DDMI_FREEZE_POSE") != nullptr;
#else
    constexpr bool freeze = false;
#endif
    if (!freeze) modify_conformer(m, lig_pos, c.s_tr, c.s_rot, torsion ? c.s_tor : nullptr, s,
                                  rec && rec->pos ? rec->pos + (size_t)k * c.nL * 3 : nullptr);
  }
  c.x_last = nullptr;   // ddmi_sidechain_pred belongs to the ddmi_forward it follows: the loop's tables are not an answer to it
}

}  // namespace ddmi
