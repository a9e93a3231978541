// extern "C" surface of libddmi.so (include/ddmi.h).
#include <cstdlib>
#include <cstring>

#include "model.h"

using namespace ddmi;

struct ddmi_model { Model m; };

static thread_local std::string g_err;

template <class F> static int guard(F&& f) {
  try { f(); return DDMI_OK; }
  catch (const Error& e) { g_err = e.what(); return e.code; }
  catch (const std::exception& e) { g_err = e.what(); return DDMI_ERR_ARG; }
}

// Execution options (include/ddmi.h, ddmi_exec_options): 0 = default everywhere; the library reads no environment variable.
Routes ddmi::resolve_routes(const ddmi_config& cfg, int n_cus) {
  static const struct { const char* name; int32_t ddmi_exec_options::*field; int max; } ranges[] = {
      {"streams", &ddmi_exec_options::streams, 1}, {"dense_rows", &ddmi_exec_options::dense_rows, 2},
      {"shared_tiles", &ddmi_exec_options::shared_tiles, 2}, {"packed_granules", &ddmi_exec_options::packed_granules, 1},
      {"merged_granule", &ddmi_exec_options::merged_granule, 1}, {"pre_reduce", &ddmi_exec_options::pre_reduce, 1},
      {"hidden_mm", &ddmi_exec_options::hidden_mm, 1}, {"fc1_batch", &ddmi_exec_options::fc1_batch, 1},
      {"tile_split", &ddmi_exec_options::tile_split, 8}, {"tile_split_small", &ddmi_exec_options::tile_split_small, 8},
      {"hidden_grid", &ddmi_exec_options::hidden_grid, 1 << 20}, {"tp_apply", &ddmi_exec_options::tp_apply, 3},
      {"tile_per_pose", &ddmi_exec_options::tile_per_pose, 1}, {"layer_overlap", &ddmi_exec_options::layer_overlap, 2},
      {"grouped", &ddmi_exec_options::grouped, 2}, {"grouped_split", &ddmi_exec_options::grouped_split, 8},
      {"vn_build", &ddmi_exec_options::vn_build, 1}, {"node_update", &ddmi_exec_options::node_update, 3},
      {"tile_split_last", &ddmi_exec_options::tile_split_last, 8}, {"tile_split_rule", &ddmi_exec_options::tile_split_rule, 2},
      {"group_order", &ddmi_exec_options::group_order, 3}, {"list_caps", &ddmi_exec_options::list_caps, 1},
      {"time_terms", &ddmi_exec_options::time_terms, 1}, {"rec_share", &ddmi_exec_options::rec_share, 1}};
  const ddmi_exec_options& x = cfg.exec;
  DDMI_REQUIRE(cfg.edge_product >= 0 && cfg.edge_product <= 1, DDMI_ERR_ARG, "ddmi_config.edge_product: 0 (f32) or 1 (bf16x4)");
  for (auto& q : ranges)
    DDMI_REQUIRE(x.*q.field >= 0 && x.*q.field <= q.max, DDMI_ERR_ARG, std::string("ddmi_config.exec.") + q.name + ": out of range");
  auto use = [](int v) { return v == 0 ? Use::by_rule : v == 1 ? Use::never : Use::always; };
  Routes r;
  r.two_streams = x.streams == 0;
  r.layer_overlap = x.layer_overlap;
  r.shared_tiles = use(x.shared_tiles); r.dense_rows = use(x.dense_rows);
  r.merged_granule = x.merged_granule == 0; r.packed_granules = x.packed_granules == 0;
  r.tp_form = x.tp_apply - 1;
  r.fc1_batch = x.fc1_batch == 0; r.hidden_mm = x.hidden_mm == 0; r.pre_reduce = x.pre_reduce == 0;
  r.tile_split = x.tile_split; r.tile_split_small = x.tile_split_small; r.tile_split_last = x.tile_split_last;
  r.round_split = x.tile_split_rule != 1; r.round_split_small = x.tile_split_rule == 2;
  r.list_caps = x.list_caps == 1; r.time_terms = x.time_terms == 1;
  r.group_order = x.group_order;
  r.n_cus = n_cus;
  if (x.hidden_grid > 0) r.hidden_grid = x.hidden_grid;
  r.grouped = x.grouped; r.grouped_split = x.grouped_split;
  r.node_update = x.node_update >= 1;
  r.node_update_wpn = x.node_update == 2 ? 1 : x.node_update == 3 ? 4 : 0;
  r.vn_merge = x.vn_build == 0;
  r.tile_per_pose = x.tile_per_pose != 0;
  r.rec_share = x.rec_share == 0;
  return r;
}

// The prologue of the cfg-taking entry points: null check, the size of a struct that carries one (name = its type), the handle's device.
static Model& enter(ddmi_model* h, bool args_ok) {
  DDMI_REQUIRE(h && args_ok, DDMI_ERR_ARG, "null argument");
  DDMI_CHECK_HIP(hipSetDevice(h->m.device));
  return h->m;
}
template <class Cfg> static Model& enter(ddmi_model* h, const Cfg* cfg, const char* name, bool args_ok = true) {
  DDMI_REQUIRE(h && cfg && args_ok, DDMI_ERR_ARG, "null argument");
  DDMI_REQUIRE(cfg->struct_size == sizeof(Cfg), DDMI_ERR_ARG, std::string(name) + ".struct_size does not match this library");
  return enter(h, true);
}
// the checks ddmi_pose_metrics_cfg and ddmi_pose_fit_cfg share
template <class Cfg> static void check_pose_cfg(const Cfg& c, const std::string& name) {
  DDMI_REQUIRE(c.pos && c.ref, DDMI_ERR_ARG, name + ": pos and ref are required");
  DDMI_REQUIRE(c.n_poses > 0 && c.n_atoms > 0 && c.n_kept > 0 && c.n_refs > 0, DDMI_ERR_ARG, name + ": n_poses, n_atoms, n_kept and n_refs must be positive");
  DDMI_REQUIRE(c.n_kept <= c.n_atoms, DDMI_ERR_ARG, name + ": n_kept > n_atoms");
  DDMI_REQUIRE(c.atom_index || c.n_kept == c.n_atoms, DDMI_ERR_ARG, name + ": without atom_index n_kept must equal n_atoms");
  DDMI_REQUIRE(!c.perm || c.n_perms >= 1, DDMI_ERR_ARG, name + ": perm given with n_perms < 1");
}

extern "C" {

const char* ddmi_last_error(void) { return g_err.c_str(); }

int ddmi_create(const ddmi_config* cfg, int device, ddmi_model** out) {
  return guard([&] {
    DDMI_REQUIRE(cfg && out, DDMI_ERR_ARG, "null argument");
    DDMI_REQUIRE(cfg->struct_size == sizeof(ddmi_config), DDMI_ERR_ARG,
                 "ddmi_config.struct_size != sizeof(ddmi_config) of this library: the caller was built against another include/ddmi.h");
    DDMI_CHECK_HIP(hipSetDevice(device));
    std::unique_ptr<ddmi_model> h(new ddmi_model());
    h->m.cfg = *cfg;
    h->m.device = device;
    build_weight_spec(h->m);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 16) cus = Routes().n_cus;
    h->m.r = resolve_routes(h->m.cfg, cus);
    DDMI_CHECK_HIP(hipStreamCreateWithFlags(&h->m.side_stream, hipStreamNonBlocking));
    DDMI_CHECK_HIP(hipEventCreate(&h->m.ev_fork));
    DDMI_CHECK_HIP(hipEventCreate(&h->m.ev_join));
    DDMI_CHECK_HIP(hipEventCreate(&h->m.ev_cross));
    DDMI_CHECK_HIP(hipEventCreate(&h->m.ev_terms));
    *out = h.release();
  });
}

void ddmi_destroy(ddmi_model* h) {
  if (!h) return;
  Model& m = h->m;
  if (m.side_stream) { (void)hipStreamSynchronize(m.side_stream); (void)hipStreamDestroy(m.side_stream); }
  for (hipEvent_t e : {m.ev_fork, m.ev_join, m.ev_cross, m.ev_terms}) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : m.ev_pipe) (void)hipEventDestroy(e);
  delete h;
}

int ddmi_num_weights(ddmi_model* h) { return h ? (int)h->m.spec.size() : DDMI_ERR_ARG; }

int ddmi_weight_spec(ddmi_model* h, int i, const char** key, int64_t shape[4], int* ndim) {
  return guard([&] {
    DDMI_REQUIRE(h && i >= 0 && i < (int)h->m.spec.size(), DDMI_ERR_ARG, "bad index");
    *key = h->m.spec[i].first.c_str();
    *ndim = (int)h->m.spec[i].second.size();
    for (int d = 0; d < *ndim; ++d) shape[d] = h->m.spec[i].second[d];
  });
}

int ddmi_set_weight(ddmi_model* h, const char* key, const float* data, const int64_t* shape, int ndim) {
  return guard([&] {
    DDMI_REQUIRE(h && key && shape && ndim >= 1 && ndim <= 4, DDMI_ERR_ARG, "bad argument");
    int64_t numel = 1;
    for (int d = 0; d < ndim; ++d) numel *= shape[d];
    DDMI_REQUIRE(data || numel == 0, DDMI_ERR_ARG, "null data");
    Model& m = h->m;
    bool known = false;
    for (auto& kv : m.spec) if (kv.first == key) {
      known = true;
      DDMI_REQUIRE((int)kv.second.size() == ndim && std::equal(shape, shape + ndim, kv.second.begin()), DDMI_ERR_KEY,
                   std::string("shape mismatch for ") + key);
    }
    DDMI_REQUIRE(known, DDMI_ERR_KEY, std::string("unexpected state_dict key: ") + key);
    HostTensor t;
    t.shape.assign(shape, shape + ndim);
    if (numel) t.data.assign(data, data + numel);
    m.host_w[key] = std::move(t);
    m.committed = false;
  });
}

int ddmi_commit_weights(ddmi_model* h) {
  return guard([&] { DDMI_REQUIRE(h, DDMI_ERR_ARG, "null model"); DDMI_CHECK_HIP(hipSetDevice(h->m.device)); commit_weights(h->m); });
}

int ddmi_set_table(ddmi_model* h, int kind, const double* data, int64_t n) {
  return guard([&] {
    DDMI_REQUIRE(h && data && n > 1 && (kind == 0 || kind == 1), DDMI_ERR_ARG, "bad table");
    DDMI_CHECK_HIP(hipSetDevice(h->m.device));
    std::vector<float> f(data, data + n);  // the reference casts the looked-up values with .float()
    float* p = h->m.tpool.upload(f);
    if (kind == 0) { h->m.so3_table = p; h->m.so3_n = (int)n; }
    else { h->m.torus_table = p; h->m.torus_n = (int)n; }
  });
}

int ddmi_set_time_frequencies(ddmi_model* h, const float* freq, int64_t n) {
  return guard([&] {
    DDMI_REQUIRE(h && freq && n == h->m.cfg.sigma_embed_dim / 2, DDMI_ERR_ARG, "need sigma_embed_dim/2 frequencies");
    DDMI_REQUIRE(!h->m.committed, DDMI_ERR_STATE, "set frequencies before ddmi_commit_weights");
    h->m.time_freq_host.assign(freq, freq + n);
  });
}

int ddmi_set_complex(ddmi_model* h, const ddmi_complex* c, ddmi_stream s) {
  return guard([&] {
    Model& m = enter(h, c != nullptr);
    set_complex(m, *c, (hipStream_t)s);
  });
}

int ddmi_set_batch_layout(ddmi_model* h, const ddmi_batch_layout* l, ddmi_stream s) {
  return guard([&] {
    Model& m = enter(h, l != nullptr);
    set_batch_layout(m, *l, (hipStream_t)s);
  });
}

int ddmi_forward(ddmi_model* h, const float* lig_pos, const float* t_tr, const float* t_rot, const float* t_tor,
                 float* tr_out, float* rot_out, float* tor_out, ddmi_stream s) {
  return guard([&] {
    DDMI_REQUIRE(h && lig_pos && t_tr && t_rot && t_tor && tr_out && rot_out, DDMI_ERR_ARG, "null argument");
    DDMI_REQUIRE(!h->m.cfg.confidence_mode, DDMI_ERR_STATE, "confidence models are evaluated with ddmi_confidence");
    DDMI_CHECK_HIP(hipSetDevice(h->m.device));
    forward(h->m, lig_pos, t_tr, t_rot, t_tor, tr_out, rot_out, tor_out, (hipStream_t)s);
  });
}

int ddmi_sidechain_pred(ddmi_model* h, float* out, ddmi_stream s) {
  return guard([&] {
    DDMI_REQUIRE(h && out, DDMI_ERR_ARG, "null argument");
    DDMI_REQUIRE(h->m.cfg.sidechain_pred, DDMI_ERR_STATE, "ddmi_sidechain_pred needs a model created with sidechain_pred");
    DDMI_CHECK_HIP(hipSetDevice(h->m.device));
    sidechain_pred(h->m, out, (hipStream_t)s);
  });
}

int ddmi_confidence(ddmi_model* h, const float* lig_pos, const float* t_tr, const float* t_rot, const float* t_tor,
                    float* conf_out, float* atom_conf_out, ddmi_stream s) {
  return guard([&] {
    DDMI_REQUIRE(h && lig_pos && t_tr && t_rot && t_tor && conf_out, DDMI_ERR_ARG, "null argument");
    DDMI_REQUIRE(h->m.cfg.confidence_mode, DDMI_ERR_STATE, "ddmi_confidence needs a model created with confidence_mode");
    DDMI_REQUIRE(!h->m.cfg.atom_confidence || atom_conf_out, DDMI_ERR_ARG, "atom_confidence models need atom_conf_out");
    DDMI_CHECK_HIP(hipSetDevice(h->m.device));
    forward(h->m, lig_pos, t_tr, t_rot, t_tor, nullptr, nullptr, nullptr, (hipStream_t)s, conf_out, atom_conf_out);
  });
}

int ddmi_set_crop_cutoff(ddmi_model* h, float cutoff) {
  if (!h) return DDMI_ERR_ARG;
  h->m.crop_cutoff = cutoff > 0.f ? cutoff : 0.f;
  return DDMI_OK;
}

int ddmi_modify_conformer(ddmi_model* h, float* lig_pos, const float* tr, const float* rot, const float* tor, ddmi_stream s) {
  return guard([&] {
    DDMI_REQUIRE(h && lig_pos && tr && rot, DDMI_ERR_ARG, "null argument");
    DDMI_CHECK_HIP(hipSetDevice(h->m.device));
    modify_conformer(h->m, lig_pos, tr, rot, tor, (hipStream_t)s);
  });
}

int ddmi_sample(ddmi_model* h, float* lig_pos, const ddmi_sample_cfg* cfg, ddmi_stream s) {
  return guard([&] {
    Model& m = enter(h, lig_pos && cfg);
    sample(m, lig_pos, *cfg, (hipStream_t)s);
  });
}

int ddmi_randomize_position(ddmi_model* h, float* lig_pos, const ddmi_randomize_cfg* cfg, ddmi_stream s) {
  return guard([&] {
    Model& m = enter(h, cfg, "ddmi_randomize_cfg", lig_pos != nullptr);
    DDMI_REQUIRE(cfg->center, DDMI_ERR_ARG, "ddmi_randomize_cfg.center is required");
    randomize_position(m, lig_pos, *cfg, (hipStream_t)s);
  });
}

int ddmi_pose_metrics(ddmi_model* h, const ddmi_pose_metrics_cfg* cfg, ddmi_stream s) {
  return guard([&] {
    Model& m = enter(h, cfg, "ddmi_pose_metrics_cfg");
    check_pose_cfg(*cfg, "ddmi_pose_metrics_cfg");
    DDMI_REQUIRE(!cfg->points || cfg->n_points >= 1, DDMI_ERR_ARG, "ddmi_pose_metrics_cfg: points given with n_points < 1");
    pose_metrics(m, *cfg, (hipStream_t)s);
  });
}

int ddmi_pose_fit(ddmi_model* h, const ddmi_pose_fit_cfg* cfg, ddmi_stream s) {
  return guard([&] {
    Model& m = enter(h, cfg, "ddmi_pose_fit_cfg");
    check_pose_cfg(*cfg, "ddmi_pose_fit_cfg");
    pose_fit(m, *cfg, (hipStream_t)s);
  });
}

int ddmi_neighbor_graph(ddmi_model* h, const ddmi_neighbor_graph_cfg* cfg, ddmi_stream s) {
  return guard([&] {
    Model& m = enter(h, cfg, "ddmi_neighbor_graph_cfg");
    DDMI_REQUIRE(cfg->pos && cfg->ptr, DDMI_ERR_ARG, "ddmi_neighbor_graph_cfg: pos and ptr are required");
    DDMI_REQUIRE(cfg->n_nodes > 0 && cfg->n_sets > 0, DDMI_ERR_ARG, "ddmi_neighbor_graph_cfg: n_nodes and n_sets must be positive");
    neighbor_graph(m, *cfg, (hipStream_t)s);
  });
}

int ddmi_match_conformer(ddmi_model* h, const ddmi_match_cfg* cfg, ddmi_stream s) {
  return guard([&] {
    Model& m = enter(h, cfg, "ddmi_match_cfg");
    DDMI_REQUIRE(cfg->start && cfg->target && cfg->lig_ptr && cfg->tor_ptr, DDMI_ERR_ARG,
                 "ddmi_match_cfg: start, target, lig_ptr and tor_ptr are required");
    DDMI_REQUIRE(cfg->n_jobs >= 1, DDMI_ERR_ARG, "ddmi_match_cfg: n_jobs must be positive");
    DDMI_REQUIRE(cfg->popsize >= 1 && cfg->maxiter >= 0, DDMI_ERR_ARG, "ddmi_match_cfg: popsize must be positive and maxiter not negative");
    DDMI_REQUIRE(cfg->tol >= 0.f, DDMI_ERR_ARG, "ddmi_match_cfg: tol must not be negative");   // (false for NaN)
    DDMI_REQUIRE(cfg->n_init >= 0 && (cfg->n_init == 0 || cfg->init_angles || cfg->tor_ptr[cfg->n_jobs] == 0), DDMI_ERR_ARG,
                 "ddmi_match_cfg: n_init must not be negative, and n_init > 0 needs init_angles");
    match_conformer(m, *cfg, (hipStream_t)s);
  });
}

int ddmi_set_sample_record(ddmi_model* h, const ddmi_sample_record* r) {
  return guard([&] {
    DDMI_REQUIRE(h, DDMI_ERR_ARG, "null model");
    set_sample_record(h->m, r);
  });
}

int ddmi_perturb(ddmi_model* h, float* tr, float* rot, float* tor, const ddmi_sample_cfg* cfg, int step, ddmi_stream s) {
  return guard([&] {
    Model& m = enter(h, tr && rot && cfg);
    perturb(m, tr, rot, tor, *cfg, step, (hipStream_t)s);
  });
}

int ddmi_debug_shape(ddmi_model* h, const char* name, int64_t shape[4], int* ndim, int* is_int) {
  return guard([&] {
    DDMI_REQUIRE(h && name, DDMI_ERR_ARG, "null argument");
    auto it = h->m.debug.find(name);
    DDMI_REQUIRE(it != h->m.debug.end(), DDMI_ERR_KEY, std::string("unknown debug buffer: ") + name);
    *ndim = (int)it->second.shape.size();
    for (int d = 0; d < *ndim && d < 4; ++d) shape[d] = it->second.shape[d];
    *is_int = it->second.is_int;
  });
}

int ddmi_debug_read(ddmi_model* h, const char* name, void* dst, size_t bytes, ddmi_stream s) {
  return guard([&] {
    DDMI_REQUIRE(h && name && dst, DDMI_ERR_ARG, "null argument");
    auto it = h->m.debug.find(name);
    DDMI_REQUIRE(it != h->m.debug.end(), DDMI_ERR_KEY, std::string("unknown debug buffer: ") + name);
    size_t n = 4;
    for (auto d : it->second.shape) n *= (size_t)d;
    DDMI_REQUIRE(bytes <= n, DDMI_ERR_ARG, "read past the end of the buffer");
    DDMI_CHECK_HIP(hipStreamSynchronize((hipStream_t)s));
    DDMI_CHECK_HIP(hipMemcpy(dst, it->second.ptr, bytes, hipMemcpyDeviceToHost));
  });
}

int ddmi_wigner_3j(int l1, int l2, int l3, double* out) {
  return guard([&] {
    DDMI_REQUIRE(out && l1 >= 0 && l2 >= 0 && l3 >= std::abs(l1 - l2) && l3 <= l1 + l2, DDMI_ERR_ARG, "bad l");
    auto w = wigner_3j(l1, l2, l3);
    std::memcpy(out, w.data(), w.size() * sizeof(double));
  });
}

int ddmi_debug_philox(const uint32_t* counters, const uint32_t* keys, int n, uint32_t* host_out) {
  return guard([&] {
    DDMI_REQUIRE(counters && keys && host_out && n > 0, DDMI_ERR_ARG, "null argument");
    struct Buf {   // freed on every exit path, also when a later call throws
      unsigned* p = nullptr;
      explicit Buf(size_t bytes) { DDMI_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&p), bytes)); }
      ~Buf() { if (p) (void)hipFree(p); }
    };
    Buf c((size_t)n * 16), k((size_t)n * 8), o((size_t)n * 16);
    hipStream_t st = nullptr;
    DDMI_CHECK_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamDestroy(s); } } sg{st};
    DDMI_CHECK_HIP(hipMemcpyAsync(c.p, counters, (size_t)n * 16, hipMemcpyHostToDevice, st));
    DDMI_CHECK_HIP(hipMemcpyAsync(k.p, keys, (size_t)n * 8, hipMemcpyHostToDevice, st));
    launch_debug_philox(c.p, k.p, n, o.p, st);
    DDMI_CHECK_HIP(hipMemcpyAsync(host_out, o.p, (size_t)n * 16, hipMemcpyDeviceToHost, st));
    DDMI_CHECK_HIP(hipStreamSynchronize(st));
  });
}

int ddmi_debug_normal(uint64_t seed, int64_t sample0, int n_samples, int step, int n_comp, float* dev_out, ddmi_stream s) {
  return guard([&] {
    DDMI_REQUIRE(dev_out && n_samples > 0 && n_comp > 0, DDMI_ERR_ARG, "bad argument");
    launch_debug_normal(seed, sample0, n_samples, step, n_comp, dev_out, (hipStream_t)s);
  });
}

int ddmi_debug_reduce_bn_sum(int n_groups, int n_nodes, int d_in, int d_out, const int32_t* toff, const float* msg, const float* bn_mean,
                             const float* bn_scale, const float* bn_bias, const float* x_in, float* x_out, float* ref_out, ddmi_stream s) {
  return guard([&] {
    DDMI_REQUIRE(n_groups >= 1 && n_groups <= REDUCE_SUM_MAX && n_nodes > 0 && d_in >= 0 && d_in <= d_out && d_out <= XS, DDMI_ERR_ARG,
                 "bad sizes");
    DDMI_REQUIRE(toff && msg && bn_mean && bn_scale && bn_bias && x_in && x_out, DDMI_ERR_ARG, "null argument");
    DDMI_REQUIRE(!ref_out || n_groups == 1, DDMI_ERR_ARG, "ref_out: one group only");
    ReduceSumArgs a{};
    a.n_groups = n_groups;
    for (int g = 0; g < n_groups; ++g)
      a.g[g] = ReduceSumGroup{toff + (size_t)g * (n_nodes + 1), msg, bn_mean + (size_t)g * d_out, bn_scale + (size_t)g * d_out,
                              bn_bias + (size_t)g * d_out};
    a.nbase = 0; a.ncount = n_nodes; a.D_in = d_in; a.D_out = d_out; a.X_in = x_in; a.X_out = x_out;
    launch_reduce_bn_sum(a, (hipStream_t)s);
    if (!ref_out) return;
    struct Buf {   // freed on every exit path
      ReduceGroup* p = nullptr;
      Buf() { DDMI_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&p), sizeof(ReduceGroup))); }
      ~Buf() { if (p) (void)hipFree(p); }
    } rg;
    const ReduceGroup g0{toff, msg, 0, n_nodes};
    DDMI_CHECK_HIP(hipMemcpyAsync(rg.p, &g0, sizeof(g0), hipMemcpyHostToDevice, (hipStream_t)s));
    launch_reduce_bn(rg.p, 1, 0, n_nodes, d_in, d_out, bn_mean, bn_scale, bn_bias, 1, x_in, ref_out, XS, (hipStream_t)s);
    DDMI_CHECK_HIP(hipStreamSynchronize((hipStream_t)s));
  });
}

int ddmi_set_kernel_timing(ddmi_model* h, int enabled) {
  if (!h) return DDMI_ERR_ARG;
  resolve_timings(h->m);
#if defined(DDMI_PROFILING)
  (void)hipDeviceSynchronize();
  ddmi::fc_prof_report();   // in-kernel phase clocks / workgroup stamps since the last call (profiling builds only)
#endif
  h->m.timing = enabled != 0;
  h->m.timing_level = enabled;
  if (enabled) h->m.phases.clear();
  return DDMI_OK;
}
int ddmi_kernel_timings(ddmi_model* h, int i, const char** name, double* ms, int64_t* launches) {
  if (!h) return DDMI_ERR_ARG;
  resolve_timings(h->m);
  if (i < 0 || i >= (int)h->m.phases.size()) return DDMI_ERR_ARG;
  *name = h->m.phases[i].name.c_str(); *ms = h->m.phases[i].ms; *launches = h->m.phases[i].launches;
  return DDMI_OK;
}

}  // extern "C"
