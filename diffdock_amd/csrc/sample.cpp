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
  if (!c.s_ids) c.s_ids = m.cpool.alloc<long long>(c.B);
  std::copy(ids, ids + c.B, static_cast<long long*>(c.s_ids_stage.host((size_t)c.B * 8)));
  c.s_ids_stage.upload(c.s_ids, (size_t)c.B * 8, s);
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
  const size_t center_bytes = (size_t)3 * c.B * sizeof(float);   // the centres are staged as the sample ids are
  if (!c.rp_center) c.rp_center = m.cpool.alloc<float>((size_t)3 * c.B);
  std::copy(rc.center, rc.center + 3 * c.B, static_cast<float*>(c.rp_stage.host(center_bytes)));
  c.rp_stage.upload(c.rp_center, center_bytes, s);
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
