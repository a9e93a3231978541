// The score-model forward pass for one collated batch (reference CGModel.forward models/cg_model.py:308-424, the all-atom and
// legacy classes next to it): time terms, node tables, graphs, the interaction layers (conv_layers.cpp) and the read-outs.
// Everything is enqueued on the caller's stream.  Also the kernel-timing brackets (ddmi_set_kernel_timing).
#include <memory>
#include <string>

#include "cx.h"

namespace ddmi {

static hipEvent_t get_event(Model& m) {
  if (!m.free_events.empty()) { hipEvent_t e = m.free_events.back(); m.free_events.pop_back(); return e; }
  hipEvent_t e;
  DDMI_CHECK_HIP(hipEventCreate(&e));
  return e;
}
PhaseTimer::PhaseTimer(Model& model, const char* name, hipStream_t stream) : m(model), s(stream) {
  if (!m.timing) return;
  for (size_t i = 0; i < m.phases.size(); ++i) if (m.phases[i].name == name) idx = (int)i;
  if (idx < 0) { m.phases.push_back({name, 0.0, 0}); idx = (int)m.phases.size() - 1; }
  a = get_event(m); b = get_event(m);
  (void)hipEventRecord(a, s);
}
PhaseTimer::~PhaseTimer() {
  if (idx < 0) return;
  (void)hipEventRecord(b, s);
  m.pending.push_back({idx, a, b});
}
void resolve_timings(Model& m) {
  for (auto& p : m.pending) {
    (void)hipEventSynchronize(p.b);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { m.phases[p.phase].ms += ms; m.phases[p.phase].launches++; }
    m.free_events.push_back(p.a); m.free_events.push_back(p.b);
  }
  m.pending.clear();
}

// Score read-outs on the final ligand rows XL (cg_model.py:368-423 = old_cg_model.py:293-352): centre convolution ->
// translation / rotation heads, torsion-bond convolution -> torsion head.
static void score_readouts(Model& m, const float* XL, const float* lig_pos, const float* t_tr, const float* t_rot,
                           const float* t_tor, float* tr_out, float* rot_out, float* tor_out, hipStream_t s) {
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int ns = m.ns, sd = m.sd, B = c.B, nL = c.nL;
  if (m.r.two_streams && m.side_stream && c.nT > 0 && tor_out) {   // the torsion head below forks here
    DDMI_CHECK_HIP(hipEventRecord(m.ev_fork, s));
    DDMI_CHECK_HIP(hipStreamWaitEvent(m.side_stream, m.ev_fork, 0));
  }
  // ---- translation / rotation heads (cg_model.py:368-395)
  const ConvW& F = m.final_conv;
  // (round 6: centre vectors + harmonics + the node scalars of the attribute row in ONE launch, the edge MLP writes its ns columns
  // straight into the attribute row: 4 launches instead of 7 in front of the GEMMs)
  // fixed_center_conv: scalars of the atom; otherwise the reference indexes the ligand table by GRAPH id (cg_model.py:371-374)
  launch_center_prep(lig_pos, c.lig_batch, c.lig_ptr, nL, cfg.sh_lmax, XL, cfg.fixed_center_conv ? c.c_xrow : c.lig_batch, ns, c.c_dist,
                     c.c_nvec, c.c_sh, F.sh_dim, c.c_attr, F.n_edge, s);
  {
    EdgeMlpArgs ea = mlp_args(m.center_edge, ns, nL, nullptr, c.c_dist, m.off_center, m.D, m.coeff_center, 0, c.center_gvec, c.lig_batch, c.c_attr);
    ea.ldo = F.n_edge;
    launch_edge_mlp(ea, s);
  }
  run_direct_conv(m, F, c.c_attr, nL, c.c_hid, c.c_W, c.c_xrow, XL, c.c_sh, nullptr, nullptr, 0, c.c_out, s);
  launch_segment_mean_bn(c.c_out, F.D_out, c.lig_ptr, nullptr, 0, B, F.D_out, bn_args(F).mean, bn_args(F).scale, bn_args(F).bias, c.gp, F.D_out, s);
  {
    ScoreHeadArgs a{};
    a.B = B; a.gp = c.gp; a.odd_parity = cfg.odd_parity; a.scale_by_sigma = cfg.scale_by_sigma; a.ns = ns; a.ldw0 = 1 + sd;
    a.tr_w0n = m.tr_final.W0; a.tr_sig = c.tr_sig; a.tr_w3 = m.tr_final.W3; a.tr_b3 = m.tr_final.b3;
    a.rot_w0n = m.rot_final.W0; a.rot_sig = c.rot_sig; a.rot_w3 = m.rot_final.W3; a.rot_b3 = m.rot_final.b3;
    a.t_tr = t_tr; a.t_rot = t_rot; a.tr_smin = cfg.tr_sigma_min; a.tr_smax = cfg.tr_sigma_max;
    a.rot_smin = cfg.rot_sigma_min; a.rot_smax = cfg.rot_sigma_max; a.so3_table = m.so3_table; a.so3_n = m.so3_n;
    a.tr_out = tr_out; a.rot_out = rot_out;
    launch_score_heads(a, s);
  }
  // ---- torsion head (cg_model.py:404-423); independent of the translation / rotation heads: with two streams it runs on the
  // side stream next to them (both chains are ~10 small launches on an otherwise idle chip)
  if (c.nT > 0 && tor_out) {
    const ConvW& T = m.tor_conv;
    const hipStream_t s_main = s;
    const bool fork = m.r.two_streams && m.side_stream;
    if (fork) s = m.side_stream;
    launch_tor_radius(lig_pos, c.lig_ptr, c.tor_u, c.tor_v, c.tor_batch, c.nT, cfg.lig_max_radius, c.tor_cap,
                      cfg.smooth_edges ? cfg.lig_max_radius : 0.f, c.t_cnt, c.t_atom, c.t_dist, c.t_nvec, c.t_ew, c.t_bond_nvec, s);
    {   // (round 6: edge MLP straight into the attribute rows; the two node-scalar column blocks + the bond harmonics in one launch)
      EdgeMlpArgs ea = mlp_args(m.final_edge, ns, c.Et, nullptr, c.t_dist, m.off_lig, m.D, m.coeff_lig, 0, m.final_edge.b0, nullptr, c.t_attr);
      ea.ldo = T.n_edge;
      launch_edge_mlp(ea, s);
    }
    launch_tor_prep(c.t_nvec, c.t_bond_nvec, c.nT, c.tor_cap, cfg.sh_lmax, m.tor_T, m.tor_ds, m.tor_dts, c.t_sh, XL, c.t_atom, c.tor_eu,
                    c.tor_ev, ns, c.t_attr, T.n_edge, s);
    run_direct_conv(m, T, c.t_attr, c.Et, c.t_hid, c.t_W, c.t_atom, XL, c.t_sh, c.t_ew, c.t_cnt, c.tor_cap, c.t_out, s);
    launch_segment_mean_bn(c.t_out, T.D_out, nullptr, c.t_cnt, c.tor_cap, c.nT, T.D_out, bn_args(T).mean, bn_args(T).scale, bn_args(T).bias, c.t_feat, T.D_out, s);
    TorHeadArgs a{};
    a.nT = c.nT; a.ns = ns; a.in_dim = T.D_out; a.feat = c.t_feat; a.W0 = m.tor_W0; a.W3 = m.tor_W3;
    a.tor_batch = c.tor_batch; a.t_tor = t_tor; a.smin = cfg.tor_sigma_min; a.smax = cfg.tor_sigma_max;
    a.scale_by_sigma = cfg.scale_by_sigma; a.torus_table = m.torus_table; a.torus_n = m.torus_n; a.out = tor_out;
    launch_tor_head(a, s);
    if (fork) {
      DDMI_CHECK_HIP(hipEventRecord(m.ev_join, m.side_stream));
      DDMI_CHECK_HIP(hipStreamWaitEvent(s_main, m.ev_join, 0));
    }
  }
}

// ---- ligand graph (bonds + radius graph) and its edge attributes
static void lig_graph(Model& m, const float* lig_pos, hipStream_t s) {
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int ns = m.ns, sd = m.sd, nL = c.nL;
  launch_lig_radius(lig_pos, c.lig_batch, c.lig_ptr, nL, c.maxNl, cfg.lig_max_radius, c.lig_cap, c.adjrank, c.cnt_g, s);
  launch_ll_count(c.adjrank, c.lig_batch, c.lig_ptr, nL, c.maxNl, c.bg, c.bt, c.cnt_g, c.cnt_t, s);
  launch_exclusive_scan2(c.cnt_g, c.goff_ll, nL, c.cnt_t, c.toff_ll, nL, s);
  launch_ll_fill(lig_pos, c.lig_batch, c.lig_ptr, nL, c.maxNl, c.adjrank, c.goff_ll, c.toff_ll, c.bg, c.bt, c.Eb, c.bond_src,
                 c.bond_dst, c.bond_grank, c.bond_trank, cfg.smooth_edges ? cfg.lig_max_radius : 0.f, c.ll_tgt, c.ll_tslot,
                 c.ll_featidx, c.ll_batch, c.ll_dist, c.ll_nvec, c.ll_ew, s);
  {
    EdgeMlpArgs a = mlp_args(m.lig_edge, ns, c.Ell_cap, c.goff_ll + nL, c.ll_dist, m.off_lig, m.D, m.coeff_lig, m.nf + sd,
                             c.ll_gvec, c.ll_batch, c.ll_ea);
    a.feat = c.bond_attr; a.featidx = c.ll_featidx; a.nfeat = m.nf; a.W0f = m.lig_edge.W0; a.ldw0f = m.lig_edge.in;
    launch_edge_mlp(a, s);
  }
}

// ============================================================ legacy class, confidence mode
// models/old_cg_model.py:203-291 (CGOldModel.forward with confidence_mode): four separate OldTensorProductConvLayers per
// interaction layer, each = fc + tensor product + its own mean + BatchNorm (tensor_layers.py:338-380), summed onto the
// zero-padded node features.
static void forward_old(Model& m, const float* lig_pos, const float* t_tr, const float* t_rot, const float* t_tor, float* tr_out,
                        float* rot_out, float* tor_out, float* conf_out, hipStream_t s) {
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int ns = m.ns, sd = m.sd, B = c.B, nL = c.nL, nR = c.nR, Lc = cfg.num_conv_layers;
  ++c.epoch;
  PhaseTimer t_fwd(m, "forward_total", s);
  std::unique_ptr<PhaseTimer> t_phase(new PhaseTimer(m, "embed_and_graphs", s));
  launch_time_embedding(t_tr, B, m.time_freq, sd / 2, cfg.embedding_scale, cfg.embedding_type, c.temb, s);
  // OldAtomEncoder: ligand = sum of embeddings + linear(sigma) ; receptor = static part + the sigma columns of lm_embedding_layer
  gemm(c.temb, sd, m.old_lig_lin.W0, sd, m.old_lig_lin.b0, c.ligsig, ns, B, ns, sd, 0, s);
  if (m.lm > 0) gemm(c.temb, sd, m.old_lm_W + ns + m.lm - sd, ns + m.lm, nullptr, c.rec_sig, ns, B, ns, sd, 0, s);
  else gemm(c.temb, sd, m.old_rec_lin.W0, sd, m.old_rec_lin.b0, c.rec_sig, ns, B, ns, sd, 0, s);
  gemm(c.temb, sd, m.lig_edge.W0 + m.nf, m.lig_edge.in, m.lig_edge.b0, c.ll_gvec, ns, B, ns, sd, 0, s);
  gemm(c.temb, sd, m.cross_edge.W0, m.cross_edge.in, m.cross_edge.b0, c.cross_gvec, ns, B, ns, sd, 0, s);
  gemm(c.temb, sd, m.rec_edge.W0, m.rec_edge.in, m.rec_edge.b0, c.rr_sig_old, ns, B, ns, sd, 0, s);   // receptor-edge sigma term
  const bool conf = cfg.confidence_mode != 0;
  if (!conf) {   // sigma terms of the read-outs (old_cg_model.py:294-296,313-315)
    gemm(c.temb, sd, m.center_edge.W0 + m.D, m.center_edge.in, m.center_edge.b0, c.center_gvec, ns, B, ns, sd, 0, s);
    gemm(c.temb, sd, m.tr_final.W0 + 1, 1 + sd, m.tr_final.b0, c.tr_sig, ns, B, ns, sd, 0, s);
    gemm(c.temb, sd, m.rot_final.W0 + 1, 1 + sd, m.rot_final.b0, c.rot_sig, ns, B, ns, sd, 0, s);
  }
  float* X0 = c.X[0];
  launch_lig_node_embed(c.lig_x, nL, m.lig_emb, m.lig_emb_off, 16, ns, c.embsum, s);
  launch_add_rowvec(X0, XS, c.embsum, ns, c.ligsig, ns, c.lig_batch, nL, ns, ns, s);
  launch_add_rowvec(X0 + (size_t)nL * XS, XS, c.rec_node_base, XS, c.rec_sig, ns, c.rec_batch, nR, ns, ns, s);
  // ligand graph, receptor edge attributes (with sigma, old_cg_model.py:411-413), cross graph with the raw-t cutoff
  lig_graph(m, lig_pos, s);
  launch_edge_mlp(mlp_args(m.rec_edge, ns, c.Err, nullptr, c.rr_dist, m.off_rec, m.D, m.coeff_rec, sd, c.rr_sig_old, c.rr_batch,
                           c.rec_edge_base), s);
  const float* cut_dev = nullptr;
  if (cfg.dynamic_max_cross) {
    // confidence mode feeds the raw t as sigma (old_cg_model.py:207-210), score mode t_to_sigma(t)
    launch_cross_cutoff(t_tr, B, cfg.tr_sigma_min, cfg.tr_sigma_max, c.cutoff, s, conf ? 1 : 0);
    cut_dev = c.cutoff;
  }
  launch_cross_count(lig_pos, c.rec_pos, c.lig_batch, c.rec_batch, c.lig_ptr, c.rec_ptr, nL, nR, c.maxNr, cut_dev,
                     cfg.cross_max_distance, nullptr, c.pairrank, c.cnt_l, c.cnt_r, s);
  launch_exclusive_scan2(c.cnt_l, c.offs_l, nL, c.cnt_r, c.offs_r, nR, s);
  launch_cross_fill(lig_pos, c.rec_pos, c.rec_batch, c.lig_ptr, c.rec_ptr, nL, nR, c.maxNr, c.pairrank, c.offs_l, c.offs_r,
                    cut_dev, cfg.cross_max_distance, cfg.smooth_edges, c.g1_tgt, c.g1_tslot, c.g3_tgt, c.g3_tslot, c.pbatch,
                    c.pdist, c.pnvec, c.pew, s);
  launch_edge_mlp(mlp_args(m.cross_edge, ns, c.Elr_cap, c.offs_l + nL, c.pdist, m.off_cross, m.Dc, m.coeff_cross, sd,
                           c.cross_gvec, c.pbatch, c.cross_ea), s);
  RunGroup g_ll{0, nL, 0, nL, c.goff_ll, c.ll_tgt, c.ll_tslot, nullptr, c.ll_ea, c.Ell_cap, c.goff_ll + nL, nullptr,
                nullptr, c.ll_nvec, c.ll_ew, 1.f, c.msg[0]};
  RunGroup g_lr{nL, nR, 0, nL, c.offs_r, c.g1_tgt, c.g1_tslot, c.g1_tslot, c.cross_ea, c.Elr_cap, c.offs_l + nL, nullptr,
                nullptr, c.pnvec, c.pew, 1.f, c.msg[1]};
  RunGroup g_rr{nL, nR, nL, nR, c.rr_goff, c.rr_tgt, c.rr_tslot, c.rr_arow, c.rec_edge_base, c.Err, nullptr, nullptr, nullptr,
                c.rr_nvec, c.rr_ew, 1.f, c.msg[2]};
  RunGroup g_rl{0, nL, nL, nR, c.offs_l, c.g3_tgt, c.g3_tslot, nullptr, c.cross_ea, c.Elr_cap, c.offs_l + nL, nullptr,
                nullptr, c.pnvec, c.pew, 1.f, c.msg[3]};   // same spherical harmonics as rec->lig (old_cg_model.py:264)
  g_ll.vn = 2; g_ll.load = true; g_lr.vn = 0; g_rr.vn = 1; g_rl.vn = 3; g_rl.load = true; g_rl.swap_pq = true;
  float *Ua = c.X[Lc + 1], *Ub = c.X[Lc + 2];
  t_phase.reset();
  for (int l = 0; l < Lc; ++l) {
    const bool last = l == Lc - 1;
    const float* Xin = c.X[l];
    run_conv(m, m.old_lig[l], {g_ll}, c.rg_all + 0, 1, Xin, Ua, 0, nL, s);
    run_conv(m, m.old_r2l[l], {g_lr}, c.rg_all + 1, 1, Xin, Ub, 0, nL, s);
    if (!last) {
      run_conv(m, m.old_rec[l], {g_rr}, c.rg_all + 2, 1, Xin, Ua, nL, nR, s);
      run_conv(m, m.old_l2r[l], {g_rl}, c.rg_all + 3, 1, Xin, Ub, nL, nR, s);
    }
    const ConvW& L = m.old_lig[l];
    PhaseTimer t(m, "k_reduce_bn", s);
    launch_add3(c.X[l + 1], Xin, L.D_in, Ua, Ub, last ? nL : nL + nR, L.D_out, s);
  }
  PhaseTimer t_read(m, "readouts", s);
  if (!conf) {
    score_readouts(m, c.X[Lc], lig_pos, t_tr, t_rot, t_tor, tr_out, rot_out, tor_out, s);
    return;
  }
  ConfHeadArgs a{};
  a.B = B; a.X = c.X[Lc]; a.ldx = XS; a.col0 = 0; a.lig_ptr = c.lig_ptr; a.ns = ns;
  a.n_tail = Lc >= 3 ? ns : 0;
  a.tail_off = m.old_lig[Lc - 1].D_out - a.n_tail;
  a.W0 = m.conf_W[0]; a.b0 = m.conf_b[0]; a.sc0 = m.conf_bn_scale[0]; a.sh0 = m.conf_bn_shift[0];
  a.W1 = m.conf_W[1]; a.b1 = m.conf_b[1]; a.sc1 = m.conf_bn_scale[1]; a.sh1 = m.conf_bn_shift[1];
  a.W2 = m.conf_W[2]; a.b2 = m.conf_b[2]; a.n_out = cfg.affinity_prediction ? 2 : 1; a.out = conf_out;   // old_cg_model.py:154
  launch_conf_head(a, s);
}

// ---- per-graph time terms: the hidden layer of rec_sigma and one [B][ns] vector per consumer of the time embedding, all linear in
// it.  One list, emitted as k_time_terms (exec.time_terms: embedding, terms and rec_sigma's second layer in one launch) or as the
// embedding, one batched GEMM launch and rec_sigma's second layer.
static void time_terms(Model& m, const float* t_tr, bool conf, hipStream_t s) {
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int ns = m.ns, sd = m.sd, B = c.B;
  struct Term { const float* W; int ldw; const float* bias; float* C; int act; };
  const Term terms[] = {{m.rec_sigma.W0, sd, m.rec_sigma.b0, c.hidB, 1},
                        {m.lig_enc.W0 + ns, ns + sd, m.lig_enc.b0, c.ligsig, 0},
                        {m.lig_edge.W0 + m.nf, m.lig_edge.in, m.lig_edge.b0, c.ll_gvec, 0},
                        {m.cross_edge.W0, m.cross_edge.in, m.cross_edge.b0, c.cross_gvec, 0},
                        // score models only: sigma terms of the read-outs
                        {m.center_edge.W0 + m.D, m.center_edge.in, m.center_edge.b0, c.center_gvec, 0},
                        {m.tr_final.W0 + 1, 1 + sd, m.tr_final.b0, c.tr_sig, 0},
                        {m.rot_final.W0 + 1, 1 + sd, m.rot_final.b0, c.rot_sig, 0}};
  const int n = conf ? 4 : 7;
  if (m.r.time_terms && sd / 2 <= 128 && ns <= 128) {
    TimeTermsArgs ta{};
    ta.t = t_tr; ta.B = B; ta.freq = m.time_freq; ta.half = sd / 2; ta.scale = cfg.embedding_scale; ta.fourier = cfg.embedding_type; ta.temb = c.temb;
    ta.ns = ns;
    for (const Term& q : terms) {
      if (ta.n == n) break;
      auto& x = ta.term[ta.n++];
      x.W = q.W; x.ldw = q.ldw; x.bias = q.bias; x.C = q.C; x.act = q.act;
    }
    ta.hid_term = 0; ta.W3 = m.rec_sigma.W3; ta.b3 = m.rec_sigma.b3; ta.out3 = c.rec_sig;
    launch_time_terms(ta, s);
    return;
  }
  launch_time_embedding(t_tr, B, m.time_freq, sd / 2, cfg.embedding_scale, cfg.embedding_type, c.temb, s);
  GemmBatch gb;
  for (const Term& q : terms) {
    if (gb.n == n) break;
    GemmArgs& x = gb.g[gb.n++];
    x.A = c.temb; x.lda = sd; x.W = q.W; x.ldw = q.ldw; x.bias = q.bias; x.C = q.C; x.ldc = ns; x.M = B; x.N = ns; x.K = sd; x.act = q.act;
  }
  launch_gemm_batch(gb, s);
  gemm(c.hidB, ns, m.rec_sigma.W3, ns, m.rec_sigma.b3, c.rec_sig, ns, B, ns, ns, 0, s);
}

// a static atom relation as an edge group reads it: the per-complex CSR, or its compaction of this forward under a crop
struct Rel { const int *goff, *tgt, *tslot, *arow; };
static Rel rel_of(const Cx::StaticEdges& e, bool crop) {
  return crop ? Rel{e.goff2, e.tgt2, e.tslot2, e.arow2} : Rel{e.goff, e.tgt, e.tslot, e.arow};
}

// ---- all-atom model (aa_model.py:364-436): atom rows (atom_rows: their embedding without the sigma term), ligand<->atom radius
// graph, nine edge groups.  crop: the atoms of the cropped residues are gone too (utils/utils.py:393-411) -- masked out of the radius
// graph, the static atom relations read through their compaction (forward); g_rr comes in cropped already.
static void run_aa_layers(Model& m, const float* lig_pos, const RunGroup& g_ll, const RunGroup& g_lr, const RunGroup& g_rr,
                          const RunGroup& g_rl, bool crop, const float* atom_rows, int& xi, std::unique_ptr<PhaseTimer>& t_phase,
                          hipStream_t s) {
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int ns = m.ns, sd = m.sd, B = c.B, nL = c.nL, nR = c.nR, Lc = (int)m.conv_layers.size();
  const int nA = c.nA, aB = nL + nR;
  launch_add_rowvec(c.X[xi] + (size_t)aB * XS, XS, atom_rows, XS, c.rec_sig, ns, c.atom_batch, nA, c.rec_base_dim, ns, s);
  launch_cross_count(lig_pos, c.atom_pos, c.lig_batch, c.atom_batch, c.lig_ptr, c.atom_ptr, nL, nA, c.maxNa, nullptr,
                     cfg.lig_max_radius, crop ? c.keep_atom : nullptr, c.la_pairrank, c.la_cnt_l, c.la_cnt_a, s);
  launch_exclusive_scan2(c.la_cnt_l, c.la_offs_l, nL, c.la_cnt_a, c.la_offs_a, nA, s);
  launch_cross_fill(lig_pos, c.atom_pos, c.atom_batch, c.lig_ptr, c.atom_ptr, nL, nA, c.maxNa, c.la_pairrank, c.la_offs_l,
                    c.la_offs_a, nullptr, cfg.lig_max_radius, cfg.smooth_edges, c.la1_tgt, c.la1_tslot, c.la3_tgt, c.la3_tslot,
                    c.la_pbatch, c.la_dist, c.la_nvec, c.la_ew, s, aB);
  gemm(c.temb, sd, m.la_edge.W0, m.la_edge.in, m.la_edge.b0, c.la_gvec, ns, B, ns, sd, 0, s);
  launch_edge_mlp(mlp_args(m.la_edge, ns, c.Ela_cap, c.la_offs_l + nL, c.la_dist, m.off_lig, m.D, m.coeff_lig, sd, c.la_gvec,
                           c.la_pbatch, c.la_ea), s);
  // groups in the reference's order [ll, lr, la, rr, rl, ra, aa, al, ar]; the flipped groups reuse the forward
  // spherical harmonics (aa_model.py:411-412), so every group has sgn = +1
  RunGroup a_ll = g_ll, a_lr = g_lr, a_rr = g_rr, a_rl = g_rl;
  a_rl.sgn = 1.f;
  a_ll.msg = c.msg_aa[0]; a_lr.msg = c.msg_aa[1]; a_rr.msg = c.msg_aa[3]; a_rl.msg = c.msg_aa[4];
  RunGroup a_la{aB, nA, 0, nL, c.la_offs_a, c.la1_tgt, c.la1_tslot, c.la1_tslot, c.la_ea, c.Ela_cap, c.la_offs_l + nL, nullptr,
                nullptr, c.la_nvec, c.la_ew, 1.f, c.msg_aa[2]};
  const Rel ra = rel_of(c.se_ra, crop), aa = rel_of(c.se_aa, crop), ar = rel_of(c.se_ar, crop);
  RunGroup a_ra{aB, nA, nL, nR, ra.goff, ra.tgt, ra.tslot, ra.arow, c.ar_edge_base, c.Ear, nullptr, c.rec_sig,
                c.ar_batch, c.ar_nvec, nullptr, 1.f, c.msg_aa[5]};
  RunGroup a_aa{aB, nA, aB, nA, aa.goff, aa.tgt, aa.tslot, aa.arow, c.atom_edge_base, c.Eaa, nullptr, c.rec_sig,
                c.aa_batch, c.aa_nvec, c.aa_ew, 1.f, c.msg_aa[6]};
  RunGroup a_al{0, nL, aB, nA, c.la_offs_l, c.la3_tgt, c.la3_tslot, nullptr, c.la_ea, c.Ela_cap, c.la_offs_l + nL, nullptr,
                nullptr, c.la_nvec, c.la_ew, 1.f, c.msg_aa[7]};
  RunGroup a_ar{nL, nR, aB, nA, ar.goff, ar.tgt, ar.tslot, ar.arow, c.ar_edge_base, c.Ear, nullptr, c.rec_sig,
                c.ar_batch, c.ar_nvec, nullptr, 1.f, c.msg_aa[8]};
  a_la.vn = 4; a_ra.vn = 5; a_aa.vn = 6; a_al.vn = 7; a_al.load = true; a_ar.vn = 8;
  a_ra.static_topo = a_aa.static_topo = a_ar.static_topo = !crop;   // static atom relations (set_complex) unless cropped per step
  t_phase.reset();
  for (int l = 0; l < Lc; ++l, ++xi) {
    if (l < Lc - 1)
      run_conv(m, m.conv_layers[l], {a_ll, a_lr, a_la, a_rr, a_rl, a_ra, a_aa, a_al, a_ar}, crop ? c.rg_aa_all_crop : c.rg_aa_all, 9,
               c.X[xi], c.X[xi + 1], 0, c.N, s);
    else run_conv(m, m.conv_layers[l], {a_ll, a_lr, a_la}, c.rg_aa_lig, 3, c.X[xi], c.X[xi + 1], 0, nL, s);
  }
}

// legacy confidence head (old_cg_model.py:283-291 = old_aa_model.py:284-295) on the final ligand rows
static void old_confidence_head(Model& m, const float* XL, int D_last, int n_out, float* conf_out, hipStream_t s) {
  Cx& c = *m.cx;
  const int Lc = m.cfg.num_conv_layers;
  ConfHeadArgs a{};
  a.B = c.B; a.X = XL; a.ldx = XS; a.col0 = 0; a.lig_ptr = c.lig_ptr; a.ns = m.ns;
  a.n_tail = Lc >= 3 ? m.ns : 0;
  a.tail_off = D_last - a.n_tail;
  a.W0 = m.conf_W[0]; a.b0 = m.conf_b[0]; a.sc0 = m.conf_bn_scale[0]; a.sh0 = m.conf_bn_shift[0];
  a.W1 = m.conf_W[1]; a.b1 = m.conf_b[1]; a.sc1 = m.conf_bn_scale[1]; a.sh1 = m.conf_bn_shift[1];
  a.W2 = m.conf_W[2]; a.b2 = m.conf_b[2]; a.n_out = n_out; a.out = conf_out;
  launch_conf_head(a, s);
}

// ============================================================ legacy all-atom class
// models/old_aa_model.py:202-348 (AAOldModel.forward, score and confidence mode): ligand, residue and atom rows from OldAtomEncoders,
// six edge embeddings that all carry the sigma embedding of edge_index[0]'s graph, and per interaction layer nine separate
// OldTensorProductConvLayers conv_layers[9l + k] -- each its own fc, tensor product, mean over its own edges and BatchNorm -- three of
// which meet in every node type: X_{l+1}[type] = pad(X_l[type]) + u1 + u2 + u3 (k_reduce_bn_sum).  The last layer runs the three
// ligand modules only.  crop: as run_aa_layers -- the residues beyond the cutoff and their atoms lose every edge (masks in the pair
// searches, the static relations through their compaction); their rows stay in the tables and nothing reads them.
static void forward_old_aa(Model& m, const float* lig_pos, const float* t_tr, const float* t_rot, const float* t_tor, float* tr_out,
                           float* rot_out, float* tor_out, float* conf_out, hipStream_t s) {
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int ns = m.ns, sd = m.sd, B = c.B, nL = c.nL, nR = c.nR, nA = c.nA, aB = nL + nR, Lc = cfg.num_conv_layers;
  const bool conf = cfg.confidence_mode != 0, crop = m.crop_cutoff > 0.0;
  DDMI_REQUIRE(!crop || c.ar_arange, DDMI_ERR_ARG,
               "crop_beyond of an all-atom complex needs one atom_rec_edge_index column per atom, column k for atom k (n_atom_rec_edges == "
               "n_atom, row 0 == 0..n_atom-1): the reference rewrites the relation as arange(kept atoms) (utils/utils.py:395-399)");
  ++c.epoch;
  PhaseTimer t_fwd(m, "forward_total", s);
  std::unique_ptr<PhaseTimer> t_phase(new PhaseTimer(m, "embed_and_graphs", s));
  launch_time_embedding(t_tr, B, m.time_freq, sd / 2, cfg.embedding_scale, cfg.embedding_type, c.temb, s);
  {   // everything linear in the sigma embedding, one launch: OldAtomEncoder.linear of the three node types (the receptor's through
      // the sigma columns of lm_embedding_layer, as forward_old), the sigma columns of the six edge embeddings, the read-outs' terms
    struct Term { const float* W; int ldw; const float* bias; float* C; };
    const bool lm = m.lm > 0;
    const Term terms[] = {{m.old_lig_lin.W0, sd, m.old_lig_lin.b0, c.ligsig},
                          {lm ? m.old_lm_W + ns + m.lm - sd : m.old_rec_lin.W0, lm ? ns + m.lm : sd, lm ? nullptr : m.old_rec_lin.b0, c.rec_sig},
                          {m.old_atom_lin.W0, sd, m.old_atom_lin.b0, c.atom_sig},
                          {m.lig_edge.W0 + m.nf, m.lig_edge.in, m.lig_edge.b0, c.ll_gvec},
                          {m.rec_edge.W0, m.rec_edge.in, m.rec_edge.b0, c.rr_sig_old},
                          {m.atom_edge.W0, m.atom_edge.in, m.atom_edge.b0, c.aa_sig_old},
                          {m.cross_edge.W0, m.cross_edge.in, m.cross_edge.b0, c.cross_gvec},
                          {m.ar_edge.W0, m.ar_edge.in, m.ar_edge.b0, c.ar_sig_old},
                          {m.la_edge.W0, m.la_edge.in, m.la_edge.b0, c.la_gvec},
                          // score mode only (old_aa_model.py:299-300,311-322)
                          {m.center_edge.W0 + m.D, m.center_edge.in, m.center_edge.b0, c.center_gvec},
                          {m.tr_final.W0 + 1, 1 + sd, m.tr_final.b0, c.tr_sig},
                          {m.rot_final.W0 + 1, 1 + sd, m.rot_final.b0, c.rot_sig}};
    GemmBatch gb;
    for (const Term& q : terms) {
      if (gb.n == (conf ? 9 : 12)) break;
      GemmArgs& x = gb.g[gb.n++];
      x.A = c.temb; x.lda = sd; x.W = q.W; x.ldw = q.ldw; x.bias = q.bias; x.C = q.C; x.ldc = ns; x.M = B; x.N = ns; x.K = sd;
    }
    launch_gemm_batch(gb, s);
  }
  // ---- node table [lig | rec | atom]: static embedding sums + the per-graph sigma term
  float* X0 = c.X[0];
  launch_lig_node_embed(c.lig_x, nL, m.lig_emb, m.lig_emb_off, 16, ns, c.embsum, s);
  launch_add_rowvec(X0, XS, c.embsum, ns, c.ligsig, ns, c.lig_batch, nL, ns, ns, s);
  launch_add_rowvec(X0 + (size_t)nL * XS, XS, c.rec_node_base, XS, c.rec_sig, ns, c.rec_batch, nR, ns, ns, s);
  launch_add_rowvec(X0 + (size_t)aB * XS, XS, c.atom_node_base, XS, c.atom_sig, ns, c.atom_batch, nA, ns, ns, s);
  // ---- per-step crop: residue and atom masks, the four static relations re-compacted under them (as forward)
  if (crop) {
    const double cd = m.crop_cutoff;
    {
      PhaseTimer t(m, "k_crop_mask", s);
      launch_crop_mask(lig_pos, c.rec_pos, c.rec_batch, c.lig_ptr, nR, (float)(cd * cd), c.keep, s);
      launch_crop_atom_mask(c.keep, c.atom_res, nA, c.keep_atom, s);
    }
    RelFilterArgs fa;
    fa.r[fa.n++] = RelFilter{c.keep, c.keep, nR, nR, nL, c.rr_goff, c.rr_tgt, c.rr_arow, c.rr_toff, c.rr_tlist, c.rr_gnode,
                             c.cnt_g2, c.cnt_t2, c.goff2, c.toff2, c.tslot_tmp, c.tgt2, c.tslot2, c.arow2};
    auto add = [&](const Cx::StaticEdges& e, const int* gkeep, int gn, const int* tkeep, int tn, int tbase) {
      fa.r[fa.n++] = RelFilter{gkeep, tkeep, gn, tn, tbase, e.goff, e.tgt, e.arow, e.toff, e.tlist, e.gnode,
                               e.cnt_g, e.cnt_t, e.goff2, e.toff2, e.tslot_tmp, e.tgt2, e.tslot2, e.arow2};
    };
    add(c.se_aa, c.keep_atom, nA, c.keep_atom, nA, aB);
    add(c.se_ar, c.keep, nR, c.keep_atom, nA, aB);
    add(c.se_ra, c.keep_atom, nA, c.keep, nR, nL);
    PhaseTimer t(m, "k_rel_filter", s);
    launch_rel_filter(fa, s);
  }
  // ---- graphs and edge embeddings.  Distance expansions (old_aa_model.py:440,462,476,485): atom-atom through the LIGAND one,
  // lig-atom through the CROSS one, atom-rec through the receptor one
  lig_graph(m, lig_pos, s);
  launch_edge_mlp(mlp_args(m.rec_edge, ns, c.Err, nullptr, c.rr_dist, m.off_rec, m.D, m.coeff_rec, sd, c.rr_sig_old, c.rr_batch,
                           c.rec_edge_base), s);
  launch_edge_mlp(mlp_args(m.atom_edge, ns, c.Eaa, nullptr, c.aa_dist, m.off_lig, m.D, m.coeff_lig, sd, c.aa_sig_old, c.aa_batch,
                           c.atom_edge_base), s);
  launch_edge_mlp(mlp_args(m.ar_edge, ns, c.Ear, nullptr, c.ar_dist, m.off_rec, m.D, m.coeff_rec, sd, c.ar_sig_old, c.ar_batch,
                           c.ar_edge_base), s);
  const float* cut_dev = nullptr;
  if (cfg.dynamic_max_cross) {   // confidence mode feeds the raw t as sigma (old_aa_model.py:206-209,227)
    launch_cross_cutoff(t_tr, B, cfg.tr_sigma_min, cfg.tr_sigma_max, c.cutoff, s, conf ? 1 : 0);
    cut_dev = c.cutoff;
  }
  launch_cross_count(lig_pos, c.rec_pos, c.lig_batch, c.rec_batch, c.lig_ptr, c.rec_ptr, nL, nR, c.maxNr, cut_dev,
                     cfg.cross_max_distance, crop ? c.keep : nullptr, c.pairrank, c.cnt_l, c.cnt_r, s);
  launch_exclusive_scan2(c.cnt_l, c.offs_l, nL, c.cnt_r, c.offs_r, nR, s);
  launch_cross_fill(lig_pos, c.rec_pos, c.rec_batch, c.lig_ptr, c.rec_ptr, nL, nR, c.maxNr, c.pairrank, c.offs_l, c.offs_r,
                    cut_dev, cfg.cross_max_distance, cfg.smooth_edges, c.g1_tgt, c.g1_tslot, c.g3_tgt, c.g3_tslot, c.pbatch,
                    c.pdist, c.pnvec, c.pew, s);
  launch_edge_mlp(mlp_args(m.cross_edge, ns, c.Elr_cap, c.offs_l + nL, c.pdist, m.off_cross, m.Dc, m.coeff_cross, sd,
                           c.cross_gvec, c.pbatch, c.cross_ea), s);
  launch_cross_count(lig_pos, c.atom_pos, c.lig_batch, c.atom_batch, c.lig_ptr, c.atom_ptr, nL, nA, c.maxNa, nullptr,
                     cfg.lig_max_radius, crop ? c.keep_atom : nullptr, c.la_pairrank, c.la_cnt_l, c.la_cnt_a, s);
  launch_exclusive_scan2(c.la_cnt_l, c.la_offs_l, nL, c.la_cnt_a, c.la_offs_a, nA, s);
  launch_cross_fill(lig_pos, c.atom_pos, c.atom_batch, c.lig_ptr, c.atom_ptr, nL, nA, c.maxNa, c.la_pairrank, c.la_offs_l,
                    c.la_offs_a, nullptr, cfg.lig_max_radius, cfg.smooth_edges, c.la1_tgt, c.la1_tslot, c.la3_tgt, c.la3_tslot,
                    c.la_pbatch, c.la_dist, c.la_nvec, c.la_ew, s, aB);
  launch_edge_mlp(mlp_args(m.la_edge, ns, c.Ela_cap, c.la_offs_l + nL, c.la_dist, m.off_cross, m.Dc, m.coeff_cross, sd, c.la_gvec,
                           c.la_pbatch, c.la_ea), s);
  // ---- the nine modules of a layer in the reference's order (old_aa_model.py:236-271); every first Linear sees
  // [edge, target, gathered], the flipped ones reuse the forward spherical harmonics
  const Rel rr = crop ? Rel{c.goff2, c.tgt2, c.tslot2, c.arow2} : Rel{c.rr_goff, c.rr_tgt, c.rr_tslot, c.rr_arow};
  const Rel ra = rel_of(c.se_ra, crop), aa = rel_of(c.se_aa, crop), ar = rel_of(c.se_ar, crop);
  RunGroup g[9] = {
      {0, nL, 0, nL, c.goff_ll, c.ll_tgt, c.ll_tslot, nullptr, c.ll_ea, c.Ell_cap, c.goff_ll + nL, nullptr, nullptr, c.ll_nvec,
       c.ll_ew, 1.f, c.msg_aa[0]},                                                                                  // 9l + 0  lig <- lig
      {nL, nR, 0, nL, c.offs_r, c.g1_tgt, c.g1_tslot, c.g1_tslot, c.cross_ea, c.Elr_cap, c.offs_l + nL, nullptr, nullptr, c.pnvec,
       c.pew, 1.f, c.msg_aa[1]},                                                                                    // 9l + 1  lig <- rec
      {aB, nA, 0, nL, c.la_offs_a, c.la1_tgt, c.la1_tslot, c.la1_tslot, c.la_ea, c.Ela_cap, c.la_offs_l + nL, nullptr, nullptr,
       c.la_nvec, c.la_ew, 1.f, c.msg_aa[2]},                                                                       // 9l + 2  lig <- atom
      {aB, nA, aB, nA, aa.goff, aa.tgt, aa.tslot, aa.arow, c.atom_edge_base, c.Eaa, nullptr, nullptr, nullptr, c.aa_nvec, c.aa_ew,
       1.f, c.msg_aa[6]},                                                                                           // 9l + 3  atom <- atom
      {0, nL, aB, nA, c.la_offs_l, c.la3_tgt, c.la3_tslot, nullptr, c.la_ea, c.Ela_cap, c.la_offs_l + nL, nullptr, nullptr,
       c.la_nvec, c.la_ew, 1.f, c.msg_aa[7]},                                                                       // 9l + 4  atom <- lig
      {nL, nR, aB, nA, ar.goff, ar.tgt, ar.tslot, ar.arow, c.ar_edge_base, c.Ear, nullptr, nullptr, nullptr, c.ar_nvec, nullptr,
       1.f, c.msg_aa[8]},                                                                                           // 9l + 5  atom <- rec
      {nL, nR, nL, nR, rr.goff, rr.tgt, rr.tslot, rr.arow, c.rec_edge_base, c.Err, nullptr, nullptr, nullptr, c.rr_nvec, c.rr_ew,
       1.f, c.msg_aa[3]},                                                                                           // 9l + 6  rec <- rec
      {0, nL, nL, nR, c.offs_l, c.g3_tgt, c.g3_tslot, nullptr, c.cross_ea, c.Elr_cap, c.offs_l + nL, nullptr, nullptr, c.pnvec,
       c.pew, 1.f, c.msg_aa[4]},                                                                                    // 9l + 7  rec <- lig
      {aB, nA, nL, nR, ra.goff, ra.tgt, ra.tslot, ra.arow, c.ar_edge_base, c.Ear, nullptr, nullptr, nullptr, c.ar_nvec, nullptr,
       1.f, c.msg_aa[5]}};                                                                                          // 9l + 8  rec <- atom
  static const int vn_of[9] = {2, 0, 4, 6, 7, 8, 1, 3, 5};   // virtual-node list of every module (set_complex)
  for (int k = 0; k < 9; ++k) g[k].vn = vn_of[k];
  g[0].load = g[4].load = g[7].load = true;
  g[3].static_topo = g[5].static_topo = g[6].static_topo = g[8].static_topo = !crop;
  // target-order offsets of the nine modules' messages
  const int* toff[9] = {c.toff_ll, c.offs_l, c.la_offs_l,
                        crop ? c.se_aa.toff2 : c.se_aa.toff, c.la_offs_a, crop ? c.se_ar.toff2 : c.se_ar.toff,
                        crop ? c.toff2 : c.rr_toff, c.offs_r, crop ? c.se_ra.toff2 : c.se_ra.toff};
  t_phase.reset();
  for (int l = 0; l < Lc; ++l) {
    const bool last = l == Lc - 1;
    const float* Xin = c.X[l];
    const int n_mod = last ? 3 : 9;
    for (int k = 0; k < n_mod; ++k) run_conv(m, m.old_aa[9 * l + k], {g[k]}, nullptr, 0, Xin, nullptr, 0, 0, s);
    PhaseTimer t(m, "k_reduce_bn_sum", s);
    // summed in the reference's order: lig + lig_update + la + lr ; atom + atom_update + al + ar ; rec + rec_update + ra + rl
    static const int order[3][3] = {{0, 2, 1}, {3, 4, 5}, {6, 8, 7}};
    const int base[3] = {0, aB, nL}, count[3] = {nL, nA, nR};
    for (int ty = 0; ty < (last ? 1 : 3); ++ty) {
      ReduceSumArgs a{};
      a.n_groups = 3;
      for (int j = 0; j < 3; ++j) {
        const int k = order[ty][j];
        const BnArgs bn = bn_args(m.old_aa[9 * l + k]);
        a.g[j] = ReduceSumGroup{toff[k], g[k].msg, bn.mean, bn.scale, bn.bias};
      }
      a.nbase = base[ty]; a.ncount = count[ty]; a.D_in = m.old_aa[9 * l].D_in; a.D_out = m.old_aa[9 * l].D_out;
      a.X_in = Xin; a.X_out = c.X[l + 1];
      launch_reduce_bn_sum(a, s);
    }
  }
  PhaseTimer t_read(m, "readouts", s);
  if (conf) old_confidence_head(m, c.X[Lc], m.old_aa[9 * (Lc - 1)].D_out, cfg.num_confidence_outputs + (cfg.affinity_prediction ? 1 : 0), conf_out, s);
  else score_readouts(m, c.X[Lc], lig_pos, t_tr, t_rot, t_tor, tr_out, rot_out, tor_out, s);
}

// cg_model.py:353-366: graph-mean of the even (and, from 3 layers on, the odd) scalars -> confidence_predictor
static void confidence_readout(Model& m, const float* XL, float* conf_out, float* atom_conf_out, hipStream_t s) {
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int ns = m.ns, B = c.B, nL = c.nL;
  const int total = cfg.num_conv_layers + cfg.num_prot_emb_layers;
  const ConvW& Ll = m.conv_layers.back();
  ConfHeadArgs a{};
  a.B = B; a.X = XL; a.ldx = XS; a.col0 = 0; a.lig_ptr = c.lig_ptr; a.ns = ns;
  a.n_tail = total >= 3 ? (cfg.reduce_pseudoscalars ? cfg.nv : ns) : 0;
  a.tail_off = Ll.D_out - a.n_tail;
  if (cfg.atom_confidence) {   // cg_model.py:357-360: per-atom predictor; columns [0, n_atom_out) are the atom outputs, the
                               // remaining ns columns replace the scalar features in the graph mean
    const int n_in = ns + a.n_tail, na = cfg.atom_num_confidence_outputs, wo = na + ns;
    launch_gather_cols(c.ac_in, n_in, 0, XL, XS, nullptr, nL, ns, nullptr, s);
    if (a.n_tail > 0) launch_gather_cols(c.ac_in, n_in, ns, XL + a.tail_off, XS, nullptr, nL, a.n_tail, nullptr, s);
    gemm(c.ac_in, n_in, m.aconf_W[0], n_in, m.aconf_b[0], c.ac_h0, ns, nL, ns, n_in, 1, s);
    gemm(c.ac_h0, ns, m.aconf_W[1], ns, m.aconf_b[1], c.ac_h1, ns, nL, ns, ns, 1, s);
    gemm(c.ac_h1, ns, m.aconf_W[2], ns, m.aconf_b[2], c.ac_out, wo, nL, wo, ns, 0, s);
    launch_gather_cols(atom_conf_out, na, 0, c.ac_out, wo, nullptr, nL, na, nullptr, s);
    a.X = c.ac_out; a.ldx = wo; a.col0 = na; a.n_tail = 0; a.tail_off = 0;
  }
  a.W0 = m.conf_W[0]; a.b0 = m.conf_b[0]; a.sc0 = m.conf_bn_scale[0]; a.sh0 = m.conf_bn_shift[0];
  a.W1 = m.conf_W[1]; a.b1 = m.conf_b[1]; a.sc1 = m.conf_bn_scale[1]; a.sh1 = m.conf_bn_shift[1];
  a.W2 = m.conf_W[2]; a.b2 = m.conf_b[2]; a.n_out = cfg.num_confidence_outputs + (cfg.affinity_prediction ? 1 : 0); a.out = conf_out;
  launch_conf_head(a, s);
}

// =================================================================================== forward
void forward(Model& m, const float* lig_pos, const float* t_tr, const float* t_rot, const float* t_tor, float* tr_out,
             float* rot_out, float* tor_out, hipStream_t s, float* conf_out, float* atom_conf_out) {
  DDMI_REQUIRE(m.has_complex, DDMI_ERR_STATE, "ddmi_set_complex must precede ddmi_forward");
  const bool conf = m.cfg.confidence_mode != 0;
  DDMI_REQUIRE(conf == (conf_out != nullptr), DDMI_ERR_STATE, "score models use ddmi_forward, confidence models ddmi_confidence");
  DDMI_REQUIRE(conf || !m.cfg.scale_by_sigma || (m.so3_table && (m.cfg.no_torsion || m.torus_table)), DDMI_ERR_STATE,
               "score-norm tables not set (ddmi_set_table)");
  if (m.cfg.old_model) {
    (m.cfg.all_atoms ? forward_old_aa : forward_old)(m, lig_pos, t_tr, t_rot, t_tor, tr_out, rot_out, tor_out, conf_out, s);
    return;
  }
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int ns = m.ns, sd = m.sd, B = c.B, nL = c.nL, nR = c.nR;
  ++c.epoch;
  PhaseTimer t_fwd(m, "forward_total", s);
  std::unique_ptr<PhaseTimer> t_phase(new PhaseTimer(m, "embed_and_graphs", s));
  // ---- cross graph (cg_model.py:539-562): its pair search needs only the ligand positions and t, so without a per-step crop it runs on
  // the side stream from the very start of the forward (round 6: next to the time terms; rounds 2-5 forked behind them), its edge
  // MLP -- which needs the per-graph time term -- behind an event; the ligand node encoder and the receptor rows of the first table
  // (time terms only) follow it there, so the main stream goes from the time terms straight to the ligand graph.
  const bool crop = m.crop_cutoff > 0.0;
  DDMI_REQUIRE(!(crop && cfg.all_atoms) || c.ar_arange, DDMI_ERR_ARG,
               "crop_beyond of an all-atom complex needs one atom_rec_edge_index column per atom, column k for atom k (n_atom_rec_edges == "
               "n_atom, row 0 == 0..n_atom-1): the reference rewrites the relation as arange(kept atoms) (utils/utils.py:395-399)");
  const float* cut_dev = cfg.dynamic_max_cross ? c.cutoff : nullptr;
  auto cross_pairs = [&](hipStream_t cs, const int* keep_) {
    if (cfg.dynamic_max_cross)   // cutoff_b = 3 * tr_sigma_b + 20 (cg_model.py:321-322)
      launch_cross_cutoff(t_tr, B, cfg.tr_sigma_min, cfg.tr_sigma_max, c.cutoff, cs, conf ? 1 : 0);
    launch_cross_count(lig_pos, c.rec_pos, c.lig_batch, c.rec_batch, c.lig_ptr, c.rec_ptr, nL, nR, c.maxNr, cut_dev,
                       cfg.cross_max_distance, keep_, c.pairrank, c.cnt_l, c.cnt_r, cs);
    launch_exclusive_scan2(c.cnt_l, c.offs_l, nL, c.cnt_r, c.offs_r, nR, cs);
    launch_cross_fill(lig_pos, c.rec_pos, c.rec_batch, c.lig_ptr, c.rec_ptr, nL, nR, c.maxNr, c.pairrank, c.offs_l, c.offs_r,
                      cut_dev, cfg.cross_max_distance, cfg.smooth_edges, c.g1_tgt, c.g1_tslot, c.g3_tgt, c.g3_tslot, c.pbatch,
                      c.pdist, c.pnvec, c.pew, cs);
  };
  auto cross_attr = [&](hipStream_t cs) {
    launch_edge_mlp(mlp_args(m.cross_edge, ns, c.Elr_cap, c.offs_l + nL, c.pdist, m.off_cross, m.Dc, m.coeff_cross, sd,
                             c.cross_gvec, c.pbatch, c.cross_ea), cs);
  };
  auto cross_graph = [&](hipStream_t cs, const int* keep_) { cross_pairs(cs, keep_); cross_attr(cs); };
  const bool early_cross = m.r.two_streams && m.side_stream && !crop;
  if (early_cross) {
    DDMI_CHECK_HIP(hipEventRecord(m.ev_fork, s));
    DDMI_CHECK_HIP(hipStreamWaitEvent(m.side_stream, m.ev_fork, 0));
    cross_pairs(m.side_stream, nullptr);
  }
  time_terms(m, t_tr, conf, s);
  // ---- node tables: ligand rows [0,nL), receptor rows [nL, nL+nR)
  float* X0 = c.X[0];
  // (no embedding layers, no all-atom rows to add: the first table is complete once the encoder rows are in -- side stream)
  const bool nodes_on_side = early_cross && m.lig_emb_layers.empty() && m.rec_emb_layers.empty();
  auto lig_nodes = [&](hipStream_t ns_) {
    launch_lig_node_embed(c.lig_x, nL, m.lig_emb, m.lig_emb_off, 16, ns, c.embsum, ns_);
    gemm(c.embsum, ns, m.lig_enc.W0, ns + sd, nullptr, X0, XS, nL, ns, ns, 0, ns_, nullptr, c.ligsig, c.lig_batch, ns);
  };
  if (early_cross) {
    DDMI_CHECK_HIP(hipEventRecord(m.ev_terms, s));
    DDMI_CHECK_HIP(hipStreamWaitEvent(m.side_stream, m.ev_terms, 0));
    cross_attr(m.side_stream);
    if (nodes_on_side) {
      lig_nodes(m.side_stream);
      launch_add_rowvec(c.X[0] + (size_t)nL * XS, XS, c.rec_node_base, XS, c.rec_sig, ns, c.rec_batch, nR, c.rec_base_dim, ns, m.side_stream);
    }
    DDMI_CHECK_HIP(hipEventRecord(m.ev_cross, m.side_stream));
  }
  if (!nodes_on_side) lig_nodes(s);
  lig_graph(m, lig_pos, s);
  RunGroup g_ll{0, nL, 0, nL, c.goff_ll, c.ll_tgt, c.ll_tslot, nullptr, c.ll_ea, c.Ell_cap, c.goff_ll + nL, nullptr,
                nullptr, c.ll_nvec, c.ll_ew, 1.f, c.msg[0]};
  g_ll.vn = 2; g_ll.load = true;
  int xi = 0;
  for (size_t i = 0; i < m.lig_emb_layers.size(); ++i, ++xi)
    run_conv(m, m.lig_emb_layers[i], {g_ll}, c.rg_ll, 1, c.X[xi], c.X[xi + 1], 0, nL, s);
  // ---- per-step receptor crop (utils/sampling.py:104-109, utils/utils.py:388-413): residue mask (all_atoms: + the mask of their
  // atoms) and the static relations re-compacted under the masks -- the contact graph; all_atoms: atom-atom, atom<-rec, rec<-atom
  const int* keep = nullptr;
  if (crop) {
    const double cd = m.crop_cutoff;
    const int aB = nL + nR, nA = c.nA;
    {
      PhaseTimer t(m, "k_crop_mask", s);
      launch_crop_mask(lig_pos, c.rec_pos, c.rec_batch, c.lig_ptr, nR, (float)(cd * cd), c.keep, s);
      if (cfg.all_atoms) launch_crop_atom_mask(c.keep, c.atom_res, nA, c.keep_atom, s);
    }
    RelFilterArgs fa;
    fa.r[fa.n++] = RelFilter{c.keep, c.keep, nR, nR, nL, c.rr_goff, c.rr_tgt, c.rr_arow, c.rr_toff, c.rr_tlist, c.rr_gnode,
                             c.cnt_g2, c.cnt_t2, c.goff2, c.toff2, c.tslot_tmp, c.tgt2, c.tslot2, c.arow2};
    auto add = [&](const Cx::StaticEdges& e, const int* gkeep, int gn, const int* tkeep, int tn, int tbase) {
      fa.r[fa.n++] = RelFilter{gkeep, tkeep, gn, tn, tbase, e.goff, e.tgt, e.arow, e.toff, e.tlist, e.gnode,
                               e.cnt_g, e.cnt_t, e.goff2, e.toff2, e.tslot_tmp, e.tgt2, e.tslot2, e.arow2};
    };
    if (cfg.all_atoms) {
      add(c.se_aa, c.keep_atom, nA, c.keep_atom, nA, aB);
      add(c.se_ar, c.keep, nR, c.keep_atom, nA, aB);
      add(c.se_ra, c.keep_atom, nA, c.keep, nR, nL);
    }
    PhaseTimer t(m, "k_rel_filter", s);
    launch_rel_filter(fa, s);
    keep = c.keep;
  }
  // receptor rows of the current table: cached embedding + sigma term on the scalars (cg_model.py:298-301)
  const float* atom_rows = c.atom_node_base;
  if (crop && !m.rec_emb_layers.empty() && cfg.all_atoms) {
    // aa_model.py:296-318 on the CROPPED residue + atom graph (the reference re-embeds it every step, see below): groups
    // [rr, ar, aa, ra] through the compacted relations, from the encoder rows, in the two tables set_complex embedded in
    const int aB = nL + nR, nA = c.nA;
    DDMI_CHECK_HIP(hipMemcpyAsync(c.emb_a + (size_t)nL * XS, c.rec_node_enc, (size_t)nR * XS * 4, hipMemcpyDeviceToDevice, s));
    DDMI_CHECK_HIP(hipMemcpyAsync(c.emb_a + (size_t)aB * XS, c.atom_node_enc, (size_t)nA * XS * 4, hipMemcpyDeviceToDevice, s));
    const Rel ra = rel_of(c.se_ra, true), aa = rel_of(c.se_aa, true), ar = rel_of(c.se_ar, true);
    RunGroup e_rr{nL, nR, nL, nR, c.goff2, c.tgt2, c.tslot2, c.arow2, c.rec_edge_base, c.Err, nullptr, nullptr, nullptr,
                  c.rr_nvec, c.rr_ew, 1.f, c.msg_aa[3]};
    RunGroup e_ar{nL, nR, aB, nA, ar.goff, ar.tgt, ar.tslot, ar.arow, c.ar_edge_base, c.Ear, nullptr, nullptr, nullptr,
                  c.ar_nvec, nullptr, 1.f, c.msg_aa[8]};
    RunGroup e_aa{aB, nA, aB, nA, aa.goff, aa.tgt, aa.tslot, aa.arow, c.atom_edge_base, c.Eaa, nullptr, nullptr, nullptr,
                  c.aa_nvec, c.aa_ew, 1.f, c.msg_aa[6]};
    RunGroup e_ra{aB, nA, nL, nR, ra.goff, ra.tgt, ra.tslot, ra.arow, c.ar_edge_base, c.Ear, nullptr, nullptr, nullptr,
                  c.ar_nvec, nullptr, 1.f, c.msg_aa[5]};
    e_rr.vn = 1; e_ar.vn = 8; e_aa.vn = 6; e_ra.vn = 5;
    float *xin = c.emb_a, *xout = c.emb_b;
    for (size_t i = 0; i < m.rec_emb_layers.size(); ++i, std::swap(xin, xout))
      run_conv(m, m.rec_emb_layers[i], {e_rr, e_ar, e_aa, e_ra}, c.rg_emb_crop, 4, xin, xout, nL, nR + nA, s);
    atom_rows = xin + (size_t)aB * XS;
    launch_add_rowvec(c.X[xi] + (size_t)nL * XS, XS, xin + (size_t)nL * XS, XS, c.rec_sig, ns, c.rec_batch, nR, c.rec_base_dim, ns, s);
  } else if (crop && !m.rec_emb_layers.empty()) {
    // the reference re-embeds the CROPPED receptor every step (the cache lives on the discarded deep copy)
    launch_add_rowvec(c.X[0] + (size_t)nL * XS, XS, c.rec_node_enc, XS, nullptr, 0, nullptr, nR, ns, 0, s);
    RunGroup g_rr0{nL, nR, nL, nR, c.goff2, c.tgt2, c.tslot2, c.arow2, c.rec_edge_base, c.Err, nullptr, nullptr,
                   nullptr, c.rr_nvec, c.rr_ew, 1.f, c.msg[2]};
    g_rr0.vn = 1;
    for (size_t i = 0; i < m.rec_emb_layers.size(); ++i)
      run_conv(m, m.rec_emb_layers[i], {g_rr0}, c.rg_rr_crop, 1, c.X[i], c.X[i + 1], nL, nR, s);
    launch_add_rowvec(c.X[xi] + (size_t)nL * XS, XS, c.X[xi] + (size_t)nL * XS, XS, c.rec_sig, ns, c.rec_batch, nR,
                      c.rec_base_dim, ns, s);
  } else if (!nodes_on_side) {
    launch_add_rowvec(c.X[xi] + (size_t)nL * XS, XS, c.rec_node_base, XS, c.rec_sig, ns, c.rec_batch, nR, c.rec_base_dim, ns, s);
  }
  if (early_cross) DDMI_CHECK_HIP(hipStreamWaitEvent(s, m.ev_cross, 0));
  else cross_graph(s, keep);
  // ---- interaction layers over [ll ; lig<-rec ; rec-rec ; rec<-lig]  (cg_model.py:329-349)
  RunGroup g_lr{nL, nR, 0, nL, c.offs_r, c.g1_tgt, c.g1_tslot, c.g1_tslot, c.cross_ea, c.Elr_cap, c.offs_l + nL, nullptr,
                      nullptr, c.pnvec, c.pew, 1.f, c.msg[1]};
  RunGroup g_rr{nL, nR, nL, nR, crop ? c.goff2 : c.rr_goff, crop ? c.tgt2 : c.rr_tgt, crop ? c.tslot2 : c.rr_tslot,
                      crop ? c.arow2 : c.rr_arow, c.rec_edge_base, c.Err, nullptr, c.rec_sig, c.rr_batch, c.rr_nvec, c.rr_ew,
                      1.f, c.msg[2]};
  RunGroup g_rl{0, nL, nL, nR, c.offs_l, c.g3_tgt, c.g3_tslot, nullptr, c.cross_ea, c.Elr_cap, c.offs_l + nL, nullptr,
                nullptr, c.pnvec, c.pew, -1.f, c.msg[3]};
  g_lr.vn = 0; g_rr.vn = 1; g_rl.vn = 3; g_rl.load = true;
  g_rr.static_topo = !crop;   // the contact graph of an uncropped receptor is a per-complex constant: its lists and per-edge rows are built once
  if (cfg.all_atoms) run_aa_layers(m, lig_pos, g_ll, g_lr, g_rr, g_rl, crop, atom_rows, xi, t_phase, s);
  else {
    t_phase.reset();
    run_cg_layers(m, g_ll, g_lr, g_rr, g_rl, crop, xi, s);
  }
  const float* XL = c.X[xi];
  c.x_last = conf ? nullptr : XL;   // (a confidence pass leaves no table for ddmi_sidechain_pred to read)
  PhaseTimer t_read(m, "readouts", s);
  if (conf) confidence_readout(m, XL, conf_out, atom_conf_out, s);
  else score_readouts(m, XL, lig_pos, t_tr, t_rot, t_tor, tr_out, rot_out, tor_out, s);
}

// models/cg_model.py:397-402: sidechain_predictor (o3.Linear, folded into one [10][K] matrix at commit) on the receptor rows.
// Rows = ALL residues of the complex, in their original order: with a device-side crop (ddmi_set_crop_cutoff) the cropped
// residues are still rows of the node table (BatchNorm(0) + their input row) -- the reference crops the graph first and returns
// the kept residues only, so the caller compacts the rows through the `crop_keep` mask (MIScoreModel.__call__ does).
void sidechain_pred(Model& m, float* out, hipStream_t s) {
  DDMI_REQUIRE(m.has_complex && m.cx->x_last && m.side_Mt, DDMI_ERR_STATE,
               "ddmi_sidechain_pred reads the node table of the ddmi_forward directly before it (none since the last ddmi_confidence / ddmi_sample / ddmi_set_complex)");
  Cx& c = *m.cx;
  gemm(c.x_last + (size_t)c.nL * XS, XS, m.side_Mt, m.side_K, nullptr, out, 10, c.nR, 10, m.side_K, 0, s);
}

}  // namespace ddmi
