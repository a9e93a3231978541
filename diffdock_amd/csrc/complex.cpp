// The static description of one collated batch of complexes and its device workspace: ddmi_set_complex (one-time topology
// read-back -- the only host synchronisation of the library -- uploads, workspace, receptor-side constants) and
// ddmi_set_batch_layout.
#include <algorithm>
#include <numeric>
#include <string>

#include "cx.h"

namespace ddmi {

// ---- message buffers and the reduce-group lists of the node updates (copies: batch of copies of one receptor of R1 residues)
static void alloc_messages(Model& m, bool copies, int R1) {
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int ns = m.ns, B = c.B, nL = c.nL, nR = c.nR;
  const int ecap[4] = {c.Ell_cap, c.Elr_cap, c.Err, c.Elr_cap};
  for (int g = 0; g < 4; ++g) c.msg[g] = dalloc<float>(m, nullptr, {ecap[g], XS});
  {
    std::vector<ReduceGroup> rg = {{c.toff_ll, c.msg[0], 0, nL}, {c.offs_l, c.msg[1], 0, nL},
                                   {c.rr_toff, c.msg[2], nL, nR}, {c.offs_r, c.msg[3], nL, nR}};
    rg[1].live = c.prered ? c.vn[0].live : nullptr;   // (copied into every list that holds the lig<-rec group)
    c.rg_all = m.cpool.upload(rg);
    if (copies) {   // layer 0 under rec_share: the rec-rec rows of graph 0 serve every graph
      std::vector<ReduceGroup> rs = rg;
      rs[2].tmod = R1;
      c.rg_all_share = m.cpool.upload(rs);
    }
    std::vector<ReduceGroup> rl(rg.begin(), rg.begin() + 2);
    c.rg_lig = m.cpool.upload(rl);
    std::vector<ReduceGroup> r0(rg.begin(), rg.begin() + 1);
    c.rg_ll = m.cpool.upload(r0);
    std::vector<ReduceGroup> r2 = {{c.rr_toff, c.msg[2], 0, nR}};  // receptor-only embedding layers index nodes from 0
    c.rg_rr = m.cpool.upload(r2);
    std::vector<ReduceGroup> rc = rg;
    rc[2].toff = c.toff2;
    c.rg_all_crop = m.cpool.upload(rc);
    std::vector<ReduceGroup> r2c = {{c.toff2, c.msg[2], nL, nR}};  // cropped embedding layers run in the full node table
    c.rg_rr_crop = m.cpool.upload(r2c);
    if (cfg.all_atoms) {
      // dynamic ligand <-> atom relation (radius lig_max_radius, aa_model.py:606-614): same pair machinery as the cross graph
      const int nA = c.nA;
      c.la_pairrank = dalloc<int>(m, nullptr, {nL, c.maxNa}); c.la_cnt_l = dalloc<int>(m, nullptr, {nL});
      c.la_cnt_a = dalloc<int>(m, nullptr, {nA}); c.la_offs_l = dalloc<int>(m, "offs_la_l", {nL + 1});
      c.la_offs_a = dalloc<int>(m, "offs_la_a", {nA + 1});
      c.la1_tgt = dalloc<int>(m, nullptr, {c.Ela_cap}); c.la1_tslot = dalloc<int>(m, nullptr, {c.Ela_cap});
      c.la3_tgt = dalloc<int>(m, nullptr, {c.Ela_cap}); c.la3_tslot = dalloc<int>(m, nullptr, {c.Ela_cap});
      c.la_pbatch = dalloc<int>(m, nullptr, {c.Ela_cap}); c.la_dist = dalloc<float>(m, nullptr, {c.Ela_cap});
      c.la_nvec = dalloc<float>(m, nullptr, {c.Ela_cap, 3});
      c.la_ew = cfg.smooth_edges ? dalloc<float>(m, nullptr, {c.Ela_cap}) : nullptr;
      c.la_ea = dalloc<float>(m, nullptr, {c.Ela_cap, ns}); c.la_gvec = dalloc<float>(m, nullptr, {B, ns});
      // message buffers of the nine groups [ll, lr, la, rr, rl, ra, aa, al, ar] (aa_model.py:399-403), reduced per target type
      const int ecap9[9] = {c.Ell_cap, c.Elr_cap, c.Ela_cap, c.Err, c.Elr_cap, c.Ear, c.Eaa, c.Ela_cap, c.Ear};
      for (int g = 0; g < 9; ++g) c.msg_aa[g] = (g == 0 || g == 1 || g == 3 || g == 4) ? c.msg[g == 0 ? 0 : g == 1 ? 1 : g == 3 ? 2 : 3]
                                                                                          : dalloc<float>(m, nullptr, {ecap9[g], XS});
      std::vector<ReduceGroup> r9 = {{c.toff_ll, c.msg_aa[0], 0, nL}, {c.offs_l, c.msg_aa[1], 0, nL}, {c.la_offs_l, c.msg_aa[2], 0, nL},
                                     {c.rr_toff, c.msg_aa[3], nL, nR}, {c.offs_r, c.msg_aa[4], nL, nR}, {c.se_ra.toff, c.msg_aa[5], nL, nR},
                                     {c.se_aa.toff, c.msg_aa[6], nL + nR, nA}, {c.la_offs_a, c.msg_aa[7], nL + nR, nA},
                                     {c.se_ar.toff, c.msg_aa[8], nL + nR, nA}};
      r9[1].live = c.prered ? c.vn[0].live : nullptr;
      c.rg_aa_all = m.cpool.upload(r9);
      std::vector<ReduceGroup> r3(r9.begin(), r9.begin() + 3);
      c.rg_aa_lig = m.cpool.upload(r3);
      std::vector<ReduceGroup> r9c = r9;   // per-step crop: the four static relations through their compacted target offsets
      r9c[3].toff = c.toff2; r9c[5].toff = c.se_ra.toff2; r9c[6].toff = c.se_aa.toff2; r9c[8].toff = c.se_ar.toff2;
      c.rg_aa_all_crop = m.cpool.upload(r9c);
      std::vector<ReduceGroup> rec = {r9c[3], r9c[8], r9c[6], r9c[5]};   // the embedding layers' groups [rr, ar, aa, ra]
      c.rg_emb_crop = m.cpool.upload(rec);
    }
  }
}

// ---- read-out and sampler workspace
static void alloc_readouts(Model& m) {
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int ns = m.ns, B = c.B, nL = c.nL;
  const ConvW& F = m.final_conv;
  c.c_dist = dalloc<float>(m, nullptr, {nL}); c.c_nvec = dalloc<float>(m, nullptr, {nL, 3});
  c.c_ea = dalloc<float>(m, nullptr, {nL, ns}); c.c_attr = dalloc<float>(m, nullptr, {nL, F.n_edge});
  c.c_hid = dalloc<float>(m, nullptr, {nL, F.H}); c.c_W = dalloc<float>(m, nullptr, {nL, F.Wn});
  c.c_sh = dalloc<float>(m, nullptr, {nL, F.sh_dim}); c.c_out = dalloc<float>(m, nullptr, {nL, F.D_out});
  c.gp = dalloc<float>(m, "global_pred", {B, F.D_out});
  {
    std::vector<int> xr(nL);
    std::iota(xr.begin(), xr.end(), 0);
    c.c_xrow = m.cpool.upload(xr);
  }
  if (c.nT > 0) {
    const ConvW& T = m.tor_conv;
    c.t_cnt = dalloc<int>(m, "tor_cnt", {c.nT}); c.t_atom = dalloc<int>(m, nullptr, {c.Et});
    c.t_dist = dalloc<float>(m, nullptr, {c.Et}); c.t_nvec = dalloc<float>(m, nullptr, {c.Et, 3});
    c.t_ew = cfg.smooth_edges ? dalloc<float>(m, nullptr, {c.Et}) : nullptr;
    c.t_bond_nvec = dalloc<float>(m, nullptr, {c.nT, 3}); c.t_ea = dalloc<float>(m, nullptr, {c.Et, ns});
    c.t_attr = dalloc<float>(m, nullptr, {c.Et, T.n_edge}); c.t_hid = dalloc<float>(m, nullptr, {c.Et, T.H});
    c.t_W = dalloc<float>(m, nullptr, {c.Et, T.Wn}); c.t_sh = dalloc<float>(m, nullptr, {c.Et, T.sh_dim});
    c.t_out = dalloc<float>(m, nullptr, {c.Et, T.D_out}); c.t_feat = dalloc<float>(m, "tor_feat", {c.nT, T.D_out});
  }
  c.s_tr = dalloc<float>(m, nullptr, {B, 3}); c.s_rot = dalloc<float>(m, nullptr, {B, 3});
  c.s_tor = dalloc<float>(m, nullptr, {std::max(c.nT, 1)});
  c.s_t = nullptr; c.s_ids = nullptr;
}

// ---- receptor-side constants (CGModel.embedding caches these on the data object, cg_model.py:273-295); rr_tgt: target node of
// every rec-rec edge in gather order (host copy)
static void receptor_constants(Model& m, const ddmi_complex& cc, const std::vector<int>& rr_tgt, hipStream_t s) {
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int ns = m.ns, sd = m.sd, nL = c.nL, nR = c.nR, N = c.N;
  launch_rec_edge_geom(c.rec_pos, c.rr_src, c.rr_dst, c.Err, cfg.smooth_edges ? cfg.rec_max_radius : 0.f, c.rr_dist, c.rr_nvec,
                       c.rr_ew, s);
  if (!cfg.old_model)
    launch_edge_mlp(mlp_args(m.rec_edge, ns, c.Err, nullptr, c.rr_dist, m.off_rec, m.D, m.coeff_rec, 0, m.rec_edge.b0, nullptr,
                             c.rec_edge_base), s);
  if (cfg.old_model) {
    // OldAtomEncoder on rows [restype | ESM | sigma] (models/layers.py:104-118): scalar slice = ESM[:sd], language-model
    // slice = [ESM[sd:] | sigma].  Static per-residue part here; the sigma columns are a per-graph vector added per forward.
    std::vector<int> ident(nR);
    std::iota(ident.begin(), ident.end(), 0);
    int* rid = m.cpool.upload(ident);
    float* cat = dalloc<float>(m, nullptr, {nR, ns + m.lm});
    launch_concat_rec_input(cc.rec_x, 1 + m.lm, m.rec_emb, ns, m.lm, nR, cat, s);   // [E[restype] | ESM]
    if (m.lm > 0) {
      float* emb1 = dalloc<float>(m, nullptr, {nR, ns});
      gemm(cat + ns, ns + m.lm, m.old_rec_lin.W0, sd, m.old_rec_lin.b0, emb1, ns, nR, ns, sd, 0, s, nullptr, cat, rid, ns + m.lm);
      gemm(emb1, ns, m.old_lm_W, ns + m.lm, m.old_lm_b, c.rec_node_base, XS, nR, ns, ns, 0, s);
      gemm(cat + ns + sd, ns + m.lm, m.old_lm_W + ns, ns + m.lm, nullptr, c.rec_node_base, XS, nR, ns, m.lm - sd, 0, s, nullptr,
           c.rec_node_base, rid, XS);
    } else {
      launch_add_rowvec(c.rec_node_base, XS, cat, ns, nullptr, 0, nullptr, nR, ns, 0, s);
    }
  } else if (m.lm > 0) {
    float* cat = dalloc<float>(m, nullptr, {nR, ns + m.lm});
    launch_concat_rec_input(cc.rec_x, 1 + m.lm, m.rec_emb, ns, m.lm, nR, cat, s);
    gemm(cat, ns + m.lm, m.rec_enc_W, ns + m.lm, m.rec_enc_b, c.rec_node_base, XS, nR, ns, ns + m.lm, 0, s);
  } else {
    float* cat = dalloc<float>(m, nullptr, {nR, ns});
    launch_concat_rec_input(cc.rec_x, 1, m.rec_emb, ns, 0, nR, cat, s);
    launch_add_rowvec(c.rec_node_base, XS, cat, ns, nullptr, 0, nullptr, nR, ns, 0, s);
  }
  c.rec_base_dim = ns;
  if (cfg.all_atoms) {   // aa_model.py:288-294: atom encoder (sum of 4 embeddings, no extra features), static edge embeddings
    float* emb = dalloc<float>(m, nullptr, {c.nA, ns});
    launch_lig_node_embed(c.atom_x, c.nA, m.atom_emb, m.atom_emb_off, 4, ns, emb, s);
    launch_add_rowvec(c.atom_node_base, XS, emb, ns, nullptr, 0, nullptr, c.nA, ns, 0, s);
    if (!cfg.old_model) {   // (the legacy class feeds sigma into these MLPs: per forward, forward_old_aa)
      launch_edge_mlp(mlp_args(m.atom_edge, ns, c.Eaa, nullptr, c.aa_dist, m.off_lig, m.D, m.coeff_lig, 0, m.atom_edge.b0, nullptr,
                               c.atom_edge_base), s);
      launch_edge_mlp(mlp_args(m.ar_edge, ns, c.Ear, nullptr, c.ar_dist, m.off_rec, m.D, m.coeff_rec, 0, m.ar_edge.b0, nullptr,
                               c.ar_edge_base), s);
    }
  }
  c.rec_node_enc = nullptr;
  if (!m.rec_emb_layers.empty() && cfg.all_atoms) {
    // aa_model.py:296-318: embedding layers over the sigma-free residue + atom graph, groups [rr, ar, aa, ra]; run in the
    // full node numbering (ligand rows unused) so that the interaction-layer CSRs serve unchanged
    const int aB = nL + nR, nA = c.nA;
    float* ea = c.emb_a = dalloc<float>(m, nullptr, {N, XS}, true);
    float* eb = c.emb_b = dalloc<float>(m, nullptr, {N, XS}, true);
    // (kept for a per-step crop, which re-embeds the cropped graph from the encoder rows: forward)
    c.rec_node_enc = dalloc<float>(m, nullptr, {nR, XS}, true); c.atom_node_enc = dalloc<float>(m, nullptr, {nA, XS}, true);
    DDMI_CHECK_HIP(hipMemcpyAsync(c.rec_node_enc, c.rec_node_base, (size_t)nR * XS * 4, hipMemcpyDeviceToDevice, s));
    DDMI_CHECK_HIP(hipMemcpyAsync(c.atom_node_enc, c.atom_node_base, (size_t)nA * XS * 4, hipMemcpyDeviceToDevice, s));
    DDMI_CHECK_HIP(hipMemcpyAsync(ea + (size_t)nL * XS, c.rec_node_base, (size_t)nR * XS * 4, hipMemcpyDeviceToDevice, s));
    DDMI_CHECK_HIP(hipMemcpyAsync(ea + (size_t)aB * XS, c.atom_node_base, (size_t)nA * XS * 4, hipMemcpyDeviceToDevice, s));
    RunGroup e_rr{nL, nR, nL, nR, c.rr_goff, c.rr_tgt, c.rr_tslot, c.rr_arow, c.rec_edge_base, c.Err, nullptr, nullptr, nullptr,
                  c.rr_nvec, c.rr_ew, 1.f, c.msg_aa[3]};
    RunGroup e_ar{nL, nR, aB, nA, c.se_ar.goff, c.se_ar.tgt, c.se_ar.tslot, c.se_ar.arow, c.ar_edge_base, c.Ear, nullptr, nullptr,
                  nullptr, c.ar_nvec, nullptr, 1.f, c.msg_aa[8]};
    RunGroup e_aa{aB, nA, aB, nA, c.se_aa.goff, c.se_aa.tgt, c.se_aa.tslot, c.se_aa.arow, c.atom_edge_base, c.Eaa, nullptr, nullptr,
                  nullptr, c.aa_nvec, c.aa_ew, 1.f, c.msg_aa[6]};
    RunGroup e_ra{aB, nA, nL, nR, c.se_ra.goff, c.se_ra.tgt, c.se_ra.tslot, c.se_ra.arow, c.ar_edge_base, c.Ear, nullptr, nullptr,
                  nullptr, c.ar_nvec, nullptr, 1.f, c.msg_aa[5]};
    e_rr.vn = 1; e_ar.vn = 8; e_aa.vn = 6; e_ra.vn = 5;
    std::vector<ReduceGroup> re = {{c.rr_toff, c.msg_aa[3], nL, nR}, {c.se_ar.toff, c.msg_aa[8], aB, nA},
                                   {c.se_aa.toff, c.msg_aa[6], aB, nA}, {c.se_ra.toff, c.msg_aa[5], nL, nR}};
    ReduceGroup* rg_emb = m.cpool.upload(re);
    float *xin = ea, *xout = eb;
    for (size_t i = 0; i < m.rec_emb_layers.size(); ++i) {
      run_conv(m, m.rec_emb_layers[i], {e_rr, e_ar, e_aa, e_ra}, rg_emb, 4, xin, xout, nL, nR + nA, s);
      std::swap(xin, xout);
      c.rec_base_dim = m.rec_emb_layers[i].D_out;
    }
    DDMI_CHECK_HIP(hipMemcpyAsync(c.rec_node_base, xin + (size_t)nL * XS, (size_t)nR * XS * 4, hipMemcpyDeviceToDevice, s));
    DDMI_CHECK_HIP(hipMemcpyAsync(c.atom_node_base, xin + (size_t)aB * XS, (size_t)nA * XS * 4, hipMemcpyDeviceToDevice, s));
  } else if (!m.rec_emb_layers.empty()) {
    c.rec_node_enc = dalloc<float>(m, nullptr, {nR, XS}, true);
    DDMI_CHECK_HIP(hipMemcpyAsync(c.rec_node_enc, c.rec_node_base, (size_t)nR * XS * 4, hipMemcpyDeviceToDevice, s));
    // rec_emb_layers run on the sigma-free receptor graph (cg_model.py:288-290), node ids local to the receptor
    std::vector<int> tgt_local(c.Err);
    for (int e = 0; e < c.Err; ++e) tgt_local[e] = rr_tgt[e] - c.nL;
    int* tl = m.cpool.upload(tgt_local);
    float* xa = dalloc<float>(m, nullptr, {nR, XS}, true);
    float* xin = c.rec_node_base;
    for (size_t i = 0; i < m.rec_emb_layers.size(); ++i) {
      const ConvW& L = m.rec_emb_layers[i];
      RunGroup g{0, nR, 0, nR, c.rr_goff, tl, c.rr_tslot, c.rr_arow, c.rec_edge_base, c.Err, nullptr, nullptr, nullptr,
                 c.rr_nvec, c.rr_ew, 1.f, c.msg[2]};
      g.vn = 1;
      float* xout = (xin == c.rec_node_base) ? xa : c.rec_node_base;
      run_conv(m, L, {g}, c.rg_rr, 1, xin, xout, 0, nR, s);
      xin = xout;
      c.rec_base_dim = L.D_out;
    }
    if (xin != c.rec_node_base)
      DDMI_CHECK_HIP(hipMemcpyAsync(c.rec_node_base, xin, (size_t)nR * XS * 4, hipMemcpyDeviceToDevice, s));
  }
}

// =============================================================================== set_complex
void set_complex(Model& m, const ddmi_complex& cc, hipStream_t s) {
  DDMI_REQUIRE(m.committed, DDMI_ERR_STATE, "ddmi_commit_weights must precede ddmi_set_complex");
  DDMI_REQUIRE(cc.num_graphs > 0 && cc.n_lig > 0 && cc.n_rec > 0, DDMI_ERR_ARG, "empty batch");
  DDMI_REQUIRE(cc.lig_ptr && cc.rec_ptr && cc.lig_x && cc.rec_x && cc.rec_pos && cc.rec_edge_index, DDMI_ERR_ARG,
               "null pointer in ddmi_complex");
  DDMI_REQUIRE(cc.n_bond_edges == 0 || (cc.bond_index && cc.bond_attr && cc.edge_mask), DDMI_ERR_ARG, "null bond arrays");
  m.has_complex = false;
  m.cpool.release();
  m.debug.clear();
  m.cx = std::make_shared<Cx>();
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int ns = m.ns, sd = m.sd, H = m.H;
  c.B = cc.num_graphs; c.nL = cc.n_lig; c.nR = cc.n_rec; c.N = c.nL + c.nR; c.Eb = cc.n_bond_edges; c.Err = cc.n_rec_edges;
  if (cfg.all_atoms) {
    DDMI_REQUIRE(cc.n_atom > 0 && cc.atom_ptr && cc.atom_x && cc.atom_pos && cc.atom_edge_index && cc.atom_rec_edge_index,
                 DDMI_ERR_ARG, "all_atoms model: atom arrays missing in ddmi_complex");
    c.nA = cc.n_atom; c.Eaa = cc.n_atom_edges; c.Ear = cc.n_atom_rec_edges;
    c.N = c.nL + c.nR + c.nA;
  }
  c.nT = cfg.no_torsion ? 0 : cc.n_tor;
  c.lig_ptr_h.assign(cc.lig_ptr, cc.lig_ptr + c.B + 1);
  c.rec_ptr_h.assign(cc.rec_ptr, cc.rec_ptr + c.B + 1);
  DDMI_REQUIRE(c.lig_ptr_h[0] == 0 && c.lig_ptr_h[c.B] == c.nL && c.rec_ptr_h[0] == 0 && c.rec_ptr_h[c.B] == c.nR,
               DDMI_ERR_ARG, "lig_ptr / rec_ptr do not span the node arrays");
  DDMI_CHECK_HIP(hipStreamSynchronize(s));
  // ---- topology read-back (one-time)
  std::vector<int> bond_index(2 * (size_t)c.Eb), rr_index(2 * (size_t)c.Err);
  std::vector<unsigned char> edge_mask(c.Eb);
  if (c.Eb) {
    DDMI_CHECK_HIP(hipMemcpy(bond_index.data(), cc.bond_index, bond_index.size() * 4, hipMemcpyDeviceToHost));
    DDMI_CHECK_HIP(hipMemcpy(edge_mask.data(), cc.edge_mask, edge_mask.size(), hipMemcpyDeviceToHost));
  }
  DDMI_CHECK_HIP(hipMemcpy(rr_index.data(), cc.rec_edge_index, rr_index.size() * 4, hipMemcpyDeviceToHost));
  std::vector<int> lig_batch(c.nL), rec_batch(c.nR);
  c.Elr_cap = 0;
  c.uniform = true;
  for (int b = 0; b < c.B; ++b) {
    const int nl = c.lig_ptr_h[b + 1] - c.lig_ptr_h[b], nr = c.rec_ptr_h[b + 1] - c.rec_ptr_h[b];
    DDMI_REQUIRE(nl > 0 && nr > 0, DDMI_ERR_ARG, "graph without ligand or receptor nodes");
    c.maxNl = std::max(c.maxNl, nl); c.maxNr = std::max(c.maxNr, nr);
    c.Elr_cap += nl * nr;
    if (nl != c.lig_ptr_h[1]) c.uniform = false;
    for (int i = c.lig_ptr_h[b]; i < c.lig_ptr_h[b + 1]; ++i) lig_batch[i] = b;
    for (int i = c.rec_ptr_h[b]; i < c.rec_ptr_h[b + 1]; ++i) rec_batch[i] = b;
  }
  c.Ell_cap = c.Eb + c.lig_cap * c.nL;
  // ---- all_atoms: atom batches and the three static atom relations (gather-ordered CSR + target slots)
  std::vector<int> atom_ptr_h, atom_batch, aa_tl, aa_gl, ar_atom, ar_rec, aa_batch_h, ar_batch_h;
  struct HostEdges { std::vector<int> goff, toff, arow, tgt, tslot, tlist, gnode; };
  auto build_static = [&](const std::vector<int>& tl, const std::vector<int>& gl, int n_t, int n_g, int tgt_base) {
    HostEdges h;
    const int E = (int)tl.size();
    h.goff.assign(n_g + 1, 0); h.toff.assign(n_t + 1, 0);
    for (int k = 0; k < E; ++k) {
      DDMI_REQUIRE(tl[k] >= 0 && tl[k] < n_t && gl[k] >= 0 && gl[k] < n_g, DDMI_ERR_ARG, "atom edge index out of range");
      h.goff[gl[k] + 1]++; h.toff[tl[k] + 1]++;
    }
    for (int i = 0; i < n_g; ++i) h.goff[i + 1] += h.goff[i];
    for (int i = 0; i < n_t; ++i) h.toff[i + 1] += h.toff[i];
    h.arow.resize(E); h.tgt.resize(E); h.tslot.resize(E);
    std::vector<int> cur(h.goff.begin(), h.goff.end() - 1), tcur(h.toff.begin(), h.toff.end() - 1);
    for (int k = 0; k < E; ++k) h.arow[cur[gl[k]]++] = k;
    h.tlist.resize(E); h.gnode.resize(E);
    for (int e = 0; e < E; ++e) {
      const int k = h.arow[e];
      h.tgt[e] = tgt_base + tl[k]; h.tslot[e] = tcur[tl[k]]++;
      h.tlist[h.tslot[e]] = e; h.gnode[e] = gl[k];
    }
    return h;
  };
  HostEdges h_aa, h_ar, h_ra;
  if (cfg.all_atoms) {
    atom_ptr_h.assign(cc.atom_ptr, cc.atom_ptr + c.B + 1);
    DDMI_REQUIRE(atom_ptr_h[0] == 0 && atom_ptr_h[c.B] == c.nA, DDMI_ERR_ARG, "atom_ptr does not span the atom array");
    atom_batch.resize(c.nA);
    for (int b = 0; b < c.B; ++b) {
      const int na = atom_ptr_h[b + 1] - atom_ptr_h[b], nl = c.lig_ptr_h[b + 1] - c.lig_ptr_h[b];
      c.maxNa = std::max(c.maxNa, na);
      c.Ela_cap += nl * na;
      for (int i = atom_ptr_h[b]; i < atom_ptr_h[b + 1]; ++i) atom_batch[i] = b;
    }
    std::vector<int> aa_index(2 * (size_t)c.Eaa), ar_index(2 * (size_t)c.Ear);
    DDMI_CHECK_HIP(hipMemcpy(aa_index.data(), cc.atom_edge_index, aa_index.size() * 4, hipMemcpyDeviceToHost));
    DDMI_CHECK_HIP(hipMemcpy(ar_index.data(), cc.atom_rec_edge_index, ar_index.size() * 4, hipMemcpyDeviceToHost));
    aa_tl.assign(aa_index.begin(), aa_index.begin() + c.Eaa); aa_gl.assign(aa_index.begin() + c.Eaa, aa_index.end());
    ar_atom.assign(ar_index.begin(), ar_index.begin() + c.Ear); ar_rec.assign(ar_index.begin() + c.Ear, ar_index.end());
    h_aa = build_static(aa_tl, aa_gl, c.nA, c.nA, c.nL + c.nR);    // atom <- atom
    h_ar = build_static(ar_atom, ar_rec, c.nA, c.nR, c.nL + c.nR);  // atom <- residue  (group "ar", aa_model.py:401-403)
    h_ra = build_static(ar_rec, ar_atom, c.nR, c.nA, c.nL);         // residue <- atom  (flip(ar))
    aa_batch_h.resize(c.Eaa); ar_batch_h.resize(c.Ear);
    for (int k = 0; k < c.Eaa; ++k) aa_batch_h[k] = atom_batch[aa_tl[k]];     // atom.batch[edge_index[0]] (aa_model.py:332)
    for (int k = 0; k < c.Ear; ++k) ar_batch_h[k] = atom_batch[ar_atom[k]];   // (aa_model.py:335)
    // the reference's crop rewrites atom_rec_contact as arange(kept atoms) (utils/utils.py:395-399): defined when edge k belongs to atom k
    c.ar_arange = c.Ear == c.nA;
    for (int k = 0; k < c.Ear && c.ar_arange; ++k) c.ar_arange = ar_atom[k] == k;
  }
  // bonds: ranks inside the gather (edge_index[1]) and target (edge_index[0]) lists
  std::vector<int> bsrc(c.Eb), bdst(c.Eb), bgr(c.Eb), btr(c.Eb), bg(c.nL, 0), bt(c.nL, 0);
  for (int k = 0; k < c.Eb; ++k) {
    bsrc[k] = bond_index[k]; bdst[k] = bond_index[c.Eb + k];
    DDMI_REQUIRE(bsrc[k] >= 0 && bsrc[k] < c.nL && bdst[k] >= 0 && bdst[k] < c.nL, DDMI_ERR_ARG, "bond index out of range");
    bgr[k] = bg[bdst[k]]++;
    btr[k] = bt[bsrc[k]]++;
  }
  std::vector<int> tor_u, tor_v, tor_b;
  for (int k = 0; k < c.Eb && !cfg.no_torsion; ++k)
    if (edge_mask[k]) { tor_u.push_back(bsrc[k]); tor_v.push_back(bdst[k]); tor_b.push_back(lig_batch[bsrc[k]]); }
  DDMI_REQUIRE((int)tor_u.size() == c.nT, DDMI_ERR_ARG, "n_tor does not equal edge_mask.sum()");
  c.tor_ptr_h.assign(c.B + 1, 0);
  for (int t = 0; t < c.nT; ++t) {
    if (t > 0 && tor_b[t] < tor_b[t - 1]) c.tor_sorted = false;
    c.tor_ptr_h[tor_b[t] + 1]++;
    c.tor_lu.push_back(tor_u[t] - c.lig_ptr_h[tor_b[t]]); c.tor_lv.push_back(tor_v[t] - c.lig_ptr_h[tor_b[t]]);
  }
  for (int b = 0; b < c.B; ++b) c.tor_ptr_h[b + 1] += c.tor_ptr_h[b];
  c.Et = c.nT * c.tor_cap;
  std::vector<int> tor_eu(c.Et), tor_ev(c.Et);
  for (int t = 0; t < c.nT; ++t)
    for (int r = 0; r < c.tor_cap; ++r) { tor_eu[t * c.tor_cap + r] = tor_u[t]; tor_ev[t * c.tor_cap + r] = tor_v[t]; }
  // receptor contact graph: gather = edge_index[1], target = edge_index[0]
  std::vector<int> rr_src(c.Err), rr_dst(c.Err), rr_batch(c.Err), goff(c.nR + 1, 0), toff(c.nR + 1, 0);
  for (int k = 0; k < c.Err; ++k) {
    rr_src[k] = rr_index[k]; rr_dst[k] = rr_index[c.Err + k];
    DDMI_REQUIRE(rr_src[k] >= 0 && rr_src[k] < c.nR && rr_dst[k] >= 0 && rr_dst[k] < c.nR, DDMI_ERR_ARG, "receptor edge out of range");
    rr_batch[k] = rec_batch[rr_src[k]];
    goff[rr_dst[k] + 1]++; toff[rr_src[k] + 1]++;
  }
  for (int i = 0; i < c.nR; ++i) { goff[i + 1] += goff[i]; toff[i + 1] += toff[i]; }
  std::vector<int> rr_arow(c.Err), rr_tgt(c.Err), rr_tslot(c.Err), cur(goff.begin(), goff.end() - 1), tcur(toff.begin(), toff.end() - 1);
  for (int k = 0; k < c.Err; ++k) rr_arow[cur[rr_dst[k]]++] = k;
  std::vector<int> rr_tlist(c.Err), rr_gnode(c.Err);
  for (int e = 0; e < c.Err; ++e) {
    const int k = rr_arow[e];
    rr_tgt[e] = c.nL + rr_src[k];
    rr_tslot[e] = tcur[rr_src[k]]++;
    rr_tlist[rr_tslot[e]] = e;
    rr_gnode[e] = rr_dst[k];
  }
  // batch of copies of one receptor (the poses of ddmi_sample): equal residue counts and the contact graph of every graph = graph 0's
  // edge block offset by the graph (features and positions are compared on the device below, the flag read at the final sync)
  bool copies = c.B > 1 && !cfg.all_atoms && !cfg.old_model && c.Err > 0 && c.Err % c.B == 0;
  const int R1 = c.rec_ptr_h[1], E1 = copies ? c.Err / c.B : 0;
  for (int b = 0; b < c.B && copies; ++b) copies = c.rec_ptr_h[b + 1] - c.rec_ptr_h[b] == R1;
  for (int k = 0; k < c.Err && copies; ++k) {
    const int q = k / E1, k0 = k - q * E1;
    copies = rr_src[k] == rr_src[k0] + q * R1 && rr_dst[k] == rr_dst[k0] + q * R1 && rr_src[k0] < R1 && rr_dst[k0] < R1;
  }
  int* rec_differ = nullptr;
  if (copies) {
    c.Rc_one = R1; c.Erc_one = E1;
    rec_differ = dalloc<int>(m, nullptr, {1});
    DDMI_CHECK_HIP(hipMemsetAsync(rec_differ, 0, sizeof(int), s));
    launch_rows_differ(cc.rec_x, 1 + m.lm, cc.rec_pos, 3, R1, c.B, rec_differ, s);
  }
  // ---- uploads
  if (cfg.all_atoms) {
    c.atom_batch = dup(m, "atom_batch", atom_batch); c.atom_ptr = dup(m, nullptr, atom_ptr_h);
    c.atom_x = dalloc<int>(m, nullptr, {c.nA * 4});
    DDMI_CHECK_HIP(hipMemcpy(c.atom_x, cc.atom_x, (size_t)c.nA * 4 * 4, hipMemcpyDeviceToDevice));
    c.atom_pos = dalloc<float>(m, nullptr, {c.nA * 3});
    DDMI_CHECK_HIP(hipMemcpy(c.atom_pos, cc.atom_pos, (size_t)c.nA * 12, hipMemcpyDeviceToDevice));
    auto up_edges = [&](const HostEdges& h, const char* name, const char* crop_name) {
      Cx::StaticEdges e;
      e.E = (int)h.arow.size();
      const int n_g = (int)h.goff.size() - 1, n_t = (int)h.toff.size() - 1;
      e.goff = dup(m, name, h.goff); e.toff = dup(m, nullptr, h.toff); e.arow = dup(m, nullptr, h.arow);
      e.tgt = dup(m, nullptr, h.tgt); e.tslot = dup(m, nullptr, h.tslot);
      e.tlist = dup(m, nullptr, h.tlist); e.gnode = dup(m, nullptr, h.gnode);
      e.cnt_g = dalloc<int>(m, nullptr, {n_g}); e.cnt_t = dalloc<int>(m, nullptr, {n_t});
      e.goff2 = dalloc<int>(m, crop_name, {n_g + 1}); e.toff2 = dalloc<int>(m, nullptr, {n_t + 1});
      e.tslot_tmp = dalloc<int>(m, nullptr, {e.E}); e.tgt2 = dalloc<int>(m, nullptr, {e.E});
      e.tslot2 = dalloc<int>(m, nullptr, {e.E}); e.arow2 = dalloc<int>(m, nullptr, {e.E});
      return e;
    };
    c.se_aa = up_edges(h_aa, "aa_goff", "aa_goff_crop"); c.se_ar = up_edges(h_ar, "ar_goff", "ar_goff_crop");
    c.se_ra = up_edges(h_ra, "ra_goff", "ra_goff_crop");
    c.keep_atom = dalloc<int>(m, "crop_keep_atom", {c.nA});
    if (c.ar_arange) c.atom_res = dup(m, nullptr, ar_rec);
    c.aa_batch = dup(m, nullptr, aa_batch_h); c.ar_batch = dup(m, nullptr, ar_batch_h);
    int* aa_src = dup(m, nullptr, aa_tl); int* aa_dst = dup(m, nullptr, aa_gl);
    int* ar_src = dup(m, nullptr, ar_atom); int* ar_dst = dup(m, nullptr, ar_rec);
    c.aa_dist = dalloc<float>(m, nullptr, {c.Eaa}); c.aa_nvec = dalloc<float>(m, nullptr, {c.Eaa, 3});
    c.aa_ew = cfg.smooth_edges ? dalloc<float>(m, nullptr, {c.Eaa}) : nullptr;
    c.ar_dist = dalloc<float>(m, nullptr, {c.Ear}); c.ar_nvec = dalloc<float>(m, nullptr, {c.Ear, 3});
    c.atom_edge_base = dalloc<float>(m, nullptr, {c.Eaa, ns}); c.ar_edge_base = dalloc<float>(m, nullptr, {c.Ear, ns});
    c.atom_node_base = dalloc<float>(m, "atom_node_base", {c.nA, XS}, true);
    // static geometry: vec = pos[edge_index[1]] - pos[edge_index[0]] (aa_model.py:573-576, 627-629)
    launch_rec_edge_geom(c.atom_pos, aa_src, aa_dst, c.Eaa, cfg.smooth_edges ? cfg.lig_max_radius : 0.f, c.aa_dist, c.aa_nvec,
                         c.aa_ew, s);
    float* rp = dalloc<float>(m, nullptr, {c.nR * 3});
    DDMI_CHECK_HIP(hipMemcpy(rp, cc.rec_pos, (size_t)c.nR * 12, hipMemcpyDeviceToDevice));
    launch_rec_edge_geom(c.atom_pos, ar_src, ar_dst, c.Ear, 0.f, c.ar_dist, c.ar_nvec, nullptr, s, rp);
  }
  c.lig_batch = dup(m, "lig_batch", lig_batch); c.rec_batch = dup(m, "rec_batch", rec_batch);
  c.lig_ptr = dup(m, nullptr, c.lig_ptr_h); c.rec_ptr = dup(m, nullptr, c.rec_ptr_h);
  c.lig_x = dalloc<int>(m, nullptr, {c.nL * 16});
  DDMI_CHECK_HIP(hipMemcpy(c.lig_x, cc.lig_x, (size_t)c.nL * 16 * 4, hipMemcpyDeviceToDevice));
  c.bond_src = dup(m, nullptr, bsrc); c.bond_dst = dup(m, nullptr, bdst); c.bond_grank = dup(m, nullptr, bgr);
  c.bond_trank = dup(m, nullptr, btr); c.bg = dup(m, nullptr, bg); c.bt = dup(m, nullptr, bt);
  c.bond_attr = dalloc<float>(m, nullptr, {c.Eb * m.nf});
  if (c.Eb) DDMI_CHECK_HIP(hipMemcpy(c.bond_attr, cc.bond_attr, (size_t)c.Eb * m.nf * 4, hipMemcpyDeviceToDevice));
  c.tor_u = dup(m, "tor_u", tor_u); c.tor_v = dup(m, "tor_v", tor_v); c.tor_batch = dup(m, nullptr, tor_b);
  c.tor_eu = dup(m, nullptr, tor_eu); c.tor_ev = dup(m, nullptr, tor_ev);
  if (c.uniform && c.nT % c.B == 0) {
    c.Nl_one = c.nL / c.B; c.R_one = c.nT / c.B;
    std::vector<int> ru(tor_u.begin(), tor_u.begin() + c.R_one), rv(tor_v.begin(), tor_v.begin() + c.R_one);
    c.rot_u = dup(m, nullptr, ru); c.rot_v = dup(m, nullptr, rv);
    if (cc.mask_rotate && c.R_one > 0) {
      c.mask_rotate = dalloc<unsigned char>(m, nullptr, {c.R_one * c.Nl_one});
      DDMI_CHECK_HIP(hipMemcpy(c.mask_rotate, cc.mask_rotate, (size_t)c.R_one * c.Nl_one, hipMemcpyDeviceToDevice));
    }
  }
  c.rec_pos = dalloc<float>(m, nullptr, {c.nR * 3});
  DDMI_CHECK_HIP(hipMemcpy(c.rec_pos, cc.rec_pos, (size_t)c.nR * 12, hipMemcpyDeviceToDevice));
  c.rr_src = dup(m, nullptr, rr_src); c.rr_dst = dup(m, nullptr, rr_dst); c.rr_batch = dup(m, nullptr, rr_batch);
  c.rr_goff = dup(m, "rr_goff", goff); c.rr_toff = dup(m, "rr_toff", toff); c.rr_arow = dup(m, nullptr, rr_arow);
  c.rr_tgt = dup(m, nullptr, rr_tgt); c.rr_tslot = dup(m, nullptr, rr_tslot);
  c.rr_tlist = dup(m, nullptr, rr_tlist); c.rr_gnode = dup(m, nullptr, rr_gnode);
  c.keep = dalloc<int>(m, "crop_keep", {c.nR}); c.cnt_g2 = dalloc<int>(m, nullptr, {c.nR}); c.cnt_t2 = dalloc<int>(m, nullptr, {c.nR});
  c.goff2 = dalloc<int>(m, "rr_goff_crop", {c.nR + 1}); c.toff2 = dalloc<int>(m, nullptr, {c.nR + 1});
  c.tslot_tmp = dalloc<int>(m, nullptr, {c.Err}); c.tgt2 = dalloc<int>(m, nullptr, {c.Err});
  c.tslot2 = dalloc<int>(m, nullptr, {c.Err}); c.arow2 = dalloc<int>(m, nullptr, {c.Err});
  // ---- workspace
  const int B = c.B, nL = c.nL, nR = c.nR, N = c.N;
  c.rr_dist = dalloc<float>(m, nullptr, {c.Err}); c.rr_nvec = dalloc<float>(m, nullptr, {c.Err, 3});
  c.rr_ew = cfg.smooth_edges ? dalloc<float>(m, nullptr, {c.Err}) : nullptr;
  c.rec_edge_base = dalloc<float>(m, "rec_edge_base", {c.Err, ns});
  c.rec_node_base = dalloc<float>(m, "rec_node_base", {nR, XS}, true);
  c.temb = dalloc<float>(m, "temb", {B, sd}); c.hidB = dalloc<float>(m, nullptr, {B, std::max(ns, H)});
  c.rec_sig = dalloc<float>(m, "rec_sig", {B, ns}); c.ligsig = dalloc<float>(m, nullptr, {B, ns});
  c.ll_gvec = dalloc<float>(m, nullptr, {B, ns}); c.cross_gvec = dalloc<float>(m, nullptr, {B, ns});
  c.center_gvec = dalloc<float>(m, nullptr, {B, ns}); c.tr_sig = dalloc<float>(m, nullptr, {B, ns});
  c.rr_sig_old = dalloc<float>(m, nullptr, {B, ns});
  if (cfg.old_model && cfg.all_atoms) {
    c.atom_sig = dalloc<float>(m, nullptr, {B, ns}); c.aa_sig_old = dalloc<float>(m, nullptr, {B, ns});
    c.ar_sig_old = dalloc<float>(m, nullptr, {B, ns});
  }
  if (cfg.atom_confidence && cfg.confidence_mode) {
    c.ac_in = dalloc<float>(m, nullptr, {nL, 2 * ns}); c.ac_h0 = dalloc<float>(m, nullptr, {nL, ns});
    c.ac_h1 = dalloc<float>(m, nullptr, {nL, ns}); c.ac_out = dalloc<float>(m, nullptr, {nL, cfg.atom_num_confidence_outputs + ns});
  }
  c.rot_sig = dalloc<float>(m, nullptr, {B, ns}); c.cutoff = dalloc<float>(m, "cross_cutoff", {B});
  c.rr_rowbias = dalloc<float>(m, nullptr, {B, H});
  c.embsum = dalloc<float>(m, nullptr, {nL, ns});
  // node tables: one per layer boundary (+ two update tables for the legacy class, whose four layers are summed afterwards)
  const int n_layers = cfg.old_model ? cfg.num_conv_layers + 2 : (int)m.conv_layers.size(), K = (int)m.lig_emb_layers.size();
  for (int l = 0; l <= n_layers + K; ++l) {
    static const char* names[] = {"x0", "x1", "x2", "x3", "x4", "x5", "x6", "x7", "x8", "x9", "x10", "x11", "x12"};
    c.X.push_back(dalloc<float>(m, l < 13 ? names[l] : nullptr, {N, XS}, true));
  }
  c.adjrank = dalloc<int>(m, nullptr, {nL, c.maxNl}); c.cnt_g = dalloc<int>(m, nullptr, {nL}); c.cnt_t = dalloc<int>(m, nullptr, {nL});
  c.goff_ll = dalloc<int>(m, "goff_ll", {nL + 1}); c.toff_ll = dalloc<int>(m, "toff_ll", {nL + 1});
  c.ll_tgt = dalloc<int>(m, "ll_tgt", {c.Ell_cap}); c.ll_tslot = dalloc<int>(m, nullptr, {c.Ell_cap});
  c.ll_featidx = dalloc<int>(m, nullptr, {c.Ell_cap}); c.ll_batch = dalloc<int>(m, nullptr, {c.Ell_cap});
  c.ll_dist = dalloc<float>(m, "ll_dist", {c.Ell_cap}); c.ll_nvec = dalloc<float>(m, nullptr, {c.Ell_cap, 3});
  c.ll_ew = cfg.smooth_edges ? dalloc<float>(m, nullptr, {c.Ell_cap}) : nullptr;
  c.ll_ea = dalloc<float>(m, "ll_ea", {c.Ell_cap, ns});
  c.pairrank = dalloc<int>(m, nullptr, {nL, c.maxNr}); c.cnt_l = dalloc<int>(m, nullptr, {nL}); c.cnt_r = dalloc<int>(m, nullptr, {nR});
  c.offs_l = dalloc<int>(m, "offs_l", {nL + 1}); c.offs_r = dalloc<int>(m, "offs_r", {nR + 1});
  c.g1_tgt = dalloc<int>(m, nullptr, {c.Elr_cap}); c.g1_tslot = dalloc<int>(m, nullptr, {c.Elr_cap});
  c.g3_tgt = dalloc<int>(m, nullptr, {c.Elr_cap}); c.g3_tslot = dalloc<int>(m, nullptr, {c.Elr_cap});
  c.pbatch = dalloc<int>(m, nullptr, {c.Elr_cap}); c.pdist = dalloc<float>(m, "cross_dist", {c.Elr_cap});
  c.pnvec = dalloc<float>(m, nullptr, {c.Elr_cap, 3}); c.pew = cfg.smooth_edges ? dalloc<float>(m, nullptr, {c.Elr_cap}) : nullptr;
  c.cross_ea = dalloc<float>(m, "cross_ea", {c.Elr_cap, ns});
  const int max_rows = std::max(std::max(std::max(c.Ell_cap, c.Elr_cap), std::max(c.Err, c.Eaa)), std::max(c.Ear, c.Ela_cap));
  c.HE = dalloc<float>(m, nullptr, {max_rows, H}); c.P = dalloc<float>(m, nullptr, {N, H}); c.Q = dalloc<float>(m, nullptr, {N, H});
  c.HE_b = dalloc<float>(m, nullptr, {std::max(std::max(c.Ell_cap, c.Elr_cap), c.Ela_cap), H}); c.P_b = dalloc<float>(m, nullptr, {N, H});
  c.Q_b = dalloc<float>(m, nullptr, {N, H}); c.rowbias_b = dalloc<float>(m, nullptr, {B, H});
  if (cfg.tp_weights_layers > 2) {   // per-edge hidden rows of the deeper edge MLP (ping-pong), main and side stream
    for (int i = 0; i < 2; ++i) {
      c.HD[i] = dalloc<float>(m, nullptr, {max_rows, H});
      c.HD_b[i] = dalloc<float>(m, nullptr, {std::max(std::max(c.Ell_cap, c.Elr_cap), c.Ela_cap), H});
    }
  }
  for (int i = 0; i < (cfg.all_atoms ? 9 : 4); ++i) {
    c.Pg[i] = dalloc<float>(m, nullptr, {N, H}); c.Qg[i] = dalloc<float>(m, nullptr, {N, H}); c.rbg[i] = dalloc<float>(m, nullptr, {B, H});
  }
  for (size_t l = 0; l < m.conv_layers.size(); ++l) c.rb_l.push_back(dalloc<float>(m, nullptr, {B, H}));
  std::vector<const ConvW*> all_layers;
  for (auto* fam : {&m.conv_layers, &m.lig_emb_layers, &m.rec_emb_layers, &m.old_lig, &m.old_rec, &m.old_l2r, &m.old_r2l, &m.old_aa})
    for (auto& L : *fam) all_layers.push_back(&L);
  {
    int HKq = 0;
    for (auto* L : all_layers) HKq = std::max(HKq, L->HKq);
    // virtual-node lists: 0 lig<-rec, 1 rec-rec, 2 lig-lig, 3 rec<-lig; all_atoms: 4 lig<-atom, 5 rec<-atom, 6 atom-atom,
    // 7 atom<-lig, 8 atom<-rec; 9 rec-rec of graph 0 (batch of receptor copies, exec.rec_share).  (lig_v: lists of the side-stream
    // groups, which use the second hidden-row scratch.)
    const int ecap_v[10] = {c.Elr_cap, c.Err, c.Ell_cap, c.Elr_cap, c.Ela_cap, c.Ear, c.Eaa, c.Ela_cap, c.Ear, E1};
    const int gn_v[10] = {nR, nR, nL, nL, c.nA, c.nA, c.nA, nL, nR, R1};
    const bool lig_v[10] = {false, false, true, true, false, false, false, true, false, false};
    const char* names[10] = {"vn_off_cross", "vn_off_rr", "vn_off_ll", "vn_off_rl", "vn_off_la", "vn_off_ra", "vn_off_aa",
                             "vn_off_al", "vn_off_ar", "vn_off_rr0"};   // (vn_off_rr0 stays zero until the shared layer-0 group has run: tests)
    // Tight capacities (round 6, exec.list_caps = 1; NOT the default: neutral at 5-20 poses, -1.8 % at 40, profiles/r06_p12_*): the grids of k_conv_fused / k_vn_rows cover the CAPACITY of a list, and a workgroup whose tile does
    // not exist still has to be placed on a CU with 125-158 KB of free LDS before it can exit -- the generic bound
    // nodes + edges / 32 is twice the live count for the all-pairs cross graph (a residue's <= n_lig edges are ONE virtual node).
    // Per gather node the largest possible degree is known on the host: the other side's node count of its graph for the dynamic
    // pair graphs, the exact degree for the static relations (a crop only removes edges), neighbour cap + bonds for lig-lig.
    long tight[10];
    for (int i = 0; i < 10; ++i) tight[i] = -1;
    auto vn_of = [](long deg) { return (deg + 31) / 32; };
    auto exact = [&](const std::vector<int>& off) { long n = 0; for (size_t d = 0; d + 1 < off.size(); ++d) n += vn_of(off[d + 1] - off[d]); return n; };
    tight[0] = tight[3] = 0;
    for (int b = 0; b < B; ++b) {
      const long nl = c.lig_ptr_h[b + 1] - c.lig_ptr_h[b], nr = c.rec_ptr_h[b + 1] - c.rec_ptr_h[b];
      tight[0] += nr * vn_of(nl);     // lig<-rec: gather = residue, at most one edge to every ligand atom of its graph
      tight[3] += nl * vn_of(nr);     // rec<-lig: gather = ligand atom
    }
    tight[1] = exact(goff);           // rec-rec (static; the per-step crop compacts it)
    if (copies) tight[9] = exact(std::vector<int>(goff.begin(), goff.begin() + R1 + 1));   // rec-rec of graph 0
    tight[2] = 0;
    for (int d = 0; d < nL; ++d) tight[2] += vn_of((long)c.lig_cap + bg[d]);   // lig-lig: <= lig_cap radius neighbours + its bonds
    if (cfg.all_atoms) {
      tight[4] = tight[7] = 0;
      for (int b = 0; b < B; ++b) {
        const long nl = c.lig_ptr_h[b + 1] - c.lig_ptr_h[b], na = atom_ptr_h[b + 1] - atom_ptr_h[b];
        tight[4] += na * vn_of(nl);   // lig<-atom: gather = receptor atom
        tight[7] += nl * vn_of(na);   // atom<-lig: gather = ligand atom
      }
      tight[5] = exact(h_ra.goff); tight[6] = exact(h_aa.goff); tight[8] = exact(h_ar.goff);
    }
    int vmax = 0, vmax_b = 0;
    for (int i = 0; i < 10; ++i) {
      if (i < 9 ? i >= (cfg.all_atoms ? 9 : 4) : !copies) continue;
      Cx::VnSet& vs = c.vn[i];
      vs.graphs = i == 9 ? 1 : B;
      vs.vcap = gn_v[i] + ecap_v[i] / 32 + 2;   // a gather node with deg edges: ceil(deg / 32) <= deg / 32 + 1 virtual nodes
      if (m.r.list_caps && tight[i] >= 0) vs.vcap = (int)std::min<long>(vs.vcap, tight[i] + 2);
      if (m.r.tile_per_pose) {                    // every graph padded to whole 16-node tiles
        vs.vcap += 16 * vs.graphs;
        vs.nvn_pad = dalloc<int>(m, i == 0 ? "vn_count_cross" : nullptr, {1}, true);
      }
      vs.cnt = dalloc<int>(m, nullptr, {gn_v[i] + 1}); vs.voff = dalloc<int>(m, names[i], {gn_v[i] + 1}, i == 9);
      vs.node = dalloc<int>(m, nullptr, {vs.vcap}); vs.e0 = dalloc<int>(m, nullptr, {vs.vcap});
      const int shd = (cfg.sh_lmax + 1) * (cfg.sh_lmax + 1);
      vs.ne = dalloc<int>(m, i == 0 ? "vn_ne_cross" : nullptr, {round_up(vs.vcap, 16)});   // (named: bench.py counts the message rows a pre-reducing launch writes)
      vs.rows = dalloc<float>(m, nullptr, {round_up(vs.vcap, 16), 32, shd == 4 ? 8 : shd + 3});
      if (i == 0) {
        // in-tile pre-reduction of the lig<-rec messages: every interaction layer must run the static l <= 1 kernel variants
        c.prered = m.r.pre_reduce && shd == 4 && !cfg.old_model && !m.conv_layers.empty() && m.r.shared_tiles != Use::always;   // (shared == 2: test mode, mode-4 tiles everywhere)
        for (auto& L : m.conv_layers) c.prered = c.prered && !L.fgran_generic && L.maxd <= 3 && L.n_fgran > 0;
        if (c.prered) {
          vs.tile_hdr = dalloc<int>(m, "prered_tile_hdr", {round_up(vs.vcap, 16) / 16, FC_TILE_HDR}, true);
          vs.live = dalloc<unsigned char>(m, nullptr, {ecap_v[0]}, true);
        }
      }
      vmax = std::max(vmax, vs.vcap);
      if (lig_v[i]) vmax_b = std::max(vmax_b, vs.vcap);
    }
    c.Hb = HKq > 0 ? dalloc<float>(m, nullptr, {round_up(vmax, 16), 32, round_up(HKq, 16)}) : nullptr;   // whole 16-node tiles, whole pairs of 8-k groups
    if (m.r.grouped == 2 && HKq > 0)
      for (int i = 0; i < (cfg.all_atoms ? 9 : 4); ++i) c.Hbg[i] = dalloc<float>(m, nullptr, {round_up(c.vn[i].vcap, 16), 32, round_up(HKq, 16)});
    c.Hb_b = HKq > 0 ? dalloc<float>(m, nullptr, {round_up(vmax_b, 16), 32, round_up(HKq, 16)}) : nullptr;
  }
  alloc_messages(m, copies, R1);
  alloc_readouts(m);
  receptor_constants(m, cc, rr_tgt, s);
  DDMI_CHECK_HIP(hipStreamSynchronize(s));
  if (rec_differ) {   // (the stream has just drained: no extra wait)
    int differ = 1;
    DDMI_CHECK_HIP(hipMemcpy(&differ, rec_differ, sizeof(int), hipMemcpyDeviceToHost));
    c.rec_copies = differ == 0;
  }
  m.has_complex = true;
}

void set_batch_layout(Model& m, const ddmi_batch_layout& l, hipStream_t s) {
  DDMI_REQUIRE(l.struct_size == sizeof(ddmi_batch_layout), DDMI_ERR_ARG, "ddmi_batch_layout.struct_size does not match this library");
  DDMI_REQUIRE(m.has_complex, DDMI_ERR_STATE, "ddmi_set_complex must precede ddmi_set_batch_layout");
  Cx& c = *m.cx;
  const int G = l.num_groups;
  DDMI_REQUIRE(G >= 1 && G <= c.B && l.group_ptr, DDMI_ERR_ARG, "need 1..num_graphs groups and group_ptr");
  DDMI_REQUIRE(l.group_ptr[0] == 0 && l.group_ptr[G] == c.B, DDMI_ERR_ARG, "group_ptr must run from 0 to num_graphs");
  for (int g = 0; g < G; ++g) DDMI_REQUIRE(l.group_ptr[g + 1] > l.group_ptr[g], DDMI_ERR_ARG, "empty or decreasing group in group_ptr");
  DDMI_REQUIRE(c.tor_sorted, DDMI_ERR_ARG, "the rotatable bonds (edge_mask) are not in graph order");
  std::vector<long long> mask_off(c.B);
  long long bytes = 0;
  for (int b = 0; b < c.B; ++b) {
    mask_off[b] = bytes;
    bytes += (long long)(c.tor_ptr_h[b + 1] - c.tor_ptr_h[b]) * (c.lig_ptr_h[b + 1] - c.lig_ptr_h[b]);
  }
  DDMI_REQUIRE(l.mask_rotate_bytes == bytes, DDMI_ERR_ARG,
               "mask_rotate_bytes = " + std::to_string(l.mask_rotate_bytes) + ", the graphs' [R_b, Nl_b] blocks take " + std::to_string(bytes));
  DDMI_REQUIRE(bytes == 0 || l.mask_rotate, DDMI_ERR_ARG, "the batch has rotatable bonds: mask_rotate is required");
  DDMI_CHECK_HIP(hipStreamSynchronize(s));   // the previous layout may still be read by enqueued steps
  if (!c.grp_ptr) {   // per-complex parts: uploaded once, the groups and the mask are rewritten by every call
    c.grp_ptr = dalloc<int>(m, "layout_group_ptr", {c.B + 1});
    c.tor_ptr = dup(m, "layout_tor_ptr", c.tor_ptr_h);
    c.rot_lu = dup(m, nullptr, c.tor_lu); c.rot_lv = dup(m, nullptr, c.tor_lv);
    c.mask_off = dup(m, nullptr, mask_off);
    if (bytes) c.mask_all = dalloc<unsigned char>(m, nullptr, {bytes});
  }
  DDMI_CHECK_HIP(hipMemcpy(c.grp_ptr, l.group_ptr, (size_t)(G + 1) * sizeof(int), hipMemcpyHostToDevice));
  if (bytes) DDMI_CHECK_HIP(hipMemcpy(c.mask_all, l.mask_rotate, (size_t)bytes, hipMemcpyDeviceToDevice));
  c.layout = true; c.G = G;
  c.rec_on = false;   // a record's nan_count rows were sized for the groups of before: set it again behind the layout
}

}  // namespace ddmi
