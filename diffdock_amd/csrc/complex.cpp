// Orchestration of the score-model forward pass and the reverse-diffusion loop for one
// collated batch (reference CGModel.forward models/cg_model.py:308-424, sampling()
// utils/sampling.py:96-191).  Everything is enqueued on the caller's stream; the only host
// synchronisation is inside set_complex (one-time topology read-back).
#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <cstdlib>

#include "model.h"

namespace ddmi {

struct Model::Cx {
  int B = 0, nL = 0, nR = 0, N = 0, Eb = 0, Err = 0, nT = 0;
  int maxNl = 0, maxNr = 0, Ell_cap = 0, Elr_cap = 0, tor_cap = 32, Et = 0, lig_cap = 33;
  bool uniform = false; int Nl_one = 0, R_one = 0;
  // every graph's receptor is a bitwise copy of graph 0's (node count, features, positions, contact graph offset by the graph):
  // under one t for all graphs the layer-0 rec-rec messages are the same for every graph (forward, exec.rec_share)
  bool rec_copies = false; int Rc_one = 0, Erc_one = 0;   // residues / rec-rec edges of one copy
  ReduceGroup* rg_all_share = nullptr;                    // rg_all with the rec-rec entry folded onto graph 0 (tmod = Rc_one)
  // torsions per graph (host, from edge_mask): graph b owns [tor_ptr_h[b], tor_ptr_h[b+1]) when tor_sorted; graph-local atom indices
  std::vector<int> tor_ptr_h, tor_lu, tor_lv; bool tor_sorted = true;
  // ddmi_set_batch_layout: NaN-guard groups and per-graph masks of a batch of different complexes (layout = false: copies of graph 0)
  bool layout = false; int G = 1;
  int *grp_ptr = nullptr, *tor_ptr = nullptr, *rot_lu = nullptr, *rot_lv = nullptr; long long* mask_off = nullptr;
  unsigned char* mask_all = nullptr;
  std::vector<int> lig_ptr_h, rec_ptr_h;
  // static
  int *lig_batch, *rec_batch, *lig_ptr, *rec_ptr, *lig_x;
  int *bond_src, *bond_dst, *bond_grank, *bond_trank, *bg, *bt; float* bond_attr;
  int *tor_u, *tor_v, *tor_batch, *tor_eu, *tor_ev, *rot_u, *rot_v; unsigned char* mask_rotate = nullptr;
  float* rec_pos; int *rr_src, *rr_dst, *rr_batch; float *rr_dist, *rr_nvec, *rr_ew, *rec_edge_base;
  int *rr_goff, *rr_tgt, *rr_tslot, *rr_arow, *rr_toff, *rr_tlist, *rr_gnode;
  // per-step cropped receptor graph
  int *keep, *cnt_g2, *cnt_t2, *goff2, *toff2, *tslot_tmp, *tgt2, *tslot2, *arow2;
  ReduceGroup *rg_all_crop, *rg_rr_crop;
  float* rec_node_enc;   // receptor encoder output before the embedding layers
  float* rec_node_base; int rec_base_dim = 0;
  // per forward
  float *temb, *hidB, *rec_sig, *ligsig, *ll_gvec, *cross_gvec, *center_gvec, *tr_sig, *rot_sig, *cutoff, *rr_rowbias;
  float *ac_in = nullptr, *ac_h0 = nullptr, *ac_h1 = nullptr, *ac_out = nullptr;   // atom_confidence_predictor activations [nL, .]
  float* rr_sig_old = nullptr;   // legacy classes: sigma term of the receptor edge embedding (old_cg_model.py:411-413)
  float* embsum;
  std::vector<float*> X;
  int *adjrank, *cnt_g, *cnt_t, *goff_ll, *toff_ll, *ll_tgt, *ll_tslot, *ll_featidx, *ll_batch;
  float *ll_dist, *ll_nvec, *ll_ew, *ll_ea;
  int *pairrank, *cnt_l, *cnt_r, *offs_l, *offs_r, *g1_tgt, *g1_tslot, *g3_tgt, *g3_tslot, *pbatch;
  float *pdist, *pnvec, *pew, *cross_ea;
  float *HE, *P, *Q; float* msg[4];
  const float* x_last = nullptr;   // node table behind the last interaction layer of the last forward (sidechain_pred)
  float *HE_b, *P_b, *Q_b, *rowbias_b;   // second scratch set: ligand-gather groups on the side stream
  float *Pg[9] = {}, *Qg[9] = {}, *rbg[9] = {};   // per-group first-layer terms when a layer's GEMMs go out in one launch (run_conv)
  // fused form (k_conv_fused): virtual-node lists of the two receptor-gather topologies (0 = lig<-rec cross, 1 = rec-rec),
  // rebuilt when the edge list they were built for changes (once per forward), and the hidden-row scratch
  struct VnSet { int vcap = 0; int *cnt = nullptr, *voff = nullptr, *node = nullptr, *e0 = nullptr, *ne = nullptr;
                 float* rows = nullptr;   // per-edge rows of k_conv_fused (k_vn_rows)
                 int* tile_hdr = nullptr; unsigned char* live = nullptr;   // in-tile pre-reduction (launch_vn_tiles): tile headers, rows that get written
                 int* nvn_pad = nullptr;   // tile_per_pose: length of the list with every graph padded to whole tiles (else voff[gcount])
                 int graphs = 0;           // graphs the gather nodes of the list span (tile_per_pose padding)
                 // what the lists and per-edge rows were built from (k_vn_rows bakes target slots, attribute rows, harmonics with
                 // their sign and edge weights in): a group that reuses a list id with any other input rebuilds it
                 const int *built_goff = nullptr, *built_tgt = nullptr, *built_tslot = nullptr, *built_arow = nullptr;
                 const float *built_nvec = nullptr, *built_ew = nullptr; float built_sgn = 0.f; int built_tbase = -1; long epoch = -1; };
  bool prered = false;   // the lig<-rec group (list 0) leaves one message row per (tile, target) instead of one per edge
  VnSet vn[10];          // + 2 = ligand-ligand, 3 = rec<-lig (ligand gather nodes); all_atoms: 4 la, 5 ra, 6 aa, 7 al, 8 ar;
                         // 9 = rec-rec of graph 0 only (rec_copies)
  // ---- all_atoms (models/aa_model.py): receptor heavy atoms = third node type, node rows [nL + nR, N)
  int nA = 0, maxNa = 0, Eaa = 0, Ear = 0, Ela_cap = 0;
  int *atom_batch = nullptr, *atom_ptr = nullptr, *atom_x = nullptr;
  float* atom_pos = nullptr;
  struct StaticEdges { int E = 0; int *goff = nullptr, *toff = nullptr, *arow = nullptr, *tgt = nullptr, *tslot = nullptr; };
  StaticEdges se_aa, se_ar, se_ra;   // atom<-atom; atom<-rec (group "ar"); rec<-atom (the flipped group)
  int *aa_batch = nullptr, *ar_batch = nullptr;
  float *aa_dist = nullptr, *aa_nvec = nullptr, *aa_ew = nullptr, *atom_edge_base = nullptr;
  float *ar_dist = nullptr, *ar_nvec = nullptr, *ar_edge_base = nullptr, *atom_node_base = nullptr;
  int *la_pairrank = nullptr, *la_cnt_l = nullptr, *la_cnt_a = nullptr, *la_offs_l = nullptr, *la_offs_a = nullptr;
  int *la1_tgt = nullptr, *la1_tslot = nullptr, *la3_tgt = nullptr, *la3_tslot = nullptr, *la_pbatch = nullptr;
  float *la_dist = nullptr, *la_nvec = nullptr, *la_ew = nullptr, *la_ea = nullptr, *la_gvec = nullptr;
  float* msg_aa[9] = {};
  ReduceGroup *rg_aa_all = nullptr, *rg_aa_lig = nullptr;
  long epoch = 0;
  float *Hb = nullptr, *Hb_b = nullptr;   // hidden rows of the main-stream / side-stream group in flight
  std::vector<float*> rb_l;                 // fused node-update route: per-graph first-Linear term of the rec-rec group of every interaction layer [B][H]
  float* Hbg[9] = {};                       // grouped dispatch: hidden rows of every virtual-node list (all groups of a layer are in flight at once)
  float *HD[2] = {nullptr, nullptr}, *HD_b[2] = {nullptr, nullptr};   // tp_weights_layers > 2: plain per-edge hidden rows [E][H]
  ReduceGroup *rg_all, *rg_lig, *rg_ll, *rg_rr;
  // read-outs
  float *c_dist, *c_nvec, *c_ea, *c_attr, *c_hid, *c_W, *c_sh, *c_out, *gp;
  int* c_xrow;
  int *t_cnt, *t_atom; float *t_dist, *t_nvec, *t_ew, *t_bond_nvec, *t_ea, *t_attr, *t_hid, *t_W, *t_sh, *t_out, *t_feat;
  // sampler
  float *s_tr, *s_rot, *s_tor, *s_t = nullptr; long long* s_ids = nullptr;
  long long* s_ids_host = nullptr; hipEvent_t s_ids_ev = nullptr;   // pinned staging of the sample ids
  ~Cx() { if (s_ids_host) (void)hipHostFree(s_ids_host); if (s_ids_ev) (void)hipEventDestroy(s_ids_ev); }
};

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

namespace {

typedef Model::Cx Cx;

template <class T> T* dalloc(Model& m, const char* name, std::vector<int64_t> shape, bool zero = false) {
  size_t n = 1;
  for (auto d : shape) n *= (size_t)std::max<int64_t>(d, 0);
  T* p = m.cpool.alloc<T>(n ? n : 1);
  if (zero) DDMI_CHECK_HIP(hipMemset(p, 0, (n ? n : 1) * sizeof(T)));
  if (name) m.debug[name] = DebugEntry{p, shape, !std::is_same<T, float>::value};
  return p;
}
template <class T> T* dup(Model& m, const char* name, const std::vector<T>& v) {
  T* p = m.cpool.upload(v);
  if (name) m.debug[name] = DebugEntry{p, {(int64_t)v.size()}, !std::is_same<T, float>::value};
  return p;
}

void gemm(const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc, int M, int N, int K,
          int act, hipStream_t s, const int* m_dev = nullptr, const float* rowbias = nullptr, const int* ridx = nullptr,
          int ldrb = 0) {
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.act = act;
  g.m_dev = m_dev; g.rowbias = rowbias; g.ridx = ridx; g.ldrb = ldrb;
  launch_gemm(g, s);
}

struct RunGroup {
  int gbase, gcount, tbase, tcount;
  const int *goff, *tgt, *tslot, *arow;
  const float* ea; int ea_rows; const int* ea_rows_dev;
  const float* sig; const int* sig_idx;   // optional per-graph vector [B][ns] added to every edge attr row
  const float *nvec, *ew; float sgn;
  float* msg;
  int vn = -1;     // >= 0: virtual-node list id -> eligible for the fused kernel
  bool load = false;   // gather nodes are ligand atoms (few nodes, possibly many edges each): candidates for the shared-node tiles of k_conv_fused
  bool swap_pq = false;   // first Linear sees [edge, GATHER node, TARGET node] (legacy lig->rec layer, old_cg_model.py:263)
  const float* rb_ready = nullptr;   // per-graph term W1e . sig of THIS layer already computed ([B][H]; fused node-update route)
  bool static_topo = false;   // edges, geometry and slots are per-complex constants (rec-rec without a crop, the atom relations): lists built once
};

// tiles of 16 virtual nodes of an edge group ~ gather nodes x ceil(mean degree / 32) / 16; a SMALL layer = no group fills the chip once
static long tiles_of(const RunGroup& q) {
  const long gn = std::max(1, q.gcount);
  return std::max(1L, gn * (((long)q.ea_rows / gn + 31) / 32) / 16);
}

// Virtual-node lists and per-edge rows of an edge group (k_vn_count -> scan -> k_vn_fill -> k_vn_rows [-> k_vn_tiles]): built on the
// first use in a forward, rebuilt when any input they bake in changes.
static bool vn_fresh(const Cx& c, const RunGroup& g) {
  const Cx::VnSet& vs = c.vn[g.vn];
  return vs.built_goff == g.goff && (vs.epoch == c.epoch || (g.static_topo && vs.epoch >= 0)) && vs.built_tgt == g.tgt && vs.built_tslot == g.tslot &&
         vs.built_arow == g.arow && vs.built_nvec == g.nvec && vs.built_ew == g.ew && vs.built_sgn == g.sgn && vs.built_tbase == g.tbase;
}
static void vn_mark_built(Cx& c, const RunGroup& g) {
  Cx::VnSet& vs = c.vn[g.vn];
  vs.built_goff = g.goff; vs.epoch = c.epoch; vs.built_tgt = g.tgt; vs.built_tslot = g.tslot; vs.built_arow = g.arow;
  vs.built_nvec = g.nvec; vs.built_ew = g.ew; vs.built_sgn = g.sgn; vs.built_tbase = g.tbase;
}
static VnRowsArgs vn_rows_args(const Model& m, const RunGroup& g) {
  const Cx::VnSet& vs = m.cx->vn[g.vn];
  VnRowsArgs vr{};
  vr.arow = g.arow; vr.nvec = g.nvec; vr.ew = g.ew; vr.tslot = g.tslot; vr.sgn = g.sgn; vr.sh_lmax = m.cfg.sh_lmax;
  vr.tgt = g.tgt; vr.tbase = g.tbase;
  vr.vcap = vs.vcap; vr.rows = vs.rows; vr.vn_ne = vs.ne;
  return vr;
}
static const char vn_type[10] = {'R', 'R', 'L', 'L', 'A', 'A', 'A', 'L', 'R', 'R'};   // gather-node type of every virtual-node list (set_complex)
// the stale lists of a layer's groups in two launches (+ the tile headers of the pre-reduced group)
static void ensure_vn_all(Model& m, const std::vector<RunGroup>& groups, hipStream_t gs) {
  Cx& c = *m.cx;
  VnListsArgs LA;
  VnRowsArgs rows[VN_GROUPS_MAX];
  const RunGroup* built[VN_GROUPS_MAX];
  const RunGroup* prered_g = nullptr;
  for (auto& g : groups) {
    if (vn_fresh(c, g) || g.gcount <= 0) continue;
    bool queued = false;   // (a list is built once per launch even if two groups name it)
    for (int i = 0; i < LA.n; ++i) queued = queued || built[i]->vn == g.vn;
    if (queued) continue;
    DDMI_REQUIRE(LA.n < VN_GROUPS_MAX, DDMI_ERR_CAPACITY, "more edge groups than virtual-node list slots");
    Cx::VnSet& vs = c.vn[g.vn];
    VnListArgs& a = LA.g[LA.n];
    a = VnListArgs{g.goff, g.gcount, vs.voff, vs.node, vs.e0, nullptr, nullptr, 0, nullptr};
    if (vs.nvn_pad) {
      const bool lig = vn_type[g.vn] == 'L', atom = vn_type[g.vn] == 'A';
      a.node_batch = lig ? c.lig_batch : atom ? c.atom_batch : c.rec_batch;
      a.graph_ptr = lig ? c.lig_ptr : atom ? c.atom_ptr : c.rec_ptr;
      a.n_graphs = vs.graphs; a.nvn_pad = vs.nvn_pad;
    }
    rows[LA.n] = vn_rows_args(m, g);
    if (g.vn == 0 && c.prered) {
      prered_g = &g;
      if (m.cfg.sh_lmax <= 1) { rows[LA.n].tile_hdr = vs.tile_hdr; rows[LA.n].live = vs.live; }   // headers from the rows' own launch
    }
    built[LA.n++] = &g;
  }
  if (LA.n == 0) return;
  PhaseTimer t(m, "vn_build", gs);
  launch_vn_build_all(LA, rows, m.cfg.sh_lmax, gs);
  if (prered_g && m.cfg.sh_lmax > 1) {
    Cx::VnSet& vs = c.vn[0];
    launch_vn_tiles(vs.nvn_pad ? vs.nvn_pad : vs.voff + prered_g->gcount, vs.vcap, vs.rows, vs.ne, vs.tile_hdr, vs.live, gs);
  }
  for (int i = 0; i < LA.n; ++i) vn_mark_built(c, *built[i]);   // only once every launch went out (a throw leaves the lists stale)
}
static void ensure_vn(Model& m, const RunGroup& g, hipStream_t gs) {
  Cx& c = *m.cx;
  Cx::VnSet& vs = c.vn[g.vn];
  if (vn_fresh(c, g)) return;
  PhaseTimer t(m, "vn_build", gs);
  const VnRowsArgs vr = vn_rows_args(m, g);
  VnPoseTiles pp{};
  if (vs.nvn_pad) {   // graph of every gather node: ligand / receptor / atom rows of the node table
    const bool lig = vn_type[g.vn] == 'L', atom = vn_type[g.vn] == 'A';
    pp.node_batch = lig ? c.lig_batch : atom ? c.atom_batch : c.rec_batch;
    pp.graph_ptr = lig ? c.lig_ptr : atom ? c.atom_ptr : c.rec_ptr;
    pp.n_graphs = vs.graphs; pp.nvn_pad = vs.nvn_pad;
  }
  launch_vn_build(g.goff, g.gcount, vs.cnt, vs.voff, vs.node, vs.e0, vr, gs, vs.nvn_pad ? &pp : nullptr);
  if (g.vn == 0 && c.prered) launch_vn_tiles(vs.nvn_pad ? vs.nvn_pad : vs.voff + g.gcount, vs.vcap, vs.rows, vs.ne, vs.tile_hdr, vs.live, gs);
  vn_mark_built(c, g);
}

// row mode / arithmetic of an edge group's fused launch
struct GroupRoute { bool bf, dense_rows; };
static GroupRoute group_route(const Model& m, const ConvW& L, const RunGroup& g) {
  GroupRoute r;
  // split-bf16 edge product (ddmi_config.edge_product = 1): the static l <= 1 loops only; other layers keep the f32 route
  r.bf = m.cfg.edge_product == 1 && !L.fgran_generic && L.maxd <= 3 && m.cfg.sh_lmax <= 1;
  // dense-row loop: groups with >= 20 edges per gather node (both row tiles of every virtual node are multiplied)
  r.dense_rows = m.fused_dense == 2 || (m.fused_dense == 1 && (long)g.ea_rows >= 20L * std::max(1, g.gcount));
  return r;
}

// arguments of k_edge_hidden_mm for one edge group (first Linear straight from the edge attributes)
static EdgeHiddenArgs hidden_args(Model& m, const ConvW& L, const RunGroup& g, int wg, const float* P, const float* Q, const float* rb,
                                  float* Hb, const GroupRoute& rt) {
  Cx& c = *m.cx;
  Cx::VnSet& vs = c.vn[g.vn];
  EdgeHiddenArgs h{};
  h.nvn = vs.nvn_pad ? vs.nvn_pad : vs.voff + g.gcount;
  h.vcap = vs.vcap; h.vn_node = vs.node; h.vn_e0 = vs.e0; h.goff = g.goff; h.arow = g.arow; h.tgt = g.tgt;
  h.tbase = g.tbase; h.ea = g.ea; h.ns = m.ns; h.W1 = L.W1p[wg]; h.ldw = L.n_edge; h.P = P; h.Q = Q; h.rowbias = rb; h.ridx = g.sig_idx;
  h.H = L.H; h.NG8 = L.HKq / 8; h.Hb = Hb; h.bf = rt.bf ? 1 : 0;
  h.zero_fill = (!L.fgran_generic && rt.dense_rows) ? 1 : 0;
  if (m.cfg.sh_lmax <= 1) { h.vrows = vs.rows; h.vn_ne = vs.ne; }
  h.grid = m.eh_grid;
  return h;
}

// arguments of the fused convolution for one edge group; ys_force > 0: workgroups per tile chosen by the caller (grouped dispatch)
static FusedConvArgs fused_args(Model& m, const ConvW& L, const RunGroup& g, size_t gi, int wg, const float* Xin, const float* Hb,
                                const GroupRoute& rt, bool small_layer, int ys_force) {
  Cx& c = *m.cx;
  Cx::VnSet& vs = c.vn[g.vn];
  FusedConvArgs f{};
  f.nvn = vs.nvn_pad ? vs.nvn_pad : vs.voff + g.gcount;
  f.vcap = vs.vcap; f.vn_node = vs.node; f.vrows = vs.rows; f.vn_ne = vs.ne;
  f.X = Xin; f.gbase = g.gbase; f.wpack = L.wpack[wg]; f.KS = L.KS; f.HK = L.HK; f.Hb = Hb; f.NG8 = L.HKq / 8;
  f.sh_lmax = m.cfg.sh_lmax; f.gran = L.fgran; f.cgt = L.cgt;
  f.max_nb = L.max_nb; f.maxd = L.maxd; f.msg = g.msg; f.generic = L.fgran_generic ? 1 : 0;
  f.dense = rt.dense_rows ? 1 : 0;
  f.bf = rt.bf ? 1 : 0;
  f.tile_hdr = (g.vn == 0 && c.prered) ? vs.tile_hdr : nullptr;
  // ligand gather nodes with >= 2 virtual nodes on average (rec<-lig): a tile of 16 virtual nodes holds few distinct nodes
  f.shared = (rt.dense_rows && (m.fused_shared == 2 || (m.fused_shared == 1 && g.load && (long)g.ea_rows >= 48L * std::max(1, g.gcount)))) ? 1 : 0;
  f.prof_slot = (int)gi;
  // workgroups per tile (granule ranges): 0 = spread a launch with few tiles over the CUs
  int ys_req = ys_force > 0 ? ys_force : m.fused_ysplit;
  if (ys_req <= 0) {
    // Small batches (no group of the layer fills the chip once; tiles ~ gather nodes x ceil(mean degree / 32) / 16): up to
    // one granule per workgroup, 5 poses 94 -> 100 poses/s.  Otherwise the round-2 rule (at most 6 ranges, tiles estimated
    // from nodes + edges / 32): the small lig-lig launch that runs next to the big groups is sensitive to its split -- 4
    // ranges at 40 poses; 5-6 cost the headline 2.5 % (profiles/r03_e27..e37_ab.txt).
    auto round_model = [&](long T) {
      int pick = 1;
      double best = 1e30;
      for (int y = 1; y <= std::min(8, L.n_fgran); ++y) {
        const double rounds = std::ceil((double)T * y / (double)m.n_cus);
        const double cost = rounds * ((double)((L.n_fgran + y - 1) / y) + 0.2);
        if (cost < best - 1e-9) { best = cost; pick = y; }
      }
      return pick;
    };
    if (small_layer && m.ys_rounds_small && tiles_of(g) >= 32) ys_req = round_model(tiles_of(g));
    else if (small_layer) ys_req = (int)std::min(8L, std::max(1L, 768 / tiles_of(g)));
    else if (m.ys_rounds && tiles_of(g) >= m.n_cus) {
      // Chip-filling group (round 6): one workgroup per CU, so a launch of T x ys work items runs in ceil(T ys / CUs) rounds of
      // (granules per item + tile prologue ~ 0.2 granules): pick the split with the cheapest schedule.  The old rule gave every
      // group of >= 256 tiles ONE item per tile: 375 tiles (20 poses) = 1.46 rounds, i.e. two rounds with the second half empty
      // -- 138.2 poses/s against 145.1 with the last launch of each stream split in four (profiles/r06_p6_b20_ab.txt); 750 tiles
      // (40 poses) = 2.93 rounds keep one item per tile.
      ys_req = round_model(tiles_of(g));
    }
    else ys_req = (int)std::min(6L, std::max(1L, 768 / std::max(1L, ((long)g.gcount + g.ea_rows / 32) / 16)));
    const int ys_small = m.fused_ysplit_small;   // tuning: split of a small group next to big ones
    if (ys_small > 0 && !small_layer && tiles_of(g) < 256) ys_req = ys_small;
  }
  ys_req = std::max(ys_req, (L.n_fgran + 19) / 20);   // a workgroup keeps at most 24 granule descriptors in LDS
  const int ys = std::max(1, std::min(std::min(ys_req, 8), L.n_fgran));
  f.ysplit = ys;
  f.gsplit[0] = 0;
  for (int y = 1; y < ys; ++y) {   // split points at unit boundaries (later granules of a unit add to the first one's stores)
    int b = L.n_fgran * y / ys;
    while (b < L.n_fgran && b > 0 && L.fgran_unit[b] == L.fgran_unit[b - 1]) ++b;
    f.gsplit[y] = std::max(b, f.gsplit[y - 1]);
  }
  f.gsplit[ys] = L.n_fgran;
  f.n_units = 0;
  for (int gq = 0; gq < L.n_fgran && f.n_units < 48; ++gq)
    if (gq == 0 || L.fgran_unit[gq] != L.fgran_unit[gq - 1]) f.ustart[f.n_units++] = (short)gq;
  for (int y = 0; y < ys; ++y) {   // units of every granule range (ranges start at unit boundaries)
    f.ufirst[y] = 0; f.ucount[y] = 0;
    for (int u = 0; u < f.n_units; ++u)
      if (f.ustart[u] >= f.gsplit[y] && f.ustart[u] < f.gsplit[y + 1]) { if (f.ucount[y] == 0) f.ufirst[y] = (short)u; ++f.ucount[y]; }
  }
  return f;
}

// One edge group of a TensorProductConvLayer on stream gs: per-graph / per-node terms of the first Linear (unless mm_all: the
// layer's batched launch already produced them), virtual-node lists (first use in this forward), hidden rows, fused launch.
// side: the scratch set of the side stream.
static void run_group(Model& m, const ConvW& L, const RunGroup& g, size_t gi, bool side, bool mm_all, bool small_layer,
                      const float* Xin, hipStream_t gs, int ys_force = 0) {
  Cx& c = *m.cx;
  const int ns = m.ns, H = L.H;
  float *HE = side ? c.HE_b : c.HE, *P = side ? c.P_b : c.P, *Q = side ? c.Q_b : c.Q;
  float* rowbias = side ? c.rowbias_b : c.rr_rowbias;
  if (mm_all) { P = c.Pg[gi]; Q = c.Qg[gi]; rowbias = c.rbg[gi]; }
  const int wg = std::min<int>((int)gi, L.G - 1);
  const float* W1 = L.W1[wg];
  const float* rb = nullptr;
  // Every edge group runs k_conv_fused (a node-contracted layer always has its granule list; ligand gather nodes with many
  // edges are cut into 32-edge virtual nodes like the others -- several virtual nodes of an atom share its contraction in the
  // shared-node tiles, mode 4 of the kernel).
  DDMI_REQUIRE(g.vn >= 0 && L.n_fgran > 0 && c.Hb, DDMI_ERR_STATE, "convolution layer without a granule list / virtual-node set");
  float* Hb = side ? c.Hb_b : c.Hb;
  const bool deep = L.TL > 2;   // FCBlock with hidden Linear layers: first layer as plain per-edge rows, the hidden ones as GEMMs
  const bool fuse_mm = !deep && m.fused_mm && ns % 16 == 0 && ns <= 64 && L.W1p[wg];   // first Linear inside the hidden-row kernel
  if (m.cfg.exec.debug & 1)   // the route this group takes, for tests: hidden rows (mm / gemm / deep) and the granule loops
    fprintf(stderr, "ddmi route %s g%d: hidden %s granules %s\n", L.name.c_str(), (int)gi,
            fuse_mm ? "mm" : deep ? "deep" : "gemm", L.fgran_generic ? "generic" : "static");
  if (mm_all) {
    if (g.sig) rb = g.rb_ready ? g.rb_ready : rowbias;
  } else if (fuse_mm) {   // everything in the emission order of k_edge_hidden_mm (permuted copy of the first layer)
    PhaseTimer t(m, "conv_fc1_gemms", gs);
    const float* W1p = L.W1p[wg];
    GemmBatch gb;   // the group's per-graph and per-node terms of the first Linear: independent, one launch
    auto add = [&](const float* A, int lda, const float* W, const float* bias, float* C, int M) {
      GemmArgs& x = gb.g[gb.n++];
      x.A = A; x.lda = lda; x.W = W; x.ldw = L.n_edge; x.bias = bias; x.C = C; x.ldc = H; x.M = M; x.N = H; x.K = ns;
    };
    if (g.sig) { add(g.sig, ns, W1p, nullptr, rowbias, c.B); rb = rowbias; }
    add(Xin + (size_t)g.tbase * XS, XS, W1p + (g.swap_pq ? 2 : 1) * ns, nullptr, P, g.tcount);
    add(Xin + (size_t)g.gbase * XS, XS, W1p + (g.swap_pq ? 1 : 2) * ns, L.b1p[wg], Q, g.gcount);
    launch_gemm_batch(gb, gs);
  } else {
    PhaseTimer t(m, "conv_fc1_gemms", gs);
    if (g.sig) {  // W1e * (edge_attr + sig[b]) = W1e*edge_attr + (W1e*sig)[b]
      gemm(g.sig, ns, W1, L.n_edge, nullptr, rowbias, H, c.B, H, ns, 0, gs);
      rb = rowbias;
    }
    gemm(g.ea, ns, W1, L.n_edge, nullptr, HE, H, g.ea_rows, H, ns, 0, gs, g.ea_rows_dev, rb, g.sig_idx, H);
    gemm(Xin + (size_t)g.tbase * XS, XS, W1 + (g.swap_pq ? 2 : 1) * ns, L.n_edge, nullptr, P, H, g.tcount, H, ns, 0, gs);
    gemm(Xin + (size_t)g.gbase * XS, XS, W1 + (g.swap_pq ? 1 : 2) * ns, L.n_edge, L.b1[wg], Q, H, g.gcount, H, ns, 0, gs);
  }
  ensure_vn(m, g, gs);
  Cx::VnSet& vs = c.vn[g.vn];
  const int* nvn = vs.nvn_pad ? vs.nvn_pad : vs.voff + g.gcount;
  const GroupRoute rt = group_route(m, L, g);
  const bool bf = rt.bf;
  if (fuse_mm) {
    PhaseTimer t(m, "k_edge_hidden", gs);
    launch_edge_hidden_mm(hidden_args(m, L, g, wg, P, Q, rb, Hb, rt), gs);
  } else if (deep) {
    PhaseTimer t(m, "k_edge_hidden", gs);
    float* cur = side ? c.HD_b[0] : c.HD[0];
    float* nxt = side ? c.HD_b[1] : c.HD[1];
    DDMI_REQUIRE(cur && nxt, DDMI_ERR_STATE, "tp_weights_layers > 2: hidden-row scratch missing");
    launch_edge_rows(nvn, vs.vcap, vs.node, vs.e0, g.goff, g.arow, g.tgt, g.tbase, HE, P, Q, H, cur, gs);
    for (int j = 0; j + 2 < L.TL; ++j) {   // hidden Linear + ReLU layers (models/layers.py:14-15), rows in gather order
      gemm(cur, H, L.Wmid[wg][j], H, L.bmid[wg][j], nxt, H, g.ea_rows, H, H, 1, gs, g.ea_rows_dev);
      std::swap(cur, nxt);
    }
    launch_edge_hidden(nvn, vs.vcap, vs.node, vs.e0, g.goff, nullptr, g.tgt, g.tbase, cur, nullptr, nullptr, H, L.HKq / 8, Hb, gs, bf ? 1 : 0);
  } else {
    PhaseTimer t(m, "k_edge_hidden", gs);
    launch_edge_hidden(nvn, vs.vcap, vs.node, vs.e0, g.goff, g.arow, g.tgt, g.tbase, HE, P, Q, H, L.HKq / 8, Hb, gs, bf ? 1 : 0);
  }
  const FusedConvArgs f = fused_args(m, L, g, gi, wg, Xin, Hb, rt, small_layer, ys_force);
  if (m.timing && m.timing_level >= 2) {   // ddmi_set_kernel_timing(h, 2 | 3): one timing row per edge group / per (layer, edge group)
    const bool per_layer = m.timing_level >= 3;
    const std::string tname = "k_conv_fused:" + (per_layer ? "L" + L.name.substr(L.name.size() - 1) : std::string()) + "g" + std::to_string(gi);
    PhaseTimer t(m, tname.c_str(), gs);
    launch_conv_fused(f, gs);
  } else {
    PhaseTimer t(m, "k_conv_fused", gs);
    launch_conv_fused(f, gs);
  }
}

// Grouped dispatch of a layer (round 6, ddmi_exec_options.grouped): on ONE stream, [per-node terms of the first Linear of every
// group: one launch] -> [hidden rows of every group: one launch, each group into its own buffer] -> [k_conv_grouped: the work
// items of every group in one grid].  Same device code and arguments per work item as the per-group launches (bit-identical
// messages); what changes is that no group waits for another one's launch to drain, a small group (lig-lig: 10-79 tiles) never
// has the chip to itself, and a layer is 4 launches instead of ~11.  Supported: exact-f32 l <= 1 layers with static chain
// shapes, two-layer edge MLPs (the benchmark preset); anything else takes the per-group path of run_conv.
static bool grouped_ok(const Model& m, const ConvW& L, const std::vector<RunGroup>& groups) {
  const Cx& c = *m.cx;
  if (!c.Hbg[0] || groups.size() < 2 || groups.size() > 9 || !c.Pg[0]) return false;
  if (L.TL != 2 || !m.fused_mm || m.ns % 16 != 0 || m.ns > 64 || L.fgran_generic || L.maxd > 3 || m.cfg.sh_lmax > 1 || L.n_fgran <= 0) return false;
  if (m.cfg.edge_product != 0) return false;
  if (m.timing && m.timing_level >= 2) return false;   // per-group timing rows need per-group launches
  for (size_t gi = 0; gi < groups.size(); ++gi)
    if (!L.W1p[std::min<int>((int)gi, L.G - 1)] || groups[gi].vn < 0) return false;
  return true;
}
static void run_groups_grouped(Model& m, const ConvW& L, const std::vector<RunGroup>& groups, const float* Xin, hipStream_t s, bool pq_ready) {
  Cx& c = *m.cx;
  const int ns = m.ns, H = L.H;
  if (!pq_ready) {   // per-graph / per-node terms of the first Linear of every group
    PhaseTimer t(m, "conv_fc1_gemms", s);
    GemmBatch gb;
    auto add = [&](const float* A, int lda, const float* W, const float* bias, float* C, int M) {
      if (gb.n == GEMM_BATCH_MAX) { launch_gemm_batch(gb, s); gb.n = 0; }
      GemmArgs& x = gb.g[gb.n++];
      x = GemmArgs{};
      x.A = A; x.lda = lda; x.W = W; x.ldw = L.n_edge; x.bias = bias; x.C = C; x.ldc = H; x.M = M; x.N = H; x.K = ns;
    };
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      const RunGroup& g = groups[gi];
      const int wg = std::min<int>((int)gi, L.G - 1);
      const float* W1p = L.W1p[wg];
      if (g.sig && !g.rb_ready) add(g.sig, ns, W1p, nullptr, c.rbg[gi], c.B);
      add(Xin + (size_t)g.tbase * XS, XS, W1p + (g.swap_pq ? 2 : 1) * ns, nullptr, c.Pg[gi], g.tcount);
      add(Xin + (size_t)g.gbase * XS, XS, W1p + (g.swap_pq ? 1 : 2) * ns, L.b1p[wg], c.Qg[gi], g.gcount);
    }
    launch_gemm_batch(gb, s);
  }
  ensure_vn_all(m, groups, s);
  // workgroups per tile: all groups of the layer share the chip, so the split follows the layer's total tile count
  long tiles = 0;
  for (auto& g : groups) tiles += tiles_of(g);
  int ys = m.grouped_split;
  if (ys <= 0) ys = (int)std::min(8L, std::max(1L, (long)m.grouped_target / std::max(1L, tiles)));
  // launch order: the groups with the longest work items first (dense residue / atom gathers), sparse-row groups last -- the short
  // items of the small groups fill the tail of the launch
  std::vector<size_t> order(groups.size());
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    const GroupRoute ra = group_route(m, L, groups[a]), rb_ = group_route(m, L, groups[b]);
    if (ra.dense_rows != rb_.dense_rows) return ra.dense_rows;
    return tiles_of(groups[a]) > tiles_of(groups[b]);
  });
  for (size_t o0 = 0; o0 < order.size(); o0 += FC_GROUPS_MAX) {
    const size_t n = std::min<size_t>(FC_GROUPS_MAX, order.size() - o0);
    EdgeHiddenGroupedArgs HG;
    FusedGroupedArgs FG;
    HG.n = FG.n = (int)n;
    for (size_t k = 0; k < n; ++k) {
      const size_t gi = order[o0 + k];
      const RunGroup& g = groups[gi];
      const int wg = std::min<int>((int)gi, L.G - 1);
      const GroupRoute rt = group_route(m, L, g);
      HG.g[k] = hidden_args(m, L, g, wg, c.Pg[gi], c.Qg[gi], g.sig ? (g.rb_ready ? g.rb_ready : c.rbg[gi]) : nullptr, c.Hbg[g.vn], rt);
      HG.g[k].grid = std::max(64, (int)((long)m.eh_grid * tiles_of(g) / std::max(1L, tiles)));   // the launch's workgroups dealt by tile count
      FG.g[k] = fused_args(m, L, g, gi, wg, Xin, c.Hbg[g.vn], rt, false, ys);
    }
    {
      PhaseTimer t(m, "k_edge_hidden", s);
      launch_edge_hidden_mm_grouped(HG, s);
    }
    PhaseTimer t(m, "k_conv_fused", s);
    launch_conv_grouped(FG, s);
  }
}

// One TensorProductConvLayer in the node-contracted form (k_conv.hip).
// pq_mode: 0 = the per-node terms of the first Linear as the size rule says (per group, or batched for small layers), 1 = all of
// them in one launch in front of the groups (first layer of the fused node-update route), 2 = already there (written by the
// previous layer's k_node_update).  Lnext / gnext: the NEXT interaction layer and its groups -- the node update then also
// produces their per-node terms (k_node_update instead of k_reduce_bn).
void run_conv(Model& m, const ConvW& L, const std::vector<RunGroup>& groups, const ReduceGroup* rg_dev, int n_rg,
              const float* Xin, float* Xout, int nbase, int ncount, hipStream_t s, int pq_mode = 0, const ConvW* Lnext = nullptr,
              const std::vector<RunGroup>* gnext = nullptr) {
  Cx& c = *m.cx;
  const int ns = m.ns, H = L.H;
  auto node_update = [&]() {   // the layer's node update: mean over all groups' messages + BatchNorm + residual (+ the next layer's P / Q)
    if (!Lnext) {
      PhaseTimer t(m, "k_reduce_bn", s);
      launch_reduce_bn(rg_dev, n_rg, nbase, ncount, L.D_in, L.D_out, L.has_bn ? L.bn_mean : nullptr,
                       L.has_bn ? L.bn_scale : nullptr, L.has_bn ? L.bn_bias : nullptr, L.residual ? 1 : 0, Xin, Xout, XS, s);
      return;
    }
    DDMI_REQUIRE(rg_dev != c.rg_all_share, DDMI_ERR_STATE, "k_node_update does not fold message rows onto graph 0 (ReduceGroup::tmod)");
    PhaseTimer t(m, "k_reduce_bn", s);   // (same timer row: the scatter stage of the layer)
    NodeUpdateArgs a{};
    a.groups = rg_dev; a.n_groups = n_rg; a.nbase = nbase; a.ncount = ncount; a.D_in = L.D_in; a.D_out = L.D_out;
    a.bn_mean = L.has_bn ? L.bn_mean : nullptr; a.bn_scale = L.has_bn ? L.bn_scale : nullptr; a.bn_bias = L.has_bn ? L.bn_bias : nullptr;
    a.residual = L.residual ? 1 : 0; a.X_in = Xin; a.X_out = Xout;
    a.ns = ns; a.H = Lnext->H; a.ldw = Lnext->n_edge; a.wpn = m.node_update_wpn;
    for (size_t gi = 0; gi < gnext->size(); ++gi) {
      const RunGroup& g = (*gnext)[gi];
      const int wg = std::min<int>((int)gi, Lnext->G - 1);
      const float* W1p = Lnext->W1p[wg];
      DDMI_REQUIRE(a.n_terms + 2 <= NU_TERMS_MAX, DDMI_ERR_CAPACITY, "k_node_update: more first-Linear terms than slots");
      a.term[a.n_terms++] = NodeTerm{W1p + (g.swap_pq ? 2 : 1) * ns, nullptr, c.Pg[gi], g.tbase, g.tcount};
      a.term[a.n_terms++] = NodeTerm{W1p + (g.swap_pq ? 1 : 2) * ns, Lnext->b1p[wg], c.Qg[gi], g.gbase, g.gcount};
    }
    launch_node_update(a, s);
  };
  // Groups whose gather nodes are ligand atoms (few nodes, many edges each: MFMA-bound) run on the side stream with
  // their own scratch, concurrently with the receptor-gather groups (HBM-bound on the contracted rows).
  bool forked = false;
  if (m.two_streams && m.side_stream && groups.size() > 1) {
    for (auto& g : groups) forked = forked || (g.gbase == 0 && g.gcount == c.nL && c.nR > 0);
    bool any_main = false;
    for (auto& g : groups) any_main = any_main || !(g.gbase == 0 && g.gcount == c.nL);
    forked = forked && any_main;
  }
  long biggest = 1;
  for (auto& q : groups) biggest = std::max(biggest, tiles_of(q));
  const bool small_layer = biggest < 256;
  // (default = per-group launches on two streams: the grouped dispatch shortens the time covered by fused workgroups by 3-5 % but
  // leaves the hidden rows of the whole layer exposed in front of it -- 151.5 against 155.2 poses/s at 40 poses, 124.8 / 127.3 at
  // 10, 106.8 / 107.9 at 5, profiles/r06_p2_*)
  if (m.grouped == 2 && grouped_ok(m, L, groups)) {
    run_groups_grouped(m, L, groups, Xin, s, pq_mode == 2);
    node_update();
    return;
  }
  // The per-graph and per-node terms of the first Linear of EVERY group (P = W1s x_target, Q = W1d x_gather + b1, sigma rows)
  // depend on the layer input only.  Small layers: one batched launch in front of the fork instead of one small launch at the
  // head of every group's chain (5 poses: 101.4 -> 102.9 poses/s).  Large layers keep them per group: there the other stream
  // fills the gap, and a common launch in front of the fork delays the side stream (40 poses: -0.5 %; profiles/r03_e42_ab.txt).
  bool mm_all = L.TL == 2 && (pq_mode != 0 || (m.fc1_batch && small_layer)) && m.fused_mm && ns % 16 == 0 && ns <= 64 && groups.size() <= 9 && c.Pg[0];
  for (size_t gi = 0; gi < groups.size(); ++gi) mm_all = mm_all && L.W1p[std::min<int>((int)gi, L.G - 1)];
  DDMI_REQUIRE(pq_mode == 0 || mm_all, DDMI_ERR_STATE, "fused node-update route on a layer without batched first-Linear terms");
  if (mm_all && pq_mode != 2) {
    PhaseTimer t(m, "conv_fc1_gemms", s);
    GemmBatch gb;
    auto add = [&](const float* A, int lda, const float* W, const float* bias, float* C, int M) {
      if (gb.n == GEMM_BATCH_MAX) { launch_gemm_batch(gb, s); gb.n = 0; }
      GemmArgs& x = gb.g[gb.n++];
      x = GemmArgs{};
      x.A = A; x.lda = lda; x.W = W; x.ldw = L.n_edge; x.bias = bias; x.C = C; x.ldc = H; x.M = M; x.N = H; x.K = ns;
    };
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      const RunGroup& g = groups[gi];
      const int wg = std::min<int>((int)gi, L.G - 1);
      const float* W1p = L.W1p[wg];
      if (g.sig && !g.rb_ready) add(g.sig, ns, W1p, nullptr, c.rbg[gi], c.B);
      add(Xin + (size_t)g.tbase * XS, XS, W1p + (g.swap_pq ? 2 : 1) * ns, nullptr, c.Pg[gi], g.tcount);
      add(Xin + (size_t)g.gbase * XS, XS, W1p + (g.swap_pq ? 1 : 2) * ns, L.b1p[wg], c.Qg[gi], g.gcount);
    }
    launch_gemm_batch(gb, s);
  }
  // virtual-node lists and per-edge rows of every group whose topology changed since they were built (first layer of a forward):
  // two launches in front of the fork instead of a count -> scan -> fill -> rows chain at the head of every group's stream
  if (m.vn_merge) ensure_vn_all(m, groups, s);
  if (forked) {
    DDMI_CHECK_HIP(hipEventRecord(m.ev_fork, s));
    DDMI_CHECK_HIP(hipStreamWaitEvent(m.side_stream, m.ev_fork, 0));
  }
  // (Measured and dropped in round 4, profiles/r04_e5_ab.txt: the GEMMs / hidden rows of a stream's SECOND group on extra
  // "preparation" streams next to the first group's fused launch.  The time with no k_conv_fused dispatch running stayed at
  // 1.87 ms per forward, the fused launches themselves got 4 % slower -- 27-KB k_edge_hidden_mm workgroups scattered over the
  // CUs keep 158-KB fused workgroups from being placed: 139.8 -> 135.7 poses/s on the same box.)
  // issue order of the groups (exec.group_order, A/B knob): bit 0 = the side stream's groups in reverse order (rec<-lig in front of
  // lig-lig: the short lig-lig items then fill the layer's tail), bit 1 = the main stream's groups in reverse order
  std::vector<size_t> issue;
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<size_t> part;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      const bool side_g = forked && groups[gi].gbase == 0 && groups[gi].gcount == c.nL;
      if (side_g == (pass == 1)) part.push_back(gi);
    }
    if (forked && ((m.group_order >> (pass == 1 ? 0 : 1)) & 1)) std::reverse(part.begin(), part.end());
    issue.insert(issue.end(), part.begin(), part.end());
  }
  if (!forked || m.group_order == 0) { issue.clear(); for (size_t gi = 0; gi < groups.size(); ++gi) issue.push_back(gi); }
  for (size_t ii = 0; ii < issue.size(); ++ii) {
    const size_t gi = issue[ii];
    const RunGroup& g = groups[gi];
    const bool side = forked && g.gbase == 0 && g.gcount == c.nL;
    // exec.tile_split_last: the LAST fused launch of each stream in finer work items -- the launch whose final partial round of
    // workgroups is the layer's straggler tail (workgroup stamps: 0.46 ms per forward with < 32 of 256 CUs busy, profiles/r06_p2_wg_idle_b40_g1.txt)
    int ys_last = 0;
    if (m.fused_ysplit_last > 0 && !small_layer) {
      bool last_on_stream = true;
      for (size_t jj = ii + 1; jj < issue.size(); ++jj) {
        const size_t gj = issue[jj];
        const bool side_j = forked && groups[gj].gbase == 0 && groups[gj].gcount == c.nL;
        if (side_j == side) last_on_stream = false;
      }
      if (last_on_stream && tiles_of(g) >= 256) ys_last = m.fused_ysplit_last;
    }
    run_group(m, L, g, gi, side, mm_all, small_layer, Xin, side ? m.side_stream : s, ys_last);
  }
  if (forked) {
    DDMI_CHECK_HIP(hipEventRecord(m.ev_join, m.side_stream));
    DDMI_CHECK_HIP(hipStreamWaitEvent(s, m.ev_join, 0));
  }
  node_update();
}

// The interaction layers of the CG model with the layer boundaries overlapped (round 5, ddmi_exec_options.layer_overlap; NOT the
// default: measured neutral at 40 poses -- 154.1 / 154.7 against 154.8 / 155.1 poses/s joined, profiles/r05_e11_ab.txt: the lig-lig
// launch that now runs alone at the boundary takes half its time, the rec<-lig launch next to the boundary kernels a third more;
// the forward is the SUM of its kernels' stand-alone times on either schedule -- and 6 % slower at 5 poses).
// run_conv joins both streams behind a layer's four fused launches, reduces every node and only then starts the next layer's
// chains: per boundary the chip runs [k_reduce_bn -> first-Linear GEMMs -> k_edge_hidden_mm] with no fused workgroup in flight
// (2.0 ms of a 13.7-ms forward at 40 poses, profiles/r05_v1_timeline.txt).  The node update is per node, so it splits by node
// type -- ligand rows need the lig-lig and lig<-rec messages, receptor rows the rec-rec and rec<-lig ones -- and every chain
// starts as soon as the rows IT reads exist:
//   main stream: lig<-rec(l) | reduce ligand rows(l) | rec-rec(l) | reduce receptor rows(l) | lig<-rec(l+1) ...
//   side stream: lig-lig(l)  | rec<-lig(l)           | lig-lig(l+1) [behind rec-rec(l)'s launch] | rec<-lig(l+1) ...
// lig-lig(l+1) reads ligand rows only: it is deliberately held until the rec-rec launch of layer l has finished, so that its
// fused workgroups fill the chip while the main stream is in the receptor update and the lig<-rec chain of layer l+1.
// Same kernels, same arguments, same arithmetic as run_conv (bit-identical scores); only the order of the launches differs.
void run_conv_layers_overlapped(Model& m, const RunGroup& g_ll, const RunGroup& g_lr, const RunGroup& g_rr, const RunGroup& g_rl,
                                const ReduceGroup* rg, int& xi, hipStream_t s) {
  Cx& c = *m.cx;
  const int Lc = (int)m.conv_layers.size(), nL = c.nL, nR = c.nR;
  hipStream_t side = m.side_stream;
  enum { E_LL, E_RL, E_RR, E_RED_L, E_RED_R, E_N };   // fused launch of a group finished / rows of a node type written
  while ((int)m.ev_pipe.size() < E_N * Lc) {
    hipEvent_t e;
    DDMI_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    m.ev_pipe.push_back(e);
  }
  auto ev = [&](int l, int k) { return m.ev_pipe[(size_t)l * E_N + k]; };
  auto record = [&](int l, int k, hipStream_t st) { DDMI_CHECK_HIP(hipEventRecord(ev(l, k), st)); };
  auto wait = [&](hipStream_t st, int l, int k) { DDMI_CHECK_HIP(hipStreamWaitEvent(st, ev(l, k), 0)); };   // (always behind its record in host order)
  auto reduce = [&](const ConvW& L, const ReduceGroup* groups, int nbase, int ncount, const float* Xin, float* Xout) {
    PhaseTimer t(m, "k_reduce_bn", s);
    launch_reduce_bn(groups, 2, nbase, ncount, L.D_in, L.D_out, L.has_bn ? L.bn_mean : nullptr, L.has_bn ? L.bn_scale : nullptr,
                     L.has_bn ? L.bn_bias : nullptr, L.residual ? 1 : 0, Xin, Xout, XS, s);
  };
  DDMI_CHECK_HIP(hipEventRecord(m.ev_fork, s));            // the layer-0 table
  DDMI_CHECK_HIP(hipStreamWaitEvent(side, m.ev_fork, 0));
  for (int l = 0; l < Lc; ++l, ++xi) {
    const ConvW& L = m.conv_layers[l];
    const float* Xin = c.X[xi];
    float* Xout = c.X[xi + 1];
    const bool last = l == Lc - 1;   // the last layer updates the ligand rows only (cg_model.py:345-349)
    if (l > 0) { wait(side, l - 1, E_RR); wait(side, l - 1, E_RED_L); }
    run_group(m, L, g_ll, 0, true, false, false, Xin, side);
    record(l, E_LL, side);
    run_group(m, L, g_lr, 1, false, false, false, Xin, s);
    wait(s, l, E_LL);
    reduce(L, rg, 0, last && m.cfg.sidechain_pred ? c.N : nL, Xin, Xout);
    if (last) continue;
    record(l, E_RED_L, s);
    run_group(m, L, g_rr, 2, false, false, false, Xin, s);
    record(l, E_RR, s);
    if (l > 0) wait(side, l - 1, E_RED_R);
    run_group(m, L, g_rl, 3, true, false, false, Xin, side);
    record(l, E_RL, side);
    wait(s, l, E_RL);
    reduce(L, rg + 2, nL, nR, Xin, Xout);
    record(l, E_RED_R, s);
  }
}

// final_conv / tor_bond_conv: per-edge weights, then the table-driven tensor product.
void run_direct_conv(Model& m, const ConvW& L, const float* attr, int E, float* hid, float* Wt, const int* xrow,
                     const float* X, const float* sh, const float* ew, const int* valid_cnt, int cap, float* out_rows,
                     hipStream_t s) {
  gemm(attr, L.n_edge, L.W1[0], L.n_edge, L.b1[0], hid, L.H, E, L.H, L.n_edge, 1, s);
  gemm(hid, L.H, L.W2[0], L.H, L.b2[0], Wt, L.Wn, E, L.Wn, L.H, 0, s);
  TpApplyArgs a{};
  a.E = E; a.valid_cnt = valid_cnt; a.cap = cap; a.Wt = Wt; a.ldw = L.Wn; a.X = X; a.xrow = xrow; a.sh = sh;
  a.lds_ = L.sh_dim; a.ew = ew; a.paths = L.paths; a.ctab = L.ctab; a.items = L.items; a.n_items = L.n_items;
  a.out = out_rows; a.ldo = L.D_out;
  a.n_paths = (int)L.table.paths.size();
  a.form = m.tp_form;
  a.z_floats = 0;
  for (auto& p : L.table.paths) a.z_floats += p.mul_in * p.dout;
  launch_tp_apply(a, s);
}

EdgeMlpArgs mlp_args(const Mlp2W& w, int ns, int E, const int* e_dev, const float* dist, const float* offsets, int D,
                     float coeff, int g_col, const float* gvec, const int* gidx, float* out) {
  EdgeMlpArgs a;
  a.E = E; a.e_dev = e_dev; a.dist = dist; a.offsets = offsets; a.D = D; a.coeff = coeff;
  a.W0g = w.W0 + g_col; a.ldw0g = w.in; a.gvec = gvec; a.gidx = gidx; a.W1 = w.W3; a.b1 = w.b3; a.ns = ns;
  a.out = out; a.ldo = ns;
  return a;
}

}  // namespace

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
    DDMI_REQUIRE(m.crop_cutoff <= 0.0, DDMI_ERR_ARG, "crop_beyond is not implemented for the all-atom model (aa_model.py:365-367)");
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
  struct HostEdges { std::vector<int> goff, toff, arow, tgt, tslot; };
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
    for (int e = 0; e < E; ++e) { const int k = h.arow[e]; h.tgt[e] = tgt_base + tl[k]; h.tslot[e] = tcur[tl[k]]++; }
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
    auto up_edges = [&](const HostEdges& h, const char* name) {
      Cx::StaticEdges e;
      e.E = (int)h.arow.size();
      e.goff = dup(m, name, h.goff); e.toff = dup(m, nullptr, h.toff); e.arow = dup(m, nullptr, h.arow);
      e.tgt = dup(m, nullptr, h.tgt); e.tslot = dup(m, nullptr, h.tslot);
      return e;
    };
    c.se_aa = up_edges(h_aa, "aa_goff"); c.se_ar = up_edges(h_ar, "ar_goff"); c.se_ra = up_edges(h_ra, "ra_goff");
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
  for (auto* fam : {&m.conv_layers, &m.lig_emb_layers, &m.rec_emb_layers, &m.old_lig, &m.old_rec, &m.old_l2r, &m.old_r2l})
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
      if (m.tight_caps && tight[i] >= 0) vs.vcap = (int)std::min<long>(vs.vcap, tight[i] + 2);
      if (m.tile_per_pose) {                    // every graph padded to whole 16-node tiles
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
        c.prered = m.fused_prered && shd == 4 && !cfg.old_model && !m.conv_layers.empty() && m.fused_shared != 2;   // (shared == 2: test mode, mode-4 tiles everywhere)
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
    if (m.grouped == 2 && HKq > 0)
      for (int i = 0; i < (cfg.all_atoms ? 9 : 4); ++i) c.Hbg[i] = dalloc<float>(m, nullptr, {round_up(c.vn[i].vcap, 16), 32, round_up(HKq, 16)});
    c.Hb_b = HKq > 0 ? dalloc<float>(m, nullptr, {round_up(vmax_b, 16), 32, round_up(HKq, 16)}) : nullptr;
  }
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
    }
  }
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

  // ---- receptor-side constants (CGModel.embedding caches these on the data object, cg_model.py:273-295)
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
    launch_edge_mlp(mlp_args(m.atom_edge, ns, c.Eaa, nullptr, c.aa_dist, m.off_lig, m.D, m.coeff_lig, 0, m.atom_edge.b0, nullptr,
                             c.atom_edge_base), s);
    launch_edge_mlp(mlp_args(m.ar_edge, ns, c.Ear, nullptr, c.ar_dist, m.off_rec, m.D, m.coeff_rec, 0, m.ar_edge.b0, nullptr,
                             c.ar_edge_base), s);
  }
  c.rec_node_enc = nullptr;
  if (!m.rec_emb_layers.empty() && cfg.all_atoms) {
    // aa_model.py:296-318: embedding layers over the sigma-free residue + atom graph, groups [rr, ar, aa, ra]; run in the
    // full node numbering (ligand rows unused) so that the interaction-layer CSRs serve unchanged
    const int aB = nL + nR, nA = c.nA;
    float* ea = dalloc<float>(m, nullptr, {N, XS}, true);
    float* eb = dalloc<float>(m, nullptr, {N, XS}, true);
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
  DDMI_CHECK_HIP(hipStreamSynchronize(s));
  if (rec_differ) {   // (the stream has just drained: no extra wait)
    int differ = 1;
    DDMI_CHECK_HIP(hipMemcpy(&differ, rec_differ, sizeof(int), hipMemcpyDeviceToHost));
    c.rec_copies = differ == 0;
  }
  m.has_complex = true;
}

// ============================================================ legacy class, confidence mode
// models/old_cg_model.py:203-291 (CGOldModel.forward with confidence_mode): four separate OldTensorProductConvLayers per
// interaction layer, each = fc + tensor product + its own mean + BatchNorm (tensor_layers.py:338-380), summed onto the
// zero-padded node features.
// Score read-outs on the final ligand rows XL (cg_model.py:368-423 = old_cg_model.py:293-352): centre convolution ->
// translation / rotation heads, torsion-bond convolution -> torsion head.
static void score_readouts(Model& m, const float* XL, const float* lig_pos, const float* t_tr, const float* t_rot,
                           const float* t_tor, float* tr_out, float* rot_out, float* tor_out, hipStream_t s) {
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int ns = m.ns, sd = m.sd, B = c.B, nL = c.nL;
  if (m.two_streams && m.side_stream && c.nT > 0 && tor_out) {   // the torsion head below forks here
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
  launch_segment_mean_bn(c.c_out, F.D_out, c.lig_ptr, nullptr, 0, B, F.D_out, F.has_bn ? F.bn_mean : nullptr,
                         F.has_bn ? F.bn_scale : nullptr, F.has_bn ? F.bn_bias : nullptr, c.gp, F.D_out, s);
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
    const bool fork = m.two_streams && m.side_stream;
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
    launch_segment_mean_bn(c.t_out, T.D_out, nullptr, c.t_cnt, c.tor_cap, c.nT, T.D_out, T.has_bn ? T.bn_mean : nullptr,
                           T.has_bn ? T.bn_scale : nullptr, T.has_bn ? T.bn_bias : nullptr, c.t_feat, T.D_out, s);
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

// =================================================================================== forward
void forward(Model& m, const float* lig_pos, const float* t_tr, const float* t_rot, const float* t_tor, float* tr_out,
             float* rot_out, float* tor_out, hipStream_t s, float* conf_out, float* atom_conf_out) {
  DDMI_REQUIRE(m.has_complex, DDMI_ERR_STATE, "ddmi_set_complex must precede ddmi_forward");
  const bool conf = m.cfg.confidence_mode != 0;
  DDMI_REQUIRE(conf == (conf_out != nullptr), DDMI_ERR_STATE, "score models use ddmi_forward, confidence models ddmi_confidence");
  DDMI_REQUIRE(conf || !m.cfg.scale_by_sigma || (m.so3_table && (m.cfg.no_torsion || m.torus_table)), DDMI_ERR_STATE,
               "score-norm tables not set (ddmi_set_table)");
  if (m.cfg.old_model) { forward_old(m, lig_pos, t_tr, t_rot, t_tor, tr_out, rot_out, tor_out, conf_out, s); return; }
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
  DDMI_REQUIRE(!(crop && cfg.all_atoms), DDMI_ERR_ARG, "crop_beyond is not implemented for the all-atom model (aa_model.py:365-367)");
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
  const bool early_cross = m.two_streams && m.side_stream && !crop;
  if (early_cross) {
    DDMI_CHECK_HIP(hipEventRecord(m.ev_fork, s));
    DDMI_CHECK_HIP(hipStreamWaitEvent(m.side_stream, m.ev_fork, 0));
    cross_pairs(m.side_stream, nullptr);
  }
  // ---- per-graph time terms
  if (m.time_terms_fused && sd / 2 <= 128 && ns <= 128) {   // one launch: embedding, every linear term of it, rec_sigma's second layer
    TimeTermsArgs ta{};
    ta.t = t_tr; ta.B = B; ta.freq = m.time_freq; ta.half = sd / 2; ta.scale = cfg.embedding_scale; ta.fourier = cfg.embedding_type; ta.temb = c.temb;
    ta.ns = ns;
    auto add = [&](const float* W, int ldw, const float* bias, float* C, int act) {
      auto& x = ta.term[ta.n++];
      x.W = W; x.ldw = ldw; x.bias = bias; x.C = C; x.act = act;
    };
    add(m.rec_sigma.W0, sd, m.rec_sigma.b0, c.hidB, 1);
    add(m.lig_enc.W0 + ns, ns + sd, m.lig_enc.b0, c.ligsig, 0);
    add(m.lig_edge.W0 + m.nf, m.lig_edge.in, m.lig_edge.b0, c.ll_gvec, 0);
    add(m.cross_edge.W0, m.cross_edge.in, m.cross_edge.b0, c.cross_gvec, 0);
    if (!conf) {
      add(m.center_edge.W0 + m.D, m.center_edge.in, m.center_edge.b0, c.center_gvec, 0);
      add(m.tr_final.W0 + 1, 1 + sd, m.tr_final.b0, c.tr_sig, 0);
      add(m.rot_final.W0 + 1, 1 + sd, m.rot_final.b0, c.rot_sig, 0);
    }
    ta.hid_term = 0; ta.W3 = m.rec_sigma.W3; ta.b3 = m.rec_sigma.b3; ta.out3 = c.rec_sig;
    launch_time_terms(ta, s);
  } else {
  launch_time_embedding(t_tr, B, m.time_freq, sd / 2, cfg.embedding_scale, cfg.embedding_type, c.temb, s);
  {   // the per-graph terms of the time embedding: independent tiny GEMMs, one launch (+ the second layer of rec_sigma)
    GemmBatch gb;
    auto add = [&](const float* W, int ldw, const float* bias, float* C, int act) {
      GemmArgs& x = gb.g[gb.n++];
      x.A = c.temb; x.lda = sd; x.W = W; x.ldw = ldw; x.bias = bias; x.C = C; x.ldc = ns; x.M = B; x.N = ns; x.K = sd; x.act = act;
    };
    add(m.rec_sigma.W0, sd, m.rec_sigma.b0, c.hidB, 1);
    add(m.lig_enc.W0 + ns, ns + sd, m.lig_enc.b0, c.ligsig, 0);
    add(m.lig_edge.W0 + m.nf, m.lig_edge.in, m.lig_edge.b0, c.ll_gvec, 0);
    add(m.cross_edge.W0, m.cross_edge.in, m.cross_edge.b0, c.cross_gvec, 0);
    if (!conf) {
      add(m.center_edge.W0 + m.D, m.center_edge.in, m.center_edge.b0, c.center_gvec, 0);
      add(m.tr_final.W0 + 1, 1 + sd, m.tr_final.b0, c.tr_sig, 0);
      add(m.rot_final.W0 + 1, 1 + sd, m.rot_final.b0, c.rot_sig, 0);
    }
    launch_gemm_batch(gb, s);
    gemm(c.hidB, ns, m.rec_sigma.W3, ns, m.rec_sigma.b3, c.rec_sig, ns, B, ns, ns, 0, s);
  }
  }
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
  // ---- ligand graph (bonds + radius graph)
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
  RunGroup g_ll{0, nL, 0, nL, c.goff_ll, c.ll_tgt, c.ll_tslot, nullptr, c.ll_ea, c.Ell_cap, c.goff_ll + nL, nullptr,
                nullptr, c.ll_nvec, c.ll_ew, 1.f, c.msg[0]};
  g_ll.vn = 2; g_ll.load = true;
  int xi = 0;
  for (size_t i = 0; i < m.lig_emb_layers.size(); ++i, ++xi)
    run_conv(m, m.lig_emb_layers[i], {g_ll}, c.rg_ll, 1, c.X[xi], c.X[xi + 1], 0, nL, s);
  // ---- per-step receptor crop (utils/sampling.py:104-109): residue mask + re-compacted contact graph
  const int* keep = nullptr;
  if (crop) {
    const double cd = m.crop_cutoff;
    launch_crop_mask(lig_pos, c.rec_pos, c.rec_batch, c.lig_ptr, nR, (float)(cd * cd), c.keep, s);
    launch_rr_filter(c.keep, c.rr_goff, c.rr_tgt, c.rr_arow, c.rr_toff, c.rr_tlist, c.rr_gnode, nL, nR, c.cnt_g2, c.cnt_t2,
                     c.goff2, c.toff2, c.tslot_tmp, c.tgt2, c.tslot2, c.arow2, s);
    keep = c.keep;
  }
  // receptor rows of the current table: cached embedding + sigma term on the scalars (cg_model.py:298-301)
  if (crop && !m.rec_emb_layers.empty()) {
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
  // ligand gather nodes carry up to Nr edges each: their 32-edge passes are dealt over several workgroups
  const int Lc = (int)m.conv_layers.size();
  if (cfg.all_atoms) {
    // ---- all-atom model (aa_model.py:364-436): atom rows, ligand<->atom radius graph, nine edge groups
    const int nA = c.nA, aB = nL + nR;
    launch_add_rowvec(c.X[xi] + (size_t)aB * XS, XS, c.atom_node_base, XS, c.rec_sig, ns, c.atom_batch, nA, c.rec_base_dim, ns, s);
    launch_cross_count(lig_pos, c.atom_pos, c.lig_batch, c.atom_batch, c.lig_ptr, c.atom_ptr, nL, nA, c.maxNa, nullptr,
                       cfg.lig_max_radius, nullptr, c.la_pairrank, c.la_cnt_l, c.la_cnt_a, s);
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
    RunGroup a_ra{aB, nA, nL, nR, c.se_ra.goff, c.se_ra.tgt, c.se_ra.tslot, c.se_ra.arow, c.ar_edge_base, c.Ear, nullptr, c.rec_sig,
                  c.ar_batch, c.ar_nvec, nullptr, 1.f, c.msg_aa[5]};
    RunGroup a_aa{aB, nA, aB, nA, c.se_aa.goff, c.se_aa.tgt, c.se_aa.tslot, c.se_aa.arow, c.atom_edge_base, c.Eaa, nullptr, c.rec_sig,
                  c.aa_batch, c.aa_nvec, c.aa_ew, 1.f, c.msg_aa[6]};
    RunGroup a_al{0, nL, aB, nA, c.la_offs_l, c.la3_tgt, c.la3_tslot, nullptr, c.la_ea, c.Ela_cap, c.la_offs_l + nL, nullptr,
                  nullptr, c.la_nvec, c.la_ew, 1.f, c.msg_aa[7]};
    RunGroup a_ar{nL, nR, aB, nA, c.se_ar.goff, c.se_ar.tgt, c.se_ar.tslot, c.se_ar.arow, c.ar_edge_base, c.Ear, nullptr, c.rec_sig,
                  c.ar_batch, c.ar_nvec, nullptr, 1.f, c.msg_aa[8]};
    a_la.vn = 4; a_ra.vn = 5; a_aa.vn = 6; a_al.vn = 7; a_al.load = true; a_ar.vn = 8;
    a_ra.static_topo = a_aa.static_topo = a_ar.static_topo = true;   // static atom relations (set_complex)
    t_phase.reset();
    for (int l = 0; l < Lc; ++l, ++xi) {
      if (l < Lc - 1)
        run_conv(m, m.conv_layers[l], {a_ll, a_lr, a_la, a_rr, a_rl, a_ra, a_aa, a_al, a_ar}, c.rg_aa_all, 9, c.X[xi], c.X[xi + 1], 0,
                 c.N, s);
      else run_conv(m, m.conv_layers[l], {a_ll, a_lr, a_la}, c.rg_aa_lig, 3, c.X[xi], c.X[xi + 1], 0, nL, s);
    }
  } else {
    t_phase.reset();
    // layer boundaries overlapped on request (ddmi_exec_options.layer_overlap, see run_conv_layers_overlapped): 1 = chip-filling
    // batches (small ones keep the joined form with its one batched first-Linear launch per layer), 2 = every batch
    bool overlapped = m.layer_overlap && m.two_streams && m.side_stream && nR > 0 && Lc >= 2;
    if (overlapped) {
      long biggest = 1;
      for (const RunGroup* q : {&g_ll, &g_lr, &g_rr, &g_rl}) biggest = std::max(biggest, tiles_of(*q));
      overlapped = biggest >= 256 || m.layer_overlap == 2;
    }
    // Fused node update (ddmi_exec_options.node_update = 1; not the default: -0.9 %, profiles/r06_p5_*): k_node_update writes a layer's rows AND the next layer's per-node
    // first-Linear terms P / Q, so only the first layer launches its GEMMs; the per-graph sigma term of the rec-rec group of every
    // layer comes from one batched launch here.
    bool nu = m.node_update && !overlapped && Lc >= 2 && m.fused_mm && ns % 16 == 0 && ns <= 64 && c.Pg[0] && (int)c.rb_l.size() == Lc;
    for (auto& L : m.conv_layers) {
      nu = nu && L.TL == 2 && L.H == m.conv_layers[0].H && L.n_edge == m.conv_layers[0].n_edge;
      for (int g = 0; g < 4; ++g) nu = nu && L.W1p[std::min(g, L.G - 1)];
    }
    if (nu) {
      PhaseTimer t(m, "conv_fc1_gemms", s);
      GemmBatch gb;
      for (int l = 0; l < Lc - 1; ++l) {   // (the last layer has no rec-rec group)
        const ConvW& L = m.conv_layers[l];
        if (gb.n == GEMM_BATCH_MAX) { launch_gemm_batch(gb, s); gb.n = 0; }
        GemmArgs& x = gb.g[gb.n++];
        x = GemmArgs{};
        x.A = c.rec_sig; x.lda = ns; x.W = L.W1p[std::min(2, L.G - 1)]; x.ldw = L.n_edge; x.C = c.rb_l[l]; x.ldc = L.H; x.M = B; x.N = L.H; x.K = ns;
      }
      if (gb.n) launch_gemm_batch(gb, s);
    }
    // Receptor copies under one t (exec.rec_share, ddmi_sample): the first layer's rec-rec group reads receptor rows, edge attributes
    // and the sigma term only -- the same for every graph of the batch -- so it runs on graph 0 (its own list, built once per complex)
    // and the node update reads graph 0's message rows for every graph, in the same order (bit-identical).  Layers >= 1 read
    // pose-dependent receptor rows.  The optional layer routes keep the full group.
    const bool rec_share = m.rec_share == 0 && m.uniform_t && c.rec_copies && !crop && !overlapped && !nu && m.grouped != 2 && Lc >= 2;
    RunGroup g_rr0 = g_rr;
    g_rr0.gcount = g_rr0.tcount = c.Rc_one; g_rr0.ea_rows = c.Erc_one; g_rr0.vn = 9; g_rr0.static_topo = true;
    if (overlapped) run_conv_layers_overlapped(m, g_ll, g_lr, g_rr, g_rl, crop ? c.rg_all_crop : c.rg_all, xi, s);
    else
    for (int l = 0; l < Lc; ++l, ++xi) {
      const bool share = rec_share && l == 0;
      RunGroup rr = share ? g_rr0 : g_rr;
      if (nu && l < Lc - 1) rr.rb_ready = c.rb_l[l];
      const std::vector<RunGroup> full = {g_ll, g_lr, rr, g_rl}, ligs = {g_ll, g_lr};
      std::vector<RunGroup> next;
      if (nu && l + 1 < Lc) {
        if (l + 1 < Lc - 1) next = {g_ll, g_lr, g_rr, g_rl}; else next = ligs;
      }
      const int pq = !nu ? 0 : l == 0 ? 1 : 2;
      const ConvW* Ln = next.empty() ? nullptr : &m.conv_layers[l + 1];
      if (l < Lc - 1)
        run_conv(m, m.conv_layers[l], full, share ? c.rg_all_share : crop ? c.rg_all_crop : c.rg_all, 4, c.X[xi], c.X[xi + 1], 0, c.N, s, pq, Ln,
                 Ln ? &next : nullptr);
      else run_conv(m, m.conv_layers[l], ligs, c.rg_lig, 2, c.X[xi], c.X[xi + 1], 0, cfg.sidechain_pred ? c.N : nL, s, pq);
      // (sidechain_pred reads the RECEPTOR rows of the last table: in the reference the last layer writes them too -- no message
      // reaches them, so they are BatchNorm(0) + the padded input row, cg_model.py:345-349 -- the score read-outs only need the ligand rows)
    }
  }
  const float* XL = c.X[xi];
  c.x_last = conf ? nullptr : XL;   // (a confidence pass leaves no table for ddmi_sidechain_pred to read)
  PhaseTimer t_read(m, "readouts", s);
  if (conf) {   // cg_model.py:353-366: graph-mean of the even (and, from 3 layers on, the odd) scalars -> confidence_predictor
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
    return;
  }
  score_readouts(m, XL, lig_pos, t_tr, t_rot, t_tor, tr_out, rot_out, tor_out, s);
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

// ========================================================================= conformer / sampling
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
}

void modify_conformer(Model& m, float* lig_pos, const float* tr, const float* rot, const float* tor, hipStream_t s) {
  DDMI_REQUIRE(m.has_complex, DDMI_ERR_STATE, "ddmi_set_complex must precede ddmi_modify_conformer");
  Cx& c = *m.cx;
  if (c.layout) {
    launch_modify_conformer_ragged(lig_pos, c.B, c.maxNl, c.lig_ptr, c.tor_ptr, c.rot_lu, c.rot_lv, c.mask_off, c.mask_all, tr, rot,
                                   c.nT > 0 ? tor : nullptr, s);
    return;
  }
  DDMI_REQUIRE(c.uniform && c.Nl_one > 0, DDMI_ERR_STATE,
               "modify_conformer needs a batch of copies of one complex (utils/diffusion_utils.py:60-64)");
  const bool torsion = tor != nullptr && c.R_one > 0;
  DDMI_REQUIRE(!torsion || c.mask_rotate, DDMI_ERR_STATE, "mask_rotate was not provided to ddmi_set_complex");
  launch_modify_conformer(lig_pos, c.B, c.Nl_one, torsion ? c.R_one : 0, c.rot_u, c.rot_v, c.mask_rotate, tr, rot,
                          torsion ? tor : nullptr, s);
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
static void perturb_step(Model& m, float* tr, float* rot, float* tor, const ddmi_sample_cfg& sc, int k,
                         const long long* ids_dev, hipStream_t s) {
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

void sample(Model& m, float* lig_pos, const ddmi_sample_cfg& sc, hipStream_t s) {
  DDMI_REQUIRE(m.has_complex, DDMI_ERR_STATE, "ddmi_set_complex must precede ddmi_sample");
  check_sample_cfg(m, sc);
  Cx& c = *m.cx;
  const ddmi_config& cfg = m.cfg;
  const int steps = sc.inference_steps, B = c.B;
  const bool torsion = !cfg.no_torsion && c.nT > 0;
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
    perturb_step(m, c.s_tr, c.s_rot, torsion ? c.s_tor : nullptr, sc, k, ids_dev, s);
#ifdef DDMI_PROFILING   // timing-only ablation builds produce garbage scores: DDMI_FREEZE_POSE keeps the graphs fixed (never in the shipped library)
    static const bool freeze = getenv("DDMI_FREEZE_POSE") != nullptr;
#else
    constexpr bool freeze = false;
#endif
    if (!freeze) modify_conformer(m, lig_pos, c.s_tr, c.s_rot, torsion ? c.s_tor : nullptr, s);
  }
  c.x_last = nullptr;   // ddmi_sidechain_pred belongs to the ddmi_forward it follows: the loop's tables are not an answer to it
}

}  // namespace ddmi
