// The TensorProductConvLayers of a forward in the node-contracted form (k_conv.hip): virtual-node list upkeep, the plan of a layer
// (which runner, which kernel route and buffers per edge group -- decided by plan_layer before anything is launched) and the three
// runners that issue it: joined (per-group launches on two streams, one node update), grouped (ddmi_exec_options.grouped) and
// overlapped layer boundaries (ddmi_exec_options.layer_overlap).
#include <cmath>
#include <cstdio>
#include <numeric>
#include <string>

#include "cx.h"

namespace ddmi {
namespace {

// tiles of 16 virtual nodes of an edge group ~ gather nodes x ceil(mean degree / 32) / 16
long tiles_of(const RunGroup& q) {
  const long gn = std::max(1, q.gcount);
  return std::max(1L, gn * (((long)q.ea_rows / gn + 31) / 32) / 16);
}
// a launch of this many tiles fills the chip once; a SMALL layer has no such group.  (A constant, not Routes::n_cus: only the
// round model of pick_tile_split reads the device's CU count.)
constexpr long CHIP_TILES = 256;
bool chip_filling(long tiles) { return tiles >= CHIP_TILES; }

// =========================================================================== virtual-node lists
// Virtual-node lists and per-edge rows of an edge group (k_vn_count -> scan -> k_vn_fill -> k_vn_rows [-> k_vn_tiles]): built on the
// first use in a forward, rebuilt when any input they bake in changes.
bool vn_fresh(const Cx& c, const RunGroup& g) {
  const Cx::VnSet& vs = c.vn[g.vn];
  return vs.built_goff == g.goff && (vs.epoch == c.epoch || (g.static_topo && vs.epoch >= 0)) && vs.built_tgt == g.tgt && vs.built_tslot == g.tslot &&
         vs.built_arow == g.arow && vs.built_nvec == g.nvec && vs.built_ew == g.ew && vs.built_sgn == g.sgn && vs.built_tbase == g.tbase;
}
void vn_mark_built(Cx& c, const RunGroup& g) {
  Cx::VnSet& vs = c.vn[g.vn];
  vs.built_goff = g.goff; vs.epoch = c.epoch; vs.built_tgt = g.tgt; vs.built_tslot = g.tslot; vs.built_arow = g.arow;
  vs.built_nvec = g.nvec; vs.built_ew = g.ew; vs.built_sgn = g.sgn; vs.built_tbase = g.tbase;
}
VnRowsArgs vn_rows_args(const Model& m, const RunGroup& g) {
  const Cx::VnSet& vs = m.cx->vn[g.vn];
  VnRowsArgs vr{};
  vr.arow = g.arow; vr.nvec = g.nvec; vr.ew = g.ew; vr.tslot = g.tslot; vr.sgn = g.sgn; vr.sh_lmax = m.cfg.sh_lmax;
  vr.tgt = g.tgt; vr.tbase = g.tbase;
  vr.vcap = vs.vcap; vr.rows = vs.rows; vr.vn_ne = vs.ne;
  return vr;
}
// live virtual nodes of a group's list (device): the padded count under tile_per_pose, else the end of the offsets
const int* vn_count(const Cx& c, const RunGroup& g) {
  const Cx::VnSet& vs = c.vn[g.vn];
  return vs.nvn_pad ? vs.nvn_pad : vs.voff + g.gcount;
}
// tile_per_pose: the graph of every gather node of a list -- ligand / receptor / atom rows of the node table (all null: dense lists)
VnPoseTiles pose_tiles(const Cx& c, int vn) {
  static const char vn_type[10] = {'R', 'R', 'L', 'L', 'A', 'A', 'A', 'L', 'R', 'R'};   // gather-node type of every list (set_complex)
  const Cx::VnSet& vs = c.vn[vn];
  if (!vs.nvn_pad) return VnPoseTiles{};
  const bool lig = vn_type[vn] == 'L', atom = vn_type[vn] == 'A';
  return VnPoseTiles{lig ? c.lig_batch : atom ? c.atom_batch : c.rec_batch, lig ? c.lig_ptr : atom ? c.atom_ptr : c.rec_ptr, vs.graphs, vs.nvn_pad};
}
void build_tile_headers(Cx& c, const RunGroup& g, hipStream_t gs) {   // in-tile pre-reduction of the lig<-rec group (list 0)
  Cx::VnSet& vs = c.vn[0];
  launch_vn_tiles(vn_count(c, g), vs.vcap, vs.rows, vs.ne, vs.tile_hdr, vs.live, gs);
}
// the stale lists of a layer's groups in two launches (+ the tile headers of the pre-reduced group)
void ensure_vn_all(Model& m, const RunGroup* groups, int n, hipStream_t gs) {
  Cx& c = *m.cx;
  VnListsArgs LA;
  VnRowsArgs rows[VN_GROUPS_MAX];
  const RunGroup* built[VN_GROUPS_MAX];
  const RunGroup* prered_g = nullptr;
  for (int gi = 0; gi < n; ++gi) {
    const RunGroup& g = groups[gi];
    if (vn_fresh(c, g) || g.gcount <= 0) continue;
    bool queued = false;   // (a list is built once per launch even if two groups name it)
    for (int i = 0; i < LA.n; ++i) queued = queued || built[i]->vn == g.vn;
    if (queued) continue;
    DDMI_REQUIRE(LA.n < VN_GROUPS_MAX, DDMI_ERR_CAPACITY, "more edge groups than virtual-node list slots");
    Cx::VnSet& vs = c.vn[g.vn];
    const VnPoseTiles pp = pose_tiles(c, g.vn);
    LA.g[LA.n] = VnListArgs{g.goff, g.gcount, vs.voff, vs.node, vs.e0, pp.node_batch, pp.graph_ptr, pp.n_graphs, pp.nvn_pad};
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
  if (prered_g && m.cfg.sh_lmax > 1) build_tile_headers(c, *prered_g, gs);
  for (int i = 0; i < LA.n; ++i) vn_mark_built(c, *built[i]);   // only once every launch went out (a throw leaves the lists stale)
}
void ensure_vn(Model& m, const RunGroup& g, hipStream_t gs) {
  Cx& c = *m.cx;
  Cx::VnSet& vs = c.vn[g.vn];
  if (vn_fresh(c, g)) return;
  PhaseTimer t(m, "vn_build", gs);
  const VnPoseTiles pp = pose_tiles(c, g.vn);
  launch_vn_build(g.goff, g.gcount, vs.cnt, vs.voff, vs.node, vs.e0, vn_rows_args(m, g), gs, pp.node_batch ? &pp : nullptr);
  if (g.vn == 0 && c.prered) build_tile_headers(c, g, gs);
  vn_mark_built(c, g);
}

// ========================================================================================= plans
// How an edge group's hidden rows (first Linear + ReLU of the per-edge weight MLP) are made: mm = inside k_edge_hidden_mm, straight
// from the edge attributes and the per-node terms P / Q; gemm = per-edge GEMM + k_edge_hidden; deep = FCBlock with hidden Linear
// layers (tp_weights_layers > 2): first layer as plain per-edge rows, the hidden ones as GEMMs.
enum class Hidden { mm, gemm, deep };
Hidden hidden_route(const Model& m, const ConvW& L, int wg) {
  if (L.TL > 2) return Hidden::deep;
  return m.r.hidden_mm && m.ns % 16 == 0 && m.ns <= 64 && L.W1p[wg] ? Hidden::mm : Hidden::gemm;
}
int weight_group(const ConvW& L, int gi) { return std::min(gi, L.G - 1); }

// row mode / arithmetic of an edge group's fused launch
struct GroupRoute { bool bf, dense_rows; };
GroupRoute group_route(const Model& m, const ConvW& L, const RunGroup& g) {
  GroupRoute r;
  // split-bf16 edge product (ddmi_config.edge_product = 1): the static l <= 1 loops only; other layers keep the f32 route
  r.bf = m.cfg.edge_product == 1 && !L.fgran_generic && L.maxd <= 3 && m.cfg.sh_lmax <= 1;
  // dense-row loop: groups with >= 20 edges per gather node (both row tiles of every virtual node are multiplied)
  r.dense_rows = m.r.dense_rows == Use::always || (m.r.dense_rows == Use::by_rule && (long)g.ea_rows >= 20L * std::max(1, g.gcount));
  return r;
}

struct GroupPlan {
  int wg = 0;                    // weight group of the layer
  bool side = false;             // side stream and its scratch set
  Hidden hidden = Hidden::mm;
  GroupRoute rt{};
  bool shared = false;           // shared-node tiles (mode 4 of k_conv_fused)
  float *P = nullptr, *Q = nullptr, *rowbias = nullptr, *Hb = nullptr;   // per-node / per-graph terms of the first Linear, hidden rows
  const float* rb = nullptr;     // the per-graph term the hidden rows add (rowbias, the group's rb_ready, or none)
  bool last_on_stream = false;   // last chip-filling fused launch of its stream in the layer (exec.tile_split_last)
  int ysplit = 1;                // workgroups per tile; the granule ranges follow from it (fill_granule_ranges)
  int hidden_grid = 0;           // workgroups of the group's k_edge_hidden_mm work
};
struct LayerPlan {
  enum Runner { joined, grouped, overlapped } runner = joined;
  bool forked = false;           // ligand-gather groups on the side stream
  bool small_layer = false;      // no group fills the chip once
  bool mm_all = false;           // P / Q / sigma rows of every group in the layer's buffers Pg / Qg / rbg (one launch, or the previous layer's k_node_update)
  int pq_mode = 0;               // run_conv
  int n = 0;
  GroupPlan g[VN_GROUPS_MAX];
  int issue[VN_GROUPS_MAX] = {}; // order the groups are issued in
};

// Workgroups per tile (granule ranges) of a group's fused launch.  ys_force > 0: chosen by the caller.
int pick_tile_split(const Model& m, const ConvW& L, const RunGroup& g, bool small_layer, int ys_force) {
  const Routes& r = m.r;
  const long T = tiles_of(g);
  // one workgroup per CU, so a launch of T x ys work items runs in ceil(T ys / CUs) rounds of (granules per item + tile prologue
  // ~ 0.2 granules): the split with the cheapest schedule
  auto round_model = [&]() {
    int pick = 1;
    double best = 1e30;
    for (int y = 1; y <= std::min(8, L.n_fgran); ++y) {
      const double rounds = std::ceil((double)T * y / (double)r.n_cus);
      const double cost = rounds * ((double)((L.n_fgran + y - 1) / y) + 0.2);
      if (cost < best - 1e-9) { best = cost; pick = y; }
    }
    return pick;
  };
  int ys = ys_force > 0 ? ys_force : r.tile_split;
  if (ys <= 0) {   // 0 = spread a launch with few tiles over the CUs
    // Small batches: up to one granule per workgroup, 5 poses 94 -> 100 poses/s.  Otherwise the round-2 rule (at most 6 ranges, tiles
    // estimated from nodes + edges / 32): the small lig-lig launch that runs next to the big groups is sensitive to its split -- 4
    // ranges at 40 poses; 5-6 cost the headline 2.5 % (profiles/r03_e27..e37_ab.txt).
    if (small_layer && r.round_split_small && T >= 32) ys = round_model();
    else if (small_layer) ys = (int)std::min(8L, std::max(1L, 768 / T));
    // Chip-filling group (round 6).  The old rule gave every group of >= 256 tiles ONE item per tile: 375 tiles (20 poses) = 1.46
    // rounds, i.e. two rounds with the second half empty -- 138.2 poses/s against 145.1 with the last launch of each stream split in
    // four (profiles/r06_p6_b20_ab.txt); 750 tiles (40 poses) = 2.93 rounds keep one item per tile.
    else if (r.round_split && T >= r.n_cus) ys = round_model();
    else ys = (int)std::min(6L, std::max(1L, 768 / std::max(1L, ((long)g.gcount + g.ea_rows / 32) / 16)));
    if (r.tile_split_small > 0 && !small_layer && !chip_filling(T)) ys = r.tile_split_small;   // tuning: a small group next to big ones
  }
  ys = std::max(ys, (L.n_fgran + 19) / 20);   // a workgroup keeps at most 24 granule descriptors in LDS
  return std::max(1, std::min(std::min(ys, 8), L.n_fgran));
}
void fill_granule_ranges(const ConvW& L, int ys, FusedConvArgs& f) {
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
}

// Every route decision of one layer over `groups`, from the options, the layer and the group sizes.  Launches nothing, allocates
// nothing.  overlapped: the layer is issued by run_conv_layers_overlapped (groups = [ll, lr, rr, rl] or [ll, lr]).
//
// Joined runner.  Groups whose gather nodes are ligand atoms (few nodes, many edges each: MFMA-bound) run on the side stream with
// their own scratch, concurrently with the receptor-gather groups (HBM-bound on the contracted rows).  The per-graph and per-node
// terms of the first Linear of EVERY group (P = W1s x_target, Q = W1d x_gather + b1, sigma rows) depend on the layer input only.
// Small layers: one batched launch in front of the fork instead of one small launch at the head of every group's chain (5 poses:
// 101.4 -> 102.9 poses/s).  Large layers keep them per group: there the other stream fills the gap, and a common launch in front
// of the fork delays the side stream (40 poses: -0.5 %; profiles/r03_e42_ab.txt).
// Grouped runner (not the default: it shortens the time covered by fused workgroups by 3-5 % but leaves the hidden rows of the whole
// layer exposed in front of it -- 151.5 against 155.2 poses/s at 40 poses, 124.8 / 127.3 at 10, 106.8 / 107.9 at 5,
// profiles/r06_p2_*).  Supported: exact-f32 l <= 1 layers with static chain shapes, two-layer edge MLPs (the benchmark preset);
// anything else takes the per-group path.
LayerPlan plan_layer(const Model& m, const ConvW& L, const RunGroup* groups, int n, int pq_mode, bool overlapped) {
  const Cx& c = *m.cx;
  const Routes& r = m.r;
  DDMI_REQUIRE(n <= VN_GROUPS_MAX, DDMI_ERR_CAPACITY, "more edge groups in a layer than plan slots");
  LayerPlan P;
  P.n = n; P.pq_mode = pq_mode;
  auto lig_gather = [&](const RunGroup& g) { return g.gbase == 0 && g.gcount == c.nL; };   // a side-stream group
  long biggest = 1, tiles = 0;
  bool any_side = false, any_main = false, all_mm = true, all_lists = true;
  for (int gi = 0; gi < n; ++gi) {
    const RunGroup& g = groups[gi];
    GroupPlan& p = P.g[gi];
    p.wg = weight_group(L, gi);
    p.hidden = hidden_route(m, L, p.wg);
    p.rt = group_route(m, L, g);
    // ligand gather nodes with >= 2 virtual nodes on average (rec<-lig): a tile of 16 virtual nodes holds few distinct nodes
    p.shared = p.rt.dense_rows && (r.shared_tiles == Use::always ||
                                   (r.shared_tiles == Use::by_rule && g.load && (long)g.ea_rows >= 48L * std::max(1, g.gcount)));
    biggest = std::max(biggest, tiles_of(g)); tiles += tiles_of(g);
    any_side = any_side || (lig_gather(g) && c.nR > 0); any_main = any_main || !lig_gather(g);
    all_mm = all_mm && p.hidden == Hidden::mm; all_lists = all_lists && g.vn >= 0;
    P.issue[gi] = gi;
  }
  P.forked = overlapped || (r.two_streams && m.side_stream && n > 1 && any_side && any_main);
  P.small_layer = !overlapped && !chip_filling(biggest);
  const bool layer_buffers = all_mm && n <= 9 && c.Pg[0];
  if (overlapped) P.runner = LayerPlan::overlapped;
  else if (r.grouped == 2 && layer_buffers && c.Hbg[0] && n >= 2 && all_lists && !L.fgran_generic && L.maxd <= 3 && m.cfg.sh_lmax <= 1 &&
           L.n_fgran > 0 && m.cfg.edge_product == 0 && !(m.timing && m.timing_level >= 2) &&   // (per-group timing rows need per-group launches)
           !(m.cfg.all_atoms && m.crop_cutoff > 0.0))   // (an all-atom crop takes the per-group path)
    P.runner = LayerPlan::grouped;
  const bool is_grouped = P.runner == LayerPlan::grouped;
  P.mm_all = is_grouped || (!overlapped && (pq_mode != 0 || (r.fc1_batch && P.small_layer)) && layer_buffers);
  DDMI_REQUIRE(pq_mode == 0 || P.mm_all, DDMI_ERR_STATE, "fused node-update route on a layer without batched first-Linear terms");
  // grouped: all groups of the layer share the chip, so the split follows the layer's total tile count
  const int ys_grouped = r.grouped_split > 0 ? r.grouped_split : (int)std::min(8L, std::max(1L, (long)r.grouped_target / std::max(1L, tiles)));
  if (is_grouped) {
    // launch order: the groups with the longest work items first (dense residue / atom gathers), sparse-row groups last -- the short
    // items of the small groups fill the tail of the launch
    std::stable_sort(P.issue, P.issue + n, [&](int a, int b) {
      if (P.g[a].rt.dense_rows != P.g[b].rt.dense_rows) return P.g[a].rt.dense_rows;
      return tiles_of(groups[a]) > tiles_of(groups[b]);
    });
  } else if (P.forked && r.group_order != 0 && !overlapped) {
    // issue order of the groups (exec.group_order, A/B knob): bit 0 = the side stream's groups in reverse order (rec<-lig in front of
    // lig-lig: the short lig-lig items then fill the layer's tail), bit 1 = the main stream's groups in reverse order
    int k = 0;
    for (int pass = 0; pass < 2; ++pass) {
      const int k0 = k;
      for (int gi = 0; gi < n; ++gi) if (lig_gather(groups[gi]) == (pass == 1)) P.issue[k++] = gi;
      if ((r.group_order >> (pass == 1 ? 0 : 1)) & 1) std::reverse(P.issue + k0, P.issue + k);
    }
  }
  bool seen_side = false, seen_main = false;
  for (int ii = n - 1; ii >= 0; --ii) {   // back to front: the first group met on a stream is its last launch
    const int gi = P.issue[ii];
    const RunGroup& g = groups[gi];
    GroupPlan& p = P.g[gi];
    p.side = !is_grouped && P.forked && lig_gather(g);
    bool& seen = p.side ? seen_side : seen_main;
    // exec.tile_split_last: the LAST fused launch of each stream in finer work items -- the launch whose final partial round of
    // workgroups is the layer's straggler tail (workgroup stamps: 0.46 ms per forward with < 32 of 256 CUs busy, profiles/r06_p2_wg_idle_b40_g1.txt)
    p.last_on_stream = P.runner == LayerPlan::joined && !seen && r.tile_split_last > 0 && !P.small_layer && chip_filling(tiles_of(g));
    seen = true;
    p.P = P.mm_all ? c.Pg[gi] : p.side ? c.P_b : c.P;
    p.Q = P.mm_all ? c.Qg[gi] : p.side ? c.Q_b : c.Q;
    p.rowbias = P.mm_all ? c.rbg[gi] : p.side ? c.rowbias_b : c.rr_rowbias;
    p.rb = !g.sig ? nullptr : g.rb_ready ? g.rb_ready : p.rowbias;
    p.Hb = is_grouped ? c.Hbg[g.vn] : p.side ? c.Hb_b : c.Hb;
    p.ysplit = pick_tile_split(m, L, g, P.small_layer, is_grouped ? ys_grouped : p.last_on_stream ? r.tile_split_last : 0);
    // grouped: the launch's workgroups dealt by tile count
    p.hidden_grid = is_grouped ? std::max(64, (int)((long)r.hidden_grid * tiles_of(g) / std::max(1L, tiles))) : r.hidden_grid;
  }
  return P;
}

// ======================================================================================= runners
// The terms of a group's first Linear that do not depend on the edge, from the permuted weights W1p (emission order of
// k_edge_hidden_mm): the sigma row bias W1e . sig per graph (base = -1; only with `sigma`, and not when the group brings its own),
// P = W1s x_target, Q = W1d x_gather + b1 per node.  fn(W, bias, out, first node, nodes).
template <class F> void for_fc1_terms(const Model& m, const ConvW& L, const RunGroup& g, int wg, float* P, float* Q, float* rowbias, bool sigma, F&& fn) {
  const float* W1p = L.W1p[wg];
  if (sigma && g.sig && !g.rb_ready) fn(W1p, (const float*)nullptr, rowbias, -1, m.cx->B);
  fn(W1p + (g.swap_pq ? 2 : 1) * m.ns, (const float*)nullptr, P, g.tbase, g.tcount);
  fn(W1p + (g.swap_pq ? 1 : 2) * m.ns, (const float*)L.b1p[wg], Q, g.gbase, g.gcount);
}
// ... of groups [g0, g1) as independent GEMMs of one launch
void launch_fc1_terms(Model& m, const ConvW& L, const RunGroup* groups, const LayerPlan& P, int g0, int g1, const float* Xin, hipStream_t s) {
  PhaseTimer t(m, "conv_fc1_gemms", s);
  GemmBatch gb;
  for (int gi = g0; gi < g1; ++gi) {
    const RunGroup& g = groups[gi];
    const GroupPlan& p = P.g[gi];
    for_fc1_terms(m, L, g, p.wg, p.P, p.Q, p.rowbias, true, [&](const float* W, const float* bias, float* C, int base, int count) {
      GemmArgs& x = batch_add(gb, s);
      if (base < 0) { x.A = g.sig; x.lda = m.ns; } else { x.A = Xin + (size_t)base * XS; x.lda = XS; }
      x.W = W; x.ldw = L.n_edge; x.bias = bias; x.C = C; x.ldc = L.H; x.M = count; x.N = L.H; x.K = m.ns;
    });
  }
  launch_gemm_batch(gb, s);
}

// arguments of k_edge_hidden_mm for one edge group (first Linear straight from the edge attributes)
EdgeHiddenArgs hidden_args(Model& m, const ConvW& L, const RunGroup& g, const GroupPlan& p) {
  Cx& c = *m.cx;
  Cx::VnSet& vs = c.vn[g.vn];
  EdgeHiddenArgs h{};
  h.nvn = vn_count(c, g);
  h.vcap = vs.vcap; h.vn_node = vs.node; h.vn_e0 = vs.e0; h.goff = g.goff; h.arow = g.arow; h.tgt = g.tgt;
  h.tbase = g.tbase; h.ea = g.ea; h.ns = m.ns; h.W1 = L.W1p[p.wg]; h.ldw = L.n_edge; h.P = p.P; h.Q = p.Q; h.rowbias = p.rb; h.ridx = g.sig_idx;
  h.H = L.H; h.NG8 = L.HKq / 8; h.Hb = p.Hb; h.bf = p.rt.bf ? 1 : 0;
  h.zero_fill = (!L.fgran_generic && p.rt.dense_rows) ? 1 : 0;
  if (m.cfg.sh_lmax <= 1) { h.vrows = vs.rows; h.vn_ne = vs.ne; }
  h.grid = p.hidden_grid;
  return h;
}
// arguments of the fused convolution for one edge group
FusedConvArgs fused_args(Model& m, const ConvW& L, const RunGroup& g, int gi, const GroupPlan& p, const float* Xin) {
  Cx& c = *m.cx;
  Cx::VnSet& vs = c.vn[g.vn];
  FusedConvArgs f{};
  f.nvn = vn_count(c, g);
  f.vcap = vs.vcap; f.vn_node = vs.node; f.vrows = vs.rows; f.vn_ne = vs.ne;
  f.X = Xin; f.gbase = g.gbase; f.wpack = L.wpack[p.wg]; f.KS = L.KS; f.HK = L.HK; f.Hb = p.Hb; f.NG8 = L.HKq / 8;
  f.sh_lmax = m.cfg.sh_lmax; f.gran = L.fgran; f.cgt = L.cgt;
  f.max_nb = L.max_nb; f.maxd = L.maxd; f.msg = g.msg; f.generic = L.fgran_generic ? 1 : 0;
  f.dense = p.rt.dense_rows ? 1 : 0;
  f.bf = p.rt.bf ? 1 : 0;
  f.tile_hdr = (g.vn == 0 && c.prered) ? vs.tile_hdr : nullptr;
  f.shared = p.shared ? 1 : 0;
  f.prof_slot = gi;
  fill_granule_ranges(L, p.ysplit, f);
  return f;
}

// One edge group of a layer on stream gs, as its plan says: per-graph / per-node terms of the first Linear (unless mm_all: they are
// there), virtual-node lists (first use in this forward), hidden rows, fused launch.
// Every edge group runs k_conv_fused (a node-contracted layer always has its granule list; ligand gather nodes with many edges are
// cut into 32-edge virtual nodes like the others -- several virtual nodes of an atom share its contraction in the shared-node
// tiles, mode 4 of the kernel).
void run_group(Model& m, const ConvW& L, const RunGroup* groups, int gi, const LayerPlan& LP, const float* Xin, hipStream_t gs) {
  Cx& c = *m.cx;
  const RunGroup& g = groups[gi];
  const GroupPlan& p = LP.g[gi];
  const int ns = m.ns, H = L.H;
  DDMI_REQUIRE(g.vn >= 0 && L.n_fgran > 0 && c.Hb, DDMI_ERR_STATE, "convolution layer without a granule list / virtual-node set");
  if (m.cfg.exec.debug & 1)   // the route this group takes, for tests: hidden rows (mm / gemm / deep) and the granule loops
    fprintf(stderr, "ddmi route %s g%d: hidden %s granules %s\n", L.name.c_str(), gi,
            p.hidden == Hidden::mm ? "mm" : p.hidden == Hidden::deep ? "deep" : "gemm", L.fgran_generic ? "generic" : "static");
  float* HE = p.side ? c.HE_b : c.HE;
  if (LP.mm_all) {
  } else if (p.hidden == Hidden::mm) {
    launch_fc1_terms(m, L, groups, LP, gi, gi + 1, Xin, gs);
  } else {
    PhaseTimer t(m, "conv_fc1_gemms", gs);
    const float* W1 = L.W1[p.wg];
    if (g.sig) gemm(g.sig, ns, W1, L.n_edge, nullptr, p.rowbias, H, c.B, H, ns, 0, gs);   // W1e * (edge_attr + sig[b]) = W1e*edge_attr + (W1e*sig)[b]
    gemm(g.ea, ns, W1, L.n_edge, nullptr, HE, H, g.ea_rows, H, ns, 0, gs, g.ea_rows_dev, p.rb, g.sig_idx, H);
    gemm(Xin + (size_t)g.tbase * XS, XS, W1 + (g.swap_pq ? 2 : 1) * ns, L.n_edge, nullptr, p.P, H, g.tcount, H, ns, 0, gs);
    gemm(Xin + (size_t)g.gbase * XS, XS, W1 + (g.swap_pq ? 1 : 2) * ns, L.n_edge, L.b1[p.wg], p.Q, H, g.gcount, H, ns, 0, gs);
  }
  ensure_vn(m, g, gs);
  Cx::VnSet& vs = c.vn[g.vn];
  const int* nvn = vn_count(c, g);
  const int bf = p.rt.bf ? 1 : 0;
  if (p.hidden == Hidden::mm) {
    PhaseTimer t(m, "k_edge_hidden", gs);
    launch_edge_hidden_mm(hidden_args(m, L, g, p), gs);
  } else if (p.hidden == Hidden::deep) {
    PhaseTimer t(m, "k_edge_hidden", gs);
    float* cur = p.side ? c.HD_b[0] : c.HD[0];
    float* nxt = p.side ? c.HD_b[1] : c.HD[1];
    DDMI_REQUIRE(cur && nxt, DDMI_ERR_STATE, "tp_weights_layers > 2: hidden-row scratch missing");
    launch_edge_rows(nvn, vs.vcap, vs.node, vs.e0, g.goff, g.arow, g.tgt, g.tbase, HE, p.P, p.Q, H, cur, gs);
    for (int j = 0; j + 2 < L.TL; ++j) {   // hidden Linear + ReLU layers (models/layers.py:14-15), rows in gather order
      gemm(cur, H, L.Wmid[p.wg][j], H, L.bmid[p.wg][j], nxt, H, g.ea_rows, H, H, 1, gs, g.ea_rows_dev);
      std::swap(cur, nxt);
    }
    launch_edge_hidden(nvn, vs.vcap, vs.node, vs.e0, g.goff, nullptr, g.tgt, g.tbase, cur, nullptr, nullptr, H, L.HKq / 8, p.Hb, gs, bf);
  } else {
    PhaseTimer t(m, "k_edge_hidden", gs);
    launch_edge_hidden(nvn, vs.vcap, vs.node, vs.e0, g.goff, g.arow, g.tgt, g.tbase, HE, p.P, p.Q, H, L.HKq / 8, p.Hb, gs, bf);
  }
  const FusedConvArgs f = fused_args(m, L, g, gi, p, Xin);
  std::string tname = "k_conv_fused";
  if (m.timing && m.timing_level >= 2)   // ddmi_set_kernel_timing(h, 2 | 3): one timing row per edge group / per (layer, edge group)
    tname += ":" + (m.timing_level >= 3 ? "L" + L.name.substr(L.name.size() - 1) : std::string()) + "g" + std::to_string(gi);
  PhaseTimer t(m, tname.c_str(), gs);
  launch_conv_fused(f, gs);
}

// Grouped dispatch of a layer (round 6, ddmi_exec_options.grouped): on ONE stream, [per-node terms of the first Linear of every
// group: one launch] -> [hidden rows of every group: one launch, each group into its own buffer] -> [k_conv_grouped: the work
// items of every group in one grid].  Same device code and arguments per work item as the per-group launches (bit-identical
// messages); what changes is that no group waits for another one's launch to drain, a small group (lig-lig: 10-79 tiles) never
// has the chip to itself, and a layer is 4 launches instead of ~11.
void run_groups_grouped(Model& m, const ConvW& L, const RunGroup* groups, const LayerPlan& P, const float* Xin, hipStream_t s) {
  if (P.pq_mode != 2) launch_fc1_terms(m, L, groups, P, 0, P.n, Xin, s);
  ensure_vn_all(m, groups, P.n, s);
  for (int o0 = 0; o0 < P.n; o0 += FC_GROUPS_MAX) {
    const int n = std::min(FC_GROUPS_MAX, P.n - o0);
    EdgeHiddenGroupedArgs HG;
    FusedGroupedArgs FG;
    HG.n = FG.n = n;
    for (int k = 0; k < n; ++k) {
      const int gi = P.issue[o0 + k];
      HG.g[k] = hidden_args(m, L, groups[gi], P.g[gi]);
      FG.g[k] = fused_args(m, L, groups[gi], gi, P.g[gi], Xin);
    }
    {
      PhaseTimer t(m, "k_edge_hidden", s);
      launch_edge_hidden_mm_grouped(HG, s);
    }
    PhaseTimer t(m, "k_conv_fused", s);
    launch_conv_grouped(FG, s);
  }
}

// A layer's node update on rows [nbase, nbase + ncount): mean over the groups' messages + BatchNorm + residual (k_reduce_bn); with
// Lnext / gnext also the next layer's P / Q (k_node_update, into the layer buffers Pg / Qg)
void node_update(Model& m, const ConvW& L, const ReduceGroup* rg_dev, int n_rg, int nbase, int ncount, const float* Xin, float* Xout,
                 hipStream_t s, const ConvW* Lnext = nullptr, const std::vector<RunGroup>* gnext = nullptr) {
  Cx& c = *m.cx;
  const BnArgs bn = bn_args(L);
  PhaseTimer t(m, "k_reduce_bn", s);   // (one timer row for both kernels: the scatter stage of the layer)
  if (!Lnext) {
    launch_reduce_bn(rg_dev, n_rg, nbase, ncount, L.D_in, L.D_out, bn.mean, bn.scale, bn.bias, L.residual ? 1 : 0, Xin, Xout, XS, s);
    return;
  }
  DDMI_REQUIRE(rg_dev != c.rg_all_share, DDMI_ERR_STATE, "k_node_update does not fold message rows onto graph 0 (ReduceGroup::tmod)");
  NodeUpdateArgs a{};
  a.groups = rg_dev; a.n_groups = n_rg; a.nbase = nbase; a.ncount = ncount; a.D_in = L.D_in; a.D_out = L.D_out;
  a.bn_mean = bn.mean; a.bn_scale = bn.scale; a.bn_bias = bn.bias;
  a.residual = L.residual ? 1 : 0; a.X_in = Xin; a.X_out = Xout;
  a.ns = m.ns; a.H = Lnext->H; a.ldw = Lnext->n_edge; a.wpn = m.r.node_update_wpn;
  for (size_t gi = 0; gi < gnext->size(); ++gi) {
    DDMI_REQUIRE(a.n_terms + 2 <= NU_TERMS_MAX, DDMI_ERR_CAPACITY, "k_node_update: more first-Linear terms than slots");
    for_fc1_terms(m, *Lnext, (*gnext)[gi], weight_group(*Lnext, (int)gi), c.Pg[gi], c.Qg[gi], nullptr, false,
                  [&](const float* W, const float* bias, float* out, int base, int count) { a.term[a.n_terms++] = NodeTerm{W, bias, out, base, count}; });
  }
  launch_node_update(a, s);
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
void run_conv_layers_overlapped(Model& m, const RunGroup* groups /* [ll, lr, rr, rl] */, const ReduceGroup* rg, int& xi, hipStream_t s) {
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
  DDMI_CHECK_HIP(hipEventRecord(m.ev_fork, s));            // the layer-0 table
  DDMI_CHECK_HIP(hipStreamWaitEvent(side, m.ev_fork, 0));
  for (int l = 0; l < Lc; ++l, ++xi) {
    const ConvW& L = m.conv_layers[l];
    const float* Xin = c.X[xi];
    float* Xout = c.X[xi + 1];
    const bool last = l == Lc - 1;   // the last layer updates the ligand rows only (cg_model.py:345-349)
    const LayerPlan P = plan_layer(m, L, groups, last ? 2 : 4, 0, true);
    if (l > 0) { wait(side, l - 1, E_RR); wait(side, l - 1, E_RED_L); }
    run_group(m, L, groups, 0, P, Xin, side);
    record(l, E_LL, side);
    run_group(m, L, groups, 1, P, Xin, s);
    wait(s, l, E_LL);
    node_update(m, L, rg, 2, 0, last && m.cfg.sidechain_pred ? c.N : nL, Xin, Xout, s);
    if (last) continue;
    record(l, E_RED_L, s);
    run_group(m, L, groups, 2, P, Xin, s);
    record(l, E_RR, s);
    if (l > 0) wait(side, l - 1, E_RED_R);
    run_group(m, L, groups, 3, P, Xin, side);
    record(l, E_RL, side);
    wait(s, l, E_RL);
    node_update(m, L, rg + 2, 2, nL, nR, Xin, Xout, s);
    record(l, E_RED_R, s);
  }
}

}  // namespace

void run_conv(Model& m, const ConvW& L, const std::vector<RunGroup>& groups, const ReduceGroup* rg_dev, int n_rg,
              const float* Xin, float* Xout, int nbase, int ncount, hipStream_t s, int pq_mode, const ConvW* Lnext,
              const std::vector<RunGroup>* gnext) {
  const int n = (int)groups.size();
  const LayerPlan P = plan_layer(m, L, groups.data(), n, pq_mode, false);
  if (P.runner == LayerPlan::grouped) {
    run_groups_grouped(m, L, groups.data(), P, Xin, s);
    if (rg_dev) node_update(m, L, rg_dev, n_rg, nbase, ncount, Xin, Xout, s, Lnext, gnext);
    return;
  }
  if (P.mm_all && pq_mode != 2) launch_fc1_terms(m, L, groups.data(), P, 0, n, Xin, s);
  // virtual-node lists and per-edge rows of every group whose topology changed since they were built (first layer of a forward):
  // two launches in front of the fork instead of a count -> scan -> fill -> rows chain at the head of every group's stream
  if (m.r.vn_merge) ensure_vn_all(m, groups.data(), n, s);
  if (P.forked) {
    DDMI_CHECK_HIP(hipEventRecord(m.ev_fork, s));
    DDMI_CHECK_HIP(hipStreamWaitEvent(m.side_stream, m.ev_fork, 0));
  }
  // (Measured and dropped in round 4, profiles/r04_e5_ab.txt: the GEMMs / hidden rows of a stream's SECOND group on extra
  // "preparation" streams next to the first group's fused launch.  The time with no k_conv_fused dispatch running stayed at
  // 1.87 ms per forward, the fused launches themselves got 4 % slower -- 27-KB k_edge_hidden_mm workgroups scattered over the
  // CUs keep 158-KB fused workgroups from being placed: 139.8 -> 135.7 poses/s on the same box.)
  for (int ii = 0; ii < n; ++ii) run_group(m, L, groups.data(), P.issue[ii], P, Xin, P.g[P.issue[ii]].side ? m.side_stream : s);
  if (P.forked) {
    DDMI_CHECK_HIP(hipEventRecord(m.ev_join, m.side_stream));
    DDMI_CHECK_HIP(hipStreamWaitEvent(s, m.ev_join, 0));
  }
  if (rg_dev) node_update(m, L, rg_dev, n_rg, nbase, ncount, Xin, Xout, s, Lnext, gnext);
}

// The interaction layers of the CG model over [ll ; lig<-rec ; rec-rec ; rec<-lig] (cg_model.py:329-349), from table c.X[xi] on.
void run_cg_layers(Model& m, const RunGroup& g_ll, const RunGroup& g_lr, const RunGroup& g_rr, const RunGroup& g_rl, bool crop, int& xi,
                   hipStream_t s) {
  Cx& c = *m.cx;
  const Routes& r = m.r;
  const int ns = m.ns, Lc = (int)m.conv_layers.size();
  const RunGroup four[4] = {g_ll, g_lr, g_rr, g_rl};
  const ReduceGroup* rg_all = crop ? c.rg_all_crop : c.rg_all;
  // layer boundaries overlapped on request (ddmi_exec_options.layer_overlap, see run_conv_layers_overlapped): 1 = chip-filling
  // batches (small ones keep the joined form with its one batched first-Linear launch per layer), 2 = every batch
  bool overlapped = r.layer_overlap && r.two_streams && m.side_stream && c.nR > 0 && Lc >= 2;
  if (overlapped && r.layer_overlap != 2) {
    long biggest = 1;
    for (auto& q : four) biggest = std::max(biggest, tiles_of(q));
    overlapped = chip_filling(biggest);
  }
  if (overlapped) { run_conv_layers_overlapped(m, four, rg_all, xi, s); return; }
  // Fused node update (ddmi_exec_options.node_update = 1; not the default: -0.9 %, profiles/r06_p5_*): k_node_update writes a layer's
  // rows AND the next layer's per-node first-Linear terms P / Q, so only the first layer launches its GEMMs; the per-graph sigma term
  // of the rec-rec group of every layer comes from one batched launch here.
  bool nu = r.node_update && Lc >= 2 && c.Pg[0] && (int)c.rb_l.size() == Lc;
  for (auto& L : m.conv_layers) {
    nu = nu && L.H == m.conv_layers[0].H && L.n_edge == m.conv_layers[0].n_edge;
    for (int g = 0; g < 4; ++g) nu = nu && hidden_route(m, L, weight_group(L, g)) == Hidden::mm;
  }
  if (nu) {
    PhaseTimer t(m, "conv_fc1_gemms", s);
    GemmBatch gb;
    for (int l = 0; l < Lc - 1; ++l) {   // (the last layer has no rec-rec group)
      const ConvW& L = m.conv_layers[l];
      GemmArgs& x = batch_add(gb, s);
      x.A = c.rec_sig; x.lda = ns; x.W = L.W1p[weight_group(L, 2)]; x.ldw = L.n_edge; x.C = c.rb_l[l]; x.ldc = L.H; x.M = c.B; x.N = L.H; x.K = ns;
    }
    if (gb.n) launch_gemm_batch(gb, s);
  }
  // Receptor copies under one t (exec.rec_share, ddmi_sample): the first layer's rec-rec group reads receptor rows, edge attributes
  // and the sigma term only -- the same for every graph of the batch -- so it runs on graph 0 (its own list, built once per complex)
  // and the node update reads graph 0's message rows for every graph, in the same order (bit-identical).  Layers >= 1 read
  // pose-dependent receptor rows.  The optional layer routes keep the full group.
  const bool rec_share = r.rec_share && m.uniform_t && c.rec_copies && !crop && !nu && r.grouped != 2 && Lc >= 2;
  RunGroup g_rr0 = g_rr;
  g_rr0.gcount = g_rr0.tcount = c.Rc_one; g_rr0.ea_rows = c.Erc_one; g_rr0.vn = 9; g_rr0.static_topo = true;
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
      run_conv(m, m.conv_layers[l], full, share ? c.rg_all_share : rg_all, 4, c.X[xi], c.X[xi + 1], 0, c.N, s, pq, Ln, Ln ? &next : nullptr);
    else run_conv(m, m.conv_layers[l], ligs, c.rg_lig, 2, c.X[xi], c.X[xi + 1], 0, m.cfg.sidechain_pred ? c.N : c.nL, s, pq);
    // (sidechain_pred reads the RECEPTOR rows of the last table: in the reference the last layer writes them too -- no message
    // reaches them, so they are BatchNorm(0) + the padded input row, cg_model.py:345-349 -- the score read-outs only need the ligand rows)
  }
}

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
  a.form = m.r.tp_form;
  a.z_floats = 0;
  for (auto& p : L.table.paths) a.z_floats += p.mul_in * p.dout;
  launch_tp_apply(a, s);
}

}  // namespace ddmi
