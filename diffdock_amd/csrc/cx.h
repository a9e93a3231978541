// Private to the host orchestration (complex.cpp, conv_layers.cpp, forward.cpp, sample.cpp; not standalone.cpp): the per-complex state Model::Cx, the
// description of an edge group and the few helpers all four share.  Not installed, not included by kernels.
#pragma once
#include <algorithm>
#include <type_traits>

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
  float *atom_sig = nullptr, *aa_sig_old = nullptr, *ar_sig_old = nullptr;   // legacy all-atom class: sigma terms of the atom rows and of the two static atom relations' edge embeddings
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
  // a static atom relation: gather-order CSR (goff, tgt, tslot, arow), target order (toff; tlist = gather-order id of a slot, gnode =
  // gather node of an edge) and its per-step compaction under a crop (launch_rel_filter; the *2 arrays, like goff2.. of rec-rec)
  struct StaticEdges { int E = 0; int *goff = nullptr, *toff = nullptr, *arow = nullptr, *tgt = nullptr, *tslot = nullptr;
                       int *tlist = nullptr, *gnode = nullptr;
                       int *cnt_g = nullptr, *cnt_t = nullptr, *goff2 = nullptr, *toff2 = nullptr, *tslot_tmp = nullptr, *tgt2 = nullptr,
                           *tslot2 = nullptr, *arow2 = nullptr; };
  StaticEdges se_aa, se_ar, se_ra;   // atom<-atom; atom<-rec (group "ar"); rec<-atom (the flipped group)
  // all-atom crop: atom mask = the mask of the atom's residue (atom_res = row 1 of atom_rec_edge_index)
  int *keep_atom = nullptr, *atom_res = nullptr;
  bool ar_arange = false;   // edge k of atom_rec_edge_index belongs to atom k: what the reference's all-atom crop is defined for
  ReduceGroup *rg_aa_all_crop = nullptr, *rg_emb_crop = nullptr;
  int *aa_batch = nullptr, *ar_batch = nullptr;
  float *aa_dist = nullptr, *aa_nvec = nullptr, *aa_ew = nullptr, *atom_edge_base = nullptr;
  float *ar_dist = nullptr, *ar_nvec = nullptr, *ar_edge_base = nullptr, *atom_node_base = nullptr;
  float *atom_node_enc = nullptr, *emb_a = nullptr, *emb_b = nullptr;   // embedding layers: atom encoder rows before them, the two [N] tables they run in
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
  float *s_tr, *s_rot, *s_tor, *s_t = nullptr; long long* s_ids = nullptr; PinnedStage s_ids_stage;   // s_ids [B] and its pinned staging
  bool rec_on = false; ddmi_sample_record rec{};   // ddmi_set_sample_record: caller-owned per-step arrays of the ddmi_sample loop
  float* rp_center = nullptr; PinnedStage rp_stage;   // ddmi_randomize_position: centres [B][3] and their pinned staging
};

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

inline void gemm(const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc, int M, int N, int K,
                 int act, hipStream_t s, const int* m_dev = nullptr, const float* rowbias = nullptr, const int* ridx = nullptr,
                 int ldrb = 0) {
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.act = act;
  g.m_dev = m_dev; g.rowbias = rowbias; g.ridx = ridx; g.ldrb = ldrb;
  launch_gemm(g, s);
}
// one more independent GEMM of a batched launch (a full batch goes out first)
inline GemmArgs& batch_add(GemmBatch& gb, hipStream_t s) {
  if (gb.n == GEMM_BATCH_MAX) { launch_gemm_batch(gb, s); gb.n = 0; }
  return gb.g[gb.n++] = GemmArgs{};
}

inline EdgeMlpArgs mlp_args(const Mlp2W& w, int ns, int E, const int* e_dev, const float* dist, const float* offsets, int D,
                            float coeff, int g_col, const float* gvec, const int* gidx, float* out) {
  EdgeMlpArgs a;
  a.E = E; a.e_dev = e_dev; a.dist = dist; a.offsets = offsets; a.D = D; a.coeff = coeff;
  a.W0g = w.W0 + g_col; a.ldw0g = w.in; a.gvec = gvec; a.gidx = gidx; a.W1 = w.W3; a.b1 = w.b3; a.ns = ns;
  a.out = out; a.ldo = ns;
  return a;
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

// ---- conv_layers.cpp
// One TensorProductConvLayer in the node-contracted form (k_conv.hip).
// pq_mode: 0 = the per-node terms of the first Linear as the size rule says (per group, or batched for small layers), 1 = all of
// them in one launch in front of the groups (first layer of the fused node-update route), 2 = already there (written by the
// previous layer's k_node_update).  Lnext / gnext: the NEXT interaction layer and its groups -- the node update then also
// produces their per-node terms (k_node_update instead of k_reduce_bn).  rg_dev == nullptr: the groups' messages only, the caller
// reduces them (legacy all-atom class: several modules meet in one node update, k_reduce_bn_sum).
void run_conv(Model& m, const ConvW& L, const std::vector<RunGroup>& groups, const ReduceGroup* rg_dev, int n_rg,
              const float* Xin, float* Xout, int nbase, int ncount, hipStream_t s, int pq_mode = 0, const ConvW* Lnext = nullptr,
              const std::vector<RunGroup>* gnext = nullptr);
// The interaction layers of the CG model over [ll ; lig<-rec ; rec-rec ; rec<-lig], from table X[xi] on (joined, overlapped or with
// the fused node update, as the options say); xi ends at the last table
void run_cg_layers(Model& m, const RunGroup& g_ll, const RunGroup& g_lr, const RunGroup& g_rr, const RunGroup& g_rl, bool crop, int& xi,
                   hipStream_t s);
// final_conv / tor_bond_conv: per-edge weights, then the table-driven tensor product.
void run_direct_conv(Model& m, const ConvW& L, const float* attr, int E, float* hid, float* Wt, const int* xrow,
                     const float* X, const float* sh, const float* ew, const int* valid_cnt, int cap, float* out_rows,
                     hipStream_t s);
// mean, scale and bias of a layer's BatchNorm (three null pointers without one)
struct BnArgs { const float *mean, *scale, *bias; };
inline BnArgs bn_args(const ConvW& L) { return L.has_bn ? BnArgs{L.bn_mean, L.bn_scale, L.bn_bias} : BnArgs{nullptr, nullptr, nullptr}; }

}  // namespace ddmi
