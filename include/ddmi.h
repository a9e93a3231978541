/* ddmi.h -- C ABI of the MI355X-native DiffDock score-model sampling path (libddmi.so).
 *
 * The reference (gcorso/DiffDock @ 2024_10_08) is 100 % Python and has no FFI; its
 * boundary for this path is the Python duck type
 *     model = get_model(args, device, t_to_sigma, no_parallel=True)   utils/utils.py:172
 *     tr, rot, tor = model(batch)[:3]                                 utils/sampling.py:116
 *     pos = modify_conformer_batch(pos, batch, tr, rot, tor, mask)    utils/sampling.py:189
 *     data_list, conf = sampling(data_list, model, steps, ...)        utils/sampling.py:69
 * Each entry point below names the reference interface it replaces.  The ctypes binding a
 * maintainer would add is shown in INTEGRATION.md (diffdock_amd/lib.py is that binding).
 *
 * Conventions: all tensor pointers are DEVICE pointers (fp32 / int32 / uint8) unless a
 * parameter is documented as host; they are borrowed for the duration of the call
 * (weights, tables and the static complex description are copied).  Work is enqueued on the
 * caller's HIP stream (pass torch.cuda.current_stream().cuda_stream; NULL = default
 * stream).  Every function returns 0 on success or a negative ddmi_status; the message is
 * available from ddmi_last_error() (thread-local).  A model handle is bound to one device
 * and must not be used from two threads at once; distinct handles are independent.
 */
#ifndef DDMI_H
#define DDMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ddmi_model ddmi_model;
typedef void* ddmi_stream; /* hipStream_t */

enum ddmi_status {
  DDMI_OK = 0,
  DDMI_ERR_ARG = -1,     /* bad argument / inconsistent shapes            */
  DDMI_ERR_STATE = -2,   /* call order (weights / tables / complex unset) */
  DDMI_ERR_HIP = -3,     /* HIP runtime error                             */
  DDMI_ERR_KEY = -4,     /* unknown / missing state_dict key              */
  DDMI_ERR_CAPACITY = -5 /* workspace or neighbour capacity exceeded      */
};

/* Execution options: which of the parity-tested kernel routes a model runs.  Every field 0 = the default a caller should
 * keep; the other values exist for the route-agreement tests (tests/test_gpu_parity.py::test_selectable_kernel_paths_agree_on_the_gpu)
 * and for A/B timing.  Read once at ddmi_create; libddmi.so itself reads NO environment variable -- diffdock_amd/lib.py maps
 * the DDMI_* variables of the test / bench harness onto these fields (INTEGRATION.md has the table). */
typedef struct ddmi_exec_options {
  int32_t streams;          /* 0 = two HIP streams (ligand-gather groups next to residue-gather groups), 1 = one stream            */
  int32_t dense_rows;       /* k_conv_fused dense-row loop: 0 = groups with >= 20 edges per gather node, 1 = never, 2 = always       */
  int32_t shared_tiles;     /* shared-node tiles (4x4x1 contraction): 0 = the rec<-lig group, 1 = never, 2 = every dense group       */
  int32_t packed_granules;  /* 0 = packed granules for output blocks of <= 10 channels, 1 = classic 4-slot granules only             */
  int32_t merged_granule;   /* 0 = the three scalar channel tiles of the first layer as one granule, 1 = separate                    */
  int32_t pre_reduce;       /* 0 = in-tile pre-reduction of the lig<-rec messages, 1 = one message row per edge                      */
  int32_t hidden_mm;        /* 0 = hidden rows straight from the edge attributes (k_edge_hidden_mm), 1 = GEMMs + k_edge_hidden       */
  int32_t fc1_batch;        /* 0 = per-node terms of the first Linear of all groups of a SMALL layer in one launch, 1 = per group    */
  int32_t tile_split;       /* workgroups per 16-virtual-node tile (granule ranges); 0 = automatic                                   */
  int32_t tile_split_small; /* the same for a small group that runs next to chip-filling ones; 0 = automatic                         */
  int32_t hidden_grid;      /* workgroups of k_edge_hidden_mm; 0 = 2048                                                              */
  int32_t tp_apply;         /* read-out tensor product: 0 = by launch size, 1 = wave per pair, 2 = workgroup per edge, 3 = thread    */
  int32_t debug;            /* 1 = print the granule list of every interaction layer to stderr at ddmi_commit_weights, and the route
                             * of every edge group (hidden rows, granule loops) at each forward (tests)                            */
  int32_t tile_per_pose;    /* 1 = the 16-virtual-node tiles of k_conv_fused never span two graphs of the batch (dead virtual nodes
                             * pad every graph to whole tiles): the arithmetic of a pose then does not depend on the poses batched
                             * with it -- a sharded run is BIT-identical to the one-batch run.  0 = dense tiles.     */
  int32_t layer_overlap;    /* interaction layers on the two streams: 0 = joined -- all groups of a layer, then one node update; 1 = node
                             * update split by node type and every group's chain started as soon as the rows it reads exist, for
                             * chip-filling batches; 2 = that for every batch size.  Same kernels and arithmetic (bit-identical scores);
                             * measured neutral at 40 poses and -6 % at 5 (profiles/r05_e11_ab.txt), hence not the default.            */
  int32_t grouped;          /* grouped dispatch of an interaction layer (round 6): per layer ONE launch of the per-node first-Linear terms,
                             * ONE of the hidden rows and ONE k_conv_grouped walking the (edge group, tile, granule range) work items of
                             * every edge group, on one stream -- instead of a hidden-row + k_conv_fused launch per group on two streams.
                             * 0 / 1 = per-group launches (the default: measured 1-2.4 % faster at 5 / 10 / 40 poses because hidden rows overlap
                             * the other stream's convolution, profiles/r06_p2_*), 2 = grouped wherever supported (exact-f32 l <= 1
                             * layers with a two-layer edge MLP; others keep the per-group path).  Bit-identical messages either way.   */
  int32_t grouped_split;    /* workgroups per 16-virtual-node tile in grouped launches (granule ranges), 1..8; 0 = automatic           */
  int32_t vn_build;         /* virtual-node lists + per-edge rows of a layer's edge groups: 0 = two launches for all groups
                             * (k_vn_lists: count -> scan -> fill with a workgroup per group; k_vn_rows_grouped), 1 = a
                             * count -> scan -> fill -> rows chain per group (rounds 2-5)                                              */
  int32_t node_update;      /* 1 (2 / 3: workgroup shape forced to sixteen / four nodes) = k_node_update: the node update of an interaction layer (mean over all groups' messages, BatchNorm,
                             * residual) also produces the NEXT layer's per-node first-Linear terms P / Q from the rows it holds --
                             * no k_gemm_nt_batch launch per layer; 0 = k_reduce_bn + GEMM launches (the default: the fused kernel's
                             * 16-node workgroups stream the message rows at 0.57 instead of 0.40 ms per forward and the GEMMs it
                             * removes ran next to the convolution anyway -- 154.0 against 155.3 poses/s at 40 poses, 107.4 / 108.4
                             * at 5, profiles/r06_p5_*).  CG models with two-layer edge MLPs; node rows bit-identical, P / Q equal up
                             * to the order of an ns-term fp32 sum.                                                                      */
  int32_t tile_split_last;  /* workgroups per tile for the LAST chip-filling k_conv_fused launch of each stream in a layer (its final partial
                             * round of workgroups is the layer's straggler tail); 0 = as tile_split                                   */
  int32_t tile_split_rule;  /* automatic tile_split of a chip-filling group: 0 = cheapest schedule of ceil(tiles x split / CUs) rounds of
                             * (granules per item + prologue) (round 6), 1 = one work item per tile (rounds 2-5),
                             * 2 = as 0, and the same round model for groups of >= 32 tiles in layers where no group fills the chip (A/B) */
  int32_t group_order;      /* issue order of a layer's edge groups on their streams: 0 = [lig-lig, rec<-lig] | [lig<-rec, rec-rec];
                             * bit 0 = side stream reversed, bit 1 = main stream reversed (A/B knob)                                   */
  int32_t list_caps;        /* capacity of the virtual-node lists (= grid size of k_conv_fused): 0 = nodes + edges / 32 (up to 2 x the live
                             * count), 1 = per-node degree bounds (one virtual node per residue of an all-pairs cross graph: half the
                             * workgroups of the lig<-rec and rec-rec launches never exist) -- neutral at 5-20 poses, 1.8 % SLOWER at 40
                             * (153.1 against 155.9 poses/s: the empty workgroups pace the dispatch between the two streams,
                             * profiles/r06_p12_*), hence not the default                                                               */
  int32_t time_terms;       /* 1 = k_time_terms: time embedding, its per-graph linear terms and rec_sigma's second layer in one launch
                             * (measured neutral once the cross-graph search runs beside them: profiles/r06_p18_*), 0 = k_time_embedding
                             * -> k_gemm_nt_batch -> k_gemm_nt (the default)                                                           */
  int32_t rec_share;        /* 0 = when every graph of the batch is a copy of graph 0's receptor (features, positions, contact graph) and
                             * the forward has one t for all graphs (the ddmi_sample step loop; not ddmi_forward, whose t stays on the
                             * device), the first interaction layer computes the rec-rec messages of graph 0 only and the node update
                             * reads them for every graph -- bit-identical, 1/B of that group's work.  CG model, no per-step crop,
                             * joined layers (layer_overlap, grouped = 2 and node_update keep the full group).  1 = never              */
} ddmi_exec_options;

/* Hyper-parameters: the keyword arguments get_model passes to CGModel
 * (utils/utils.py:234-276, models/cg_model.py:20-31) and the sigma bounds t_to_sigma reads
 * (utils/diffusion_utils.py:28-32).  Booleans are 0/1.
 * struct_size MUST be sizeof(ddmi_config) of the header the caller was compiled against: the struct is passed by pointer and
 * grows with the library, so ddmi_create rejects a caller built against another layout instead of reading past its struct. */
typedef struct ddmi_config {
  uint32_t struct_size;
  int32_t ns, nv, num_conv_layers, num_prot_emb_layers, sh_lmax;
  int32_t sigma_embed_dim, distance_embed_dim, cross_distance_embed_dim, in_lig_edge_features;
  int32_t lm_embedding_dim; /* 1280 for 'precomputed' ESM2 features, else 0 */
  float lig_max_radius, rec_max_radius, cross_max_distance, center_max_distance;
  int32_t dynamic_max_cross, use_second_order_repr, reduce_pseudoscalars, differentiate_convolutions;
  int32_t embed_also_ligand, batch_norm, smooth_edges, odd_parity, no_torsion, scale_by_sigma;
  int32_t fixed_center_conv;
  float embedding_scale;
  float tr_sigma_min, tr_sigma_max, rot_sigma_min, rot_sigma_max, tor_sigma_min, tor_sigma_max;
  int32_t all_atoms; /* get_model's model_class switch (utils/utils.py:221-224): 1 = AAModel (models/aa_model.py) */
  /* get_model(..., confidence_mode=True): same interaction layers, confidence_predictor read-out (cg_model.py:181-207,
   * 353-366); the model is evaluated with ddmi_confidence instead of ddmi_forward */
  int32_t confidence_mode, num_confidence_outputs;
  /* get_model(..., old=True) (utils/utils.py:180-219): legacy class models/old_cg_model.py (the released DiffDock-L
   * confidence checkpoint, `old_confidence_model: true`).  Score mode (ddmi_forward, old_cg_model.py:293-352) and confidence
   * mode (ddmi_confidence), OldAtomEncoder, sh_lmax = 2.
   * With all_atoms = 1: AAOldModel (models/old_aa_model.py), the legacy class on all-atom graphs -- the atom arrays of
   * ddmi_complex are required as for AAModel, nine OldTensorProductConvLayers per interaction layer under the state-dict keys
   * conv_layers.{9l + k}, num_confidence_outputs confidence outputs; both modes, ddmi_sample and ddmi_set_crop_cutoff included. */
  int32_t old_model;
  /* confidence-mode options of the new classes (cg_model.py:184-207, aa_model.py:177-211): per-atom predictor in front of the
   * graph mean (`atom_confidence_loss_weight > 0`, atom_num_confidence_outputs = len(atom_rmsd_classification_cutoff) + 1)
   * and one extra affinity output of confidence_predictor (`affinity_prediction`, parallel = 1) */
  int32_t atom_confidence, atom_num_confidence_outputs, affinity_prediction;
  /* get_timestep_embedding (utils/diffusion_utils.py:129-136): 0 = 'sinusoidal' (embedding_scale multiplies t), 1 = 'fourier'
   * (GaussianFourierProjection, :113-127; its frozen parameter W is the state_dict key `timestep_emb_func.W`) */
  int32_t embedding_type;
  /* FCBlock depth of the per-edge weight MLP of the embedding / interaction layers (models/layers.py:10-17,
   * tensor_layers.py:302-304): 2 (or 0) = Linear, ReLU, Linear; n > 2 adds n - 2 hidden Linear + ReLU (keys fc.3 .. fc.3(n-1)) */
  int32_t tp_weights_layers;
  /* CGModel.sidechain_predictor (models/cg_model.py:173-178,397-402; get_model: sidechain_loss_weight > 0 or backbone_loss_weight > 0,
   * utils/utils.py:274-275): an e3nn o3.Linear on the receptor rows of the last node table -> 4x0e + 2x1e + 4x0o + 2x1o, even and
   * odd halves summed -- the 4th element of the forward tuple.  State-dict key `sidechain_predictor.weight`; read with
   * ddmi_sidechain_pred after ddmi_forward.  CG models only (AAModel asserts it away, models/aa_model.py:38). */
  int32_t sidechain_pred;
  /* TensorProductConvLayer(depthwise=True) in the embedding and interaction layers (models/tensor_layers.py:248-290,324-325;
   * cg_model.py:124,147,168): an e3nn 'uvu' TensorProduct (one per-edge weight per path and input channel) followed by the shared
   * o3.Linear `linear_2`.  Both stages are linear in the weights, so at ddmi_commit_weights the pair is folded into the second
   * layer of the per-edge MLP of an equivalent fully connected tensor product (W2'[(path, u, w)] = W2[(path, u)] * linear_2[u, w];
   * the two e3nn normalisations multiply to the fully connected one) and the layer runs the same kernels.  CG models only. */
  int32_t depthwise_convolution;
  /* ---- execution options (not arguments of the reference's get_model; 0 = default).
   * edge_product: arithmetic of the per-edge product T_e = h_e . Y_d in the interaction layers (k_conv_fused):
   *   0 = v_mfma_f32_16x16x4_f32, an exact fp32 fma chain (the headline route);
   *   1 = split-bf16: both operands carried as bf16 hi + bf16 lo (16 significand bits), the four bf16 products of every
   *       f32 product on v_mfma_f32_16x16x32_bf16 with fp32 accumulation -- a quarter of the matrix-core time of route 0;
   *       applies to the static l <= 1 loops (sh_lmax = 1, ns % 16 == 0), other layers run route 0.  Same 1e-4 parity bar,
   *       reported as its own bench line (dtype "bf16x4-split edge product, f32 accumulate").
   * (The library reads no environment variable: the Python harness maps DDMI_EDGE_PRODUCT onto this field, diffdock_amd/lib.py.) */
  int32_t edge_product;
  ddmi_exec_options exec; /* kernel-route selection, all 0 = defaults (see above) */
} ddmi_config;

/* Static description of one collated batch of complexes = the fields of the PyG Batch the
 * path reads.  Node indices inside edge arrays are batch-global, as PyG
 * collation produces them.  lig_ptr / rec_ptr are HOST arrays [num_graphs+1] of cumulative
 * node counts.  The conformer fields describe ONE graph and are required only by
 * ddmi_modify_conformer / ddmi_sample, which (like the reference's modify_conformer_batch,
 * utils/diffusion_utils.py:60-64) assume all graphs in the batch are copies of one complex
 * unless ddmi_set_batch_layout gives every graph its own mask. */
typedef struct ddmi_complex {
  int32_t num_graphs, n_lig, n_rec, n_bond_edges, n_rec_edges, n_tor;
  const int32_t* lig_ptr;        /* host [B+1] */
  const int32_t* rec_ptr;        /* host [B+1] */
  const int32_t* lig_x;          /* [n_lig,16] categorical atom features            */
  const int32_t* bond_index;     /* [2,n_bond_edges] ('ligand','lig_bond','ligand') */
  const float* bond_attr;        /* [n_bond_edges, in_lig_edge_features]            */
  const uint8_t* edge_mask;      /* [n_bond_edges] rotatable directed bonds         */
  const float* rec_x;            /* [n_rec, 1+lm_embedding_dim]                     */
  const float* rec_pos;          /* [n_rec,3]                                       */
  const int32_t* rec_edge_index; /* [2,n_rec_edges] ('receptor','rec_contact','receptor') */
  const uint8_t* mask_rotate;    /* [n_tor/B, n_lig/B] or NULL                      */
  /* all_atoms only (models/aa_model.py:275-362): receptor heavy atoms and their two static relations */
  int32_t n_atom, n_atom_edges, n_atom_rec_edges;
  const int32_t* atom_ptr;            /* host [B+1] */
  const int32_t* atom_x;              /* [n_atom,4] categorical atom features                  */
  const float* atom_pos;              /* [n_atom,3]                                            */
  const int32_t* atom_edge_index;     /* [2,n_atom_edges] ('atom','atom_contact','atom')       */
  const int32_t* atom_rec_edge_index; /* [2,n_atom_rec_edges] ('atom','atom_rec_contact','receptor'): row 0 atoms, row 1 residues */
} ddmi_complex;

/* Reverse-diffusion loop parameters = the arguments of sampling() (utils/sampling.py:69-72).
 * Schedules are HOST arrays [inference_steps].  If z_* are NULL the Gaussian draws come
 * from a counter-based generator keyed by (seed, sample_ids[b], step, component), so a run
 * sharded over ranks reproduces the single-rank trajectories sample by sample. */
typedef struct ddmi_sample_cfg {
  int32_t inference_steps;
  const double* tr_schedule;
  const double* rot_schedule;
  const double* tor_schedule;
  int32_t ode, no_random, no_final_step_noise;
  double temp_sampling[3], temp_psi[3], temp_sigma_data[3];
  uint64_t seed;
  const int64_t* sample_ids; /* host [B] or NULL (= 0..B-1) */
  const float* z_tr;         /* device [steps,B,3] or NULL  */
  const float* z_rot;        /* device [steps,B,3] or NULL  */
  const float* z_tor;        /* device [steps,n_tor] or NULL */
  int32_t use_crop;          /* model_args.crop_beyond is not None (utils/sampling.py:104) */
  double crop_beyond;        /* per-step receptor crop at 3*tr_sigma + crop_beyond (utils/sampling.py:107) */
} ddmi_sample_cfg;

/* get_model(args, device, ...) -- utils/utils.py:172.  device = HIP device ordinal. */
int ddmi_create(const ddmi_config* cfg, int device, ddmi_model** out);
void ddmi_destroy(ddmi_model* m);
const char* ddmi_last_error(void);

/* model.load_state_dict(sd, strict=True) -- inference.py:202-203.  One call per tensor with
 * the reference's state_dict key, HOST fp32 data; then ddmi_commit_weights
 * checks that every expected key was provided, pre-packs and uploads. */
int ddmi_set_weight(ddmi_model* m, const char* key, const float* host_data, const int64_t* shape, int ndim);
int ddmi_commit_weights(ddmi_model* m);
/* Number of state_dict keys the configured architecture expects, and the i-th key / shape. */
int ddmi_num_weights(ddmi_model* m);
int ddmi_weight_spec(ddmi_model* m, int i, const char** key, int64_t shape[4], int* ndim);

/* Score-norm tables the reference builds at import: kind 0 = so3._exp_score_norms
 * (utils/so3.py:59, 2000 entries), kind 1 = torus.score_norm_ (utils/torus.py:72-76, 5001
 * entries).  HOST float64. */
int ddmi_set_table(ddmi_model* m, int kind, const double* host_data, int64_t n);
/* Frequencies of the sinusoidal timestep embedding (utils/diffusion_utils.py:99-104),
 * HOST fp32 [sigma_embed_dim/2]; optional -- computed in-library when not supplied. */
int ddmi_set_time_frequencies(ddmi_model* m, const float* host_freq, int64_t n);

/* batch.to(device) + the receptor-side caching of CGModel.embedding (models/cg_model.py:273-295). */
int ddmi_set_complex(ddmi_model* m, const ddmi_complex* c, ddmi_stream stream);

/* Layout of a batch that packs the poses of SEVERAL complexes for the step loop (not in the reference: there every
 * sampling() batch holds copies of one complex).  Graphs [group_ptr[g], group_ptr[g+1]) form NaN-guard group g -- one
 * sampling() batch of the reference (utils/sampling.py:117-131 runs per batch) -- and graph b's rotatable-bond mask is its
 * own [R_b, Nl_b] block, R_b = the rotatable bonds of graph b (edge_mask), Nl_b = its ligand atoms.  Call after
 * ddmi_set_complex, which resets the handle to one group and graph 0's mask for every graph (a batch of copies).  With a
 * layout set, ddmi_sample, ddmi_perturb and ddmi_modify_conformer accept batches whose graphs differ in atom and torsion
 * counts; a graph's result does not depend on the other graphs.  The mask is copied. */
typedef struct ddmi_batch_layout {
  uint32_t struct_size;       /* sizeof(ddmi_batch_layout) the caller was built against                              */
  int32_t num_groups;         /* NaN-guard groups                                                                   */
  const int32_t* group_ptr;   /* host [num_groups+1] graph offsets, group_ptr[0] = 0, increasing, group_ptr[G] = B  */
  const uint8_t* mask_rotate; /* device: graph b's [R_b, Nl_b] block, graphs in order; NULL if no graph has torsions */
  int64_t mask_rotate_bytes;  /* must equal sum_b R_b * Nl_b                                                        */
} ddmi_batch_layout;
int ddmi_set_batch_layout(ddmi_model* m, const ddmi_batch_layout* l, ddmi_stream stream);

/* tr, rot, tor = model(batch)[:3] -- models/cg_model.py:308-424.
 * lig_pos [n_lig,3]; t_* [B] = batch.complex_t[...]; outputs tr [B,3], rot [B,3], tor [n_tor]. */
int ddmi_forward(ddmi_model* m, const float* lig_pos, const float* t_tr, const float* t_rot, const float* t_tor,
                 float* tr_out, float* rot_out, float* tor_out, ddmi_stream stream);

/* sidechain_pred = model(batch)[3] -- models/cg_model.py:397-402 -- of the LAST ddmi_forward call on this handle:
 * out [n_rec, 10].  Requires ddmi_config.sidechain_pred. */
int ddmi_sidechain_pred(ddmi_model* m, float* out, ddmi_stream stream);

/* confidence, atom_confidence = confidence_model(batch) -- utils/sampling.py:221, models/cg_model.py:353-366 /
 * models/aa_model.py:431-452.  Requires ddmi_config.confidence_mode.  t_* are used raw (sampling() passes 0).
 * conf_out [B, num_confidence_outputs (+ 1 with affinity_prediction)]; atom_conf_out [n_lig, atom_num_confidence_outputs]
 * with ddmi_config.atom_confidence, else NULL (the reference returns zeros there). */
int ddmi_confidence(ddmi_model* m, const float* lig_pos, const float* t_tr, const float* t_rot, const float* t_tor,
                    float* conf_out, float* atom_conf_out, ddmi_stream stream);

/* crop_beyond(graph, cutoff, all_atoms) -- utils/utils.py:388-413 as applied by sampling() before each model call
 * (utils/sampling.py:104-109): subsequent ddmi_forward / ddmi_confidence calls drop the residues farther than `cutoff`
 * from every ligand atom of their graph, with the contact edges touching them.  cutoff <= 0 switches cropping off;
 * ddmi_sample sets its own cutoff per step (ddmi_sample_cfg.use_crop) and restores this one.
 * All-atom models: the atoms of a dropped residue go with it (atom a belongs to residue atom_rec_edge_index[1][a]),
 * atom_contact keeps the edges between kept atoms, the ligand-atom radius graph sees kept atoms only, and embedding layers
 * (num_prot_emb_layers > 0) are re-run on the cropped residue + atom graph in every call, as in the reference.  The reference
 * rewrites atom_rec_contact as arange(kept atoms), which is defined only when column k of atom_rec_edge_index belongs to
 * atom k: n_atom_rec_edges == n_atom and row 0 == 0..n_atom-1 (what the reference's preprocessing writes).  A complex that
 * does not have this form evaluates without a cutoff as always; with a cutoff set, ddmi_forward / ddmi_confidence /
 * ddmi_sample return DDMI_ERR_ARG.
 * Dropped residues and atoms stay rows of the node tables and keep no edges (debug buffers crop_keep [n_rec],
 * crop_keep_atom [n_atom]: 1 = kept).  A graph that keeps no residue is not refused on the device (the reference would
 * fail on its empty receptor): its ligand rows are computed without receptor or atom messages -- CG and all-atom alike. */
int ddmi_set_crop_cutoff(ddmi_model* m, float cutoff);

/* modify_conformer_batch -- utils/diffusion_utils.py:60-78.  pos [n_lig,3] updated in place;
 * tr_update [B,3], rot_update [B,3], tor_update [n_tor] or NULL. */
int ddmi_modify_conformer(ddmi_model* m, float* lig_pos, const float* tr_update, const float* rot_update,
                          const float* tor_update, ddmi_stream stream);

/* The hot loop of sampling() -- utils/sampling.py:96-191 -- for one collated batch, entirely
 * on the device (no host synchronisation: the call returns once the steps are enqueued).  lig_pos [n_lig,3] is updated
 * in place. */
int ddmi_sample(ddmi_model* m, float* lig_pos, const ddmi_sample_cfg* cfg, ddmi_stream stream);

/* Per-step record of the ddmi_sample loop (not in the reference, whose Python loop has every step's tensors in hand: the
 * visualisation hook at utils/sampling.py:193-206 and the NaN warning at :117-124 read them).  The kernels of the step loop that
 * already hold a value store it into row `step` of the caller's arrays as well: no extra launch, no host synchronisation, and
 * with no record set ddmi_sample enqueues exactly what it does without this entry point (final poses are bit-identical either
 * way).  The arrays are CALLER-owned device memory that must stay valid until the enqueued steps have run; every array is
 * optional (NULL = not recorded).  Rows >= inference_steps are not touched.  G = the NaN-guard groups of the batch layout in
 * force at ddmi_sample (1 without ddmi_set_batch_layout); n_tor = 0 for no_torsion models.
 * The record applies to the following ddmi_sample calls on the handle (ddmi_forward, ddmi_perturb and ddmi_modify_conformer
 * record nothing) until it is replaced, switched off with NULL, or cleared by ddmi_set_complex (the shapes change) or by
 * ddmi_set_batch_layout (G changes, and with it the row length of nan_count): set the record AFTER the layout.
 * DDMI_ERR_ARG: struct_size mismatch, capacity_steps < 1 -- and, from ddmi_sample before anything is enqueued,
 * capacity_steps < inference_steps.  DDMI_ERR_STATE: no complex set. */
typedef struct ddmi_sample_record {
  uint32_t struct_size;    /* sizeof(ddmi_sample_record) the caller was built against                                       */
  int32_t capacity_steps;  /* rows available in every non-NULL array; must be >= inference_steps of the ddmi_sample call    */
  float* pos;              /* device [capacity_steps, n_lig, 3]: ligand positions AFTER the update of step k, or NULL       */
  float* tr;               /* device [capacity_steps, B, 3]: tr score of step k after the NaN guard, before the update      */
  float* rot;              /* device [capacity_steps, B, 3]                                                                 */
  float* tor;              /* device [capacity_steps, n_tor]; ignored (may be NULL) when the batch has no torsions          */
  int32_t* nan_count;      /* device [capacity_steps, G]: poses of NaN-guard group g whose mean tr score was NaN at step k  */
} ddmi_sample_record;
int ddmi_set_sample_record(ddmi_model* m, const ddmi_sample_record* r); /* NULL switches recording off */

/* One step of the score -> perturbation arithmetic of sampling() -- utils/sampling.py:117-186 -- on caller-owned score
 * arrays, in place: the NaN guard (:117-131: if any pose's mean translation score is NaN, NaN -> 0.01 * nanmean|x|,
 * +-inf -> +-that value, per score tensor) followed by  g^2 dt (lambda + T psi / 2) * score + g sqrt(dt (1 + psi)) * z
 * with the coefficients of step `step` of cfg's schedules.  tr [B,3], rot [B,3], tor [n_tor] or NULL.  This is what
 * ddmi_sample applies between ddmi_forward and ddmi_modify_conformer. */
int ddmi_perturb(ddmi_model* m, float* tr, float* rot, float* tor, const ddmi_sample_cfg* cfg, int step,
                 ddmi_stream stream);

/* randomize_position -- utils/sampling.py:16-58 (inference.py:239-242) for every graph of the batch, on the device.  lig_pos
 * [n_lig,3] is updated in place, one workgroup per graph: the rotatable bonds in edge order, each rotating the atoms of its
 * mask_rotate row about pos[v] by the axis-angle (pos[u] - pos[v]) / |..| * angle (modify_conformer_torsion_angles,
 * utils/torsion.py:48-72: an angle of exactly 0 is skipped, no re-alignment); then (pos - mean) R^T + center; then, unless
 * no_random, the translation.  Works on a batch of copies of one complex and under ddmi_set_batch_layout; a graph's result
 * depends on nothing but its own inputs and its sample id.  No host synchronisation; the host arrays are consumed before the
 * call returns.
 * Draws the caller does not supply come from the library's Philox4x32-10 block with counter (sample id low word, sample id
 * high word, step, component) and key = seed, at step = -1 (0xffffffff as the unsigned counter word: no loop step has it):
 *   component 0-3    standard normals (w, x, y, z), as ddmi_debug_normal gives them; the normalised quaternion is the rotation
 *                    R = [[1-2(yy+zz), 2(xy-zw), 2(xz+yw)], [2(xy+zw), 1-2(xx+zz), 2(yz-xw)], [2(xz-yw), 2(yz+xw), 1-2(xx+yy)]]
 *   component 4-6    standard normals z of the translation: tr_std * z, or with choose_residue rec_pos[idx] + 0.01 * z
 *   component 7      output word 0 modulo the graph's residue count = idx, the choose_residue residue (within the graph)
 *   component 8 + j  rotatable bond j of the graph: u = ((word 0 >> 8) + 0.5) / 2^24, angle = (2u - 1) pi
 * Sharded runs and the tests rely on this layout.
 * DDMI_ERR_STATE: no complex set; a batch whose graphs differ without a layout; rotatable bonds without mask_rotate.
 * DDMI_ERR_ARG: struct_size mismatch, NULL center. */
typedef struct ddmi_randomize_cfg {
  uint32_t struct_size;       /* sizeof(ddmi_randomize_cfg) the caller was built against                                  */
  int32_t no_torsion, no_random, choose_residue;
  float tr_std;               /* host-computed: std_rec * prop / 1.73, or -prop * tr_sigma_max (utils/sampling.py:52-57) */
  const float* center;        /* HOST [B,3]: center_pocket of each graph                                                  */
  uint64_t seed;
  const int64_t* sample_ids;  /* HOST [B] or NULL (= 0..B-1)                                                              */
  const float* tor_updates;   /* device [n_tor] angles, graphs in order, or NULL                                          */
  const float* rotations;     /* device [B,3,3] row-major or NULL                                                         */
  const float* tr_updates;    /* device [B,3] or NULL: the complete translation, replaces draw and mode                   */
} ddmi_randomize_cfg;
int ddmi_randomize_position(ddmi_model* m, float* lig_pos, const ddmi_randomize_cfg* cfg, ddmi_stream stream);

/* Judging sampled poses on the device -- what evaluate.py:474-505, utils/training.py:282-287 (inference_epoch_fix) and
 * confidence/dataset.py:241 compute on the host from the final poses: the symmetry-corrected RMSD to the known pose(s), the
 * uncorrected RMSD, the centroid distance and the minimum intra-ligand distance, plus the minimum distance to a point set.
 * The handle gives the device, the stream order and the error text only: no complex, weights or tables are needed, so the poses
 * may be final poses [N] as well as a recorded trajectory [steps * N] (ddmi_sample_record.pos).  Two kernels are enqueued and the
 * call returns; there is no host synchronisation (a call larger than any before it on the handle allocates its scratch first).
 * One wave owns the sum of one (pose, reference, permutation) and reduces it in a fixed order, so every value is bit-identical
 * whatever the other poses, references and permutations of the call are; every min is deterministic.
 * m-space: atom j of a pose is pos[p][atom_index[j]] (the kept atoms in order, the reference's filterHs of evaluate.py:414 and
 * :430-431); ref and perm live in m-space.  A row of perm is one graph isomorphism as spyrmsd enumerates them: the pair
 * (idx1, idx2) of spyrmsd/rmsd.py:184-187 is the row perm[idx2[i]] = idx1[i].  Entries of perm and atom_index outside their range
 * are clamped into it.  All arrays are device memory; every output is optional (NULL = not computed).
 * DDMI_ERR_ARG: struct_size mismatch, NULL pos or ref, n_poses / n_atoms / n_kept / n_refs < 1, n_kept > n_atoms, n_kept != n_atoms
 * without atom_index, perm with n_perms < 1, points with n_points < 1.  DDMI_ERR_CAPACITY: n_refs * ceil(n_perms / 64) > 2^30. */
typedef struct ddmi_pose_metrics_cfg {
  uint32_t struct_size;        /* sizeof of this struct the caller was built against                                        */
  int32_t n_poses;             /* P: poses (evaluate.py:430 ligand_pos rows; steps * N for a trajectory)                    */
  int32_t n_atoms;             /* n: atoms of a pose                                                                        */
  int32_t n_kept;              /* m: atoms compared (evaluate.py:414 filterHs.sum()); = n_atoms without atom_index          */
  int32_t n_refs;              /* K: known poses (evaluate.py:416-428 orig_ligand_pos rows)                                 */
  int32_t n_perms;             /* S: rows of perm (len of spyrmsd's isomorphisms, rmsd.py:176); ignored without perm        */
  int32_t n_points;            /* Q: rows of points; ignored without points                                                 */
  const float* pos;            /* [P, n, 3]                                                                                 */
  const float* ref;            /* [K, m, 3]                                                                                 */
  const int32_t* perm;         /* [S, m] or NULL (identity, S = 1)                                                          */
  const int32_t* atom_index;   /* [m] or NULL (0..n-1)                                                                      */
  const float* points;         /* [Q, 3] or NULL: anything to keep clear of (residue or receptor-atom positions)            */
  float* rmsd;                 /* [P]  sqrt(min over (k, s) of sum_j |ref[k, perm[s, j]] - pos[p, atom_index[j]]|^2 / m):
                                       spyrmsd/rmsd.py:179-203 with minimize = center = False, np.min of evaluate.py:484    */
  int32_t* best;               /* [P, 2]  the (k, s) attaining it; ties go to the lowest k * S + s                          */
  float* rmsd_per_ref;         /* [P, K]  the value before the min over k (evaluate.py:483 rmsds, transposed)               */
  float* rmsd_plain;           /* [P]  identity permutation only, min over k: the fallback formula of evaluate.py:481       */
  float* centroid_distance;    /* [P]  evaluate.py:486                                                                      */
  float* min_self_distance;    /* [P]  evaluate.py:503-505 over the kept atoms; +inf for m = 1                              */
  float* min_point_distance;   /* [P]  min over j, q of |pos[p, atom_index[j]] - points[q]|; +inf without points.  The
                                       reference declares min_cross_distances_list (evaluate.py:331) and never fills it     */
} ddmi_pose_metrics_cfg;
int ddmi_pose_metrics(ddmi_model* m, const ddmi_pose_metrics_cfg* cfg, ddmi_stream stream);

/* The minimised symmetric RMSD and the fitting transform -- spyrmsd.rmsd.symmrmsd(..., minimize=True) (spyrmsd/rmsd.py:179-203 with
 * spyrmsd/qcp.py): for every graph isomorphism the RMSD after the optimal rigid superposition (Theobald's QCP), then the min.  It
 * separates "wrong conformer" from "right conformer in the wrong place".  Inputs, m-space, clamping and NULL rules are those of
 * ddmi_pose_metrics_cfg.  For pose p, known pose k and row s of perm, with a_j = pos[p, atom_index[j]], b_j = ref[k, perm[s, j]]:
 *   ca = mean_j a_j, cb = mean_j b_j, Ga = sum_j |a_j - ca|^2, Gb = sum_j |b_j - cb|^2, M = sum_j (a_j - ca)(b_j - cb)^T,
 *   lambda = the largest eigenvalue of the symmetric 4x4 key matrix of M (qcp.py:55-122), e = Ga + Gb - 2 lambda,
 *   rmsd_min = 0 where |e| < 1e-9 (the reference's atol, qcp.py:283), else sqrt(max(e, 0) / m),
 * all in float64 on the float32 inputs (e is a small difference of large numbers); lambda comes from a cyclic Jacobi iteration, not
 * from QCP's Newton iteration, so a degenerate largest eigenvalue needs no fallback.  The min over (k, s) is taken on e rounded to
 * float32, which is the rounding of the float64 min.  Two kernels are enqueued and the call returns; no atomics, no host
 * synchronisation, and every value is bit-identical whatever the other poses, known poses and permutations of the call are.
 * rotation / translation: the proper rotation R (det = +1, QCP never reflects) and t = cb - R ca of the winning (k, s), so that
 * R a_j + t ~ b_j.  m = 1 gives the identity.  Where the largest eigenvalue is degenerate (m = 2, collinear atoms) the optimal
 * rotation is not unique: any maximiser is correct, one of them is returned.
 * The errors are those of ddmi_pose_metrics (without the points rule), named ddmi_pose_fit_cfg. */
typedef struct ddmi_pose_fit_cfg {
  uint32_t struct_size;        /* sizeof of this struct the caller was built against                                        */
  int32_t n_poses;             /* P: poses (steps * N for a trajectory)                                                     */
  int32_t n_atoms;             /* n: atoms of a pose                                                                        */
  int32_t n_kept;              /* m: atoms compared; = n_atoms without atom_index                                           */
  int32_t n_refs;              /* K: known poses                                                                            */
  int32_t n_perms;             /* S: rows of perm; ignored without perm                                                     */
  const float* pos;            /* [P, n, 3]                                                                                 */
  const float* ref;            /* [K, m, 3]                                                                                 */
  const int32_t* perm;         /* [S, m] or NULL (identity, S = 1)                                                          */
  const int32_t* atom_index;   /* [m] or NULL (0..n-1)                                                                      */
  float* rmsd_min;             /* [P]  min over (k, s) of the minimised RMSD: symmrmsd(minimize=True), np.min over k        */
  int32_t* best_min;           /* [P, 2]  the (k, s) attaining it; ties go to the lowest k * S + s                          */
  float* rmsd_min_per_ref;     /* [P, K]  the value before the min over k                                                   */
  float* rotation;             /* [P, 3, 3] row-major R of the winning (k, s)                                               */
  float* translation;          /* [P, 3]  t = cb - R ca                                                                     */
} ddmi_pose_fit_cfg;
int ddmi_pose_fit(ddmi_model* m, const ddmi_pose_fit_cfg* cfg, ddmi_stream stream);

/* Capped neighbour lists of a ragged batch of point sets -- the loop of new_extract_receptor_structure
 * (datasets/process_mols.py:171-192 residues, :207-228 atoms) without its dense torch.cdist matrix.  Set g owns the rows
 * ptr[g] .. ptr[g + 1] of pos.  For node i of set g, with c = cutoff and cap = max_neighbors of that set (0 = 1000, the reference's
 * default):
 *   candidates      the other nodes j != i of the set with d(i, j) < c (strict);
 *   <= cap of them  all are kept, in ascending j;
 *   > cap of them   the cap nearest are kept, in ascending distance;
 *   none            the single nearest other node; a set of one node gets no edge.
 * Rules of this library (DESIGN.md "Neighbour graphs"): the node itself is excluded by INDEX (the reference drops the first of an
 * argsort over noisy distances, which is sometimes a real neighbour); another node at distance 0 is an ordinary neighbour; ties in
 * distance go to the lower index (the selection key is float bits of d^2 << 32 | j); d^2 = dx dx + dy dy + dz dz in float32 from direct
 * differences of the float32 coordinates, every operation rounded on its own, compared with the float32 product c c.  One wave owns a
 * node and no atomic decides an order, so the row of node i is bit-identical whatever the other sets, G and the grid are.
 * Outputs (device, each optional): deg [N]; offsets [N + 1] (exclusive scan of deg); n_edges = offsets[N]; edge_index [2, capacity]
 * int64 = [neighbour; centre] with GLOBAL row numbers, ordered by centre -- the reference's [dst_list, src_list] -- row 1 starting at
 * element `capacity`.  Only the first n_edges columns are written.  edge_index = NULL counts only.
 * The handle gives the device, the stream order and the error text; scratch belongs to the handle and only grows.  Three kernels are
 * enqueued and the call returns: no host synchronisation (the HOST arrays ptr / set_cutoff / set_max_neighbors are consumed before it
 * returns).  When every set is capped, E <= sum_g n_g min(cap_g, n_g - 1) is known in advance and `capacity` must cover it.  With an
 * uncapped set (max_neighbors 0) any capacity is accepted: columns past it are dropped and n_edges still holds the full total, so the
 * caller may count first (edge_index = NULL), read n_edges once and call again.
 * DDMI_ERR_ARG: struct_size mismatch, NULL pos or ptr, n_nodes < 1, n_sets < 1, ptr[0] != 0, ptr[n_sets] != n_nodes or a decreasing
 * ptr, a cutoff <= 0 or NaN, max_neighbors < 0, capacity < 0 or too small for a capped call.  DDMI_ERR_CAPACITY: the edge bound of
 * the call reaches 2^31. */
typedef struct ddmi_neighbor_graph_cfg {
  uint32_t struct_size;              /* sizeof(ddmi_neighbor_graph_cfg) the caller was built against                        */
  int32_t n_nodes;                   /* N: rows of pos                                                                      */
  int32_t n_sets;                    /* G                                                                                   */
  int32_t max_neighbors;             /* cap of every set without set_max_neighbors; 0 = 1000                                */
  float cutoff;                      /* cutoff of every set without set_cutoff                                              */
  int64_t capacity;                  /* columns of edge_index                                                               */
  const float* pos;                  /* device [N, 3]                                                                       */
  const int32_t* ptr;                /* HOST [G + 1]                                                                        */
  const float* set_cutoff;           /* HOST [G] or NULL: one cutoff per set                                                */
  const int32_t* set_max_neighbors;  /* HOST [G] or NULL: one cap per set                                                   */
  int32_t* deg;                      /* device [N] or NULL                                                                  */
  int32_t* offsets;                  /* device [N + 1] or NULL                                                              */
  int64_t* edge_index;               /* device [2, capacity] or NULL                                                        */
  int32_t* n_edges;                  /* device [1] or NULL                                                                  */
} ddmi_neighbor_graph_cfg;
int ddmi_neighbor_graph(ddmi_model* m, const ddmi_neighbor_graph_cfg* cfg, ddmi_stream stream);

/* Conformer matching -- datasets/conformer_matching.py (optimize_rotatable_bonds), run in front of every evaluation and training set
 * by get_lig_graph_with_matching (datasets/process_mols.py:323-384): search the torsion angles of a generated conformer for the
 * conformer closest to the known pose.  A ragged batch of J independent jobs (one ligand, one start conformer, one known pose each);
 * job j owns atoms lig_ptr[j] .. lig_ptr[j + 1] and rotatable bonds tor_ptr[j] .. tor_ptr[j + 1].
 * Objective: E(theta) = the minimised RMSD between torsions(start, theta) and target.  torsions is the loop of ddmi_randomize_position
 * (bonds in edge order, float32, an angle of exactly 0 skipped, no re-alignment); the RMSD is the formula of ddmi_pose_fit with the
 * identity permutation, in float64 on the float32 coordinates, with its atol rule.  The reference's SetDihedralRad sets absolute
 * dihedrals; the angles here are RELATIVE to the start conformer -- both cover a full period per bond, so the same conformers are
 * reachable.  AlignMol's identity atom map and proper rotation hold here as well.
 * Optimiser: differential evolution as scipy runs it for the reference (best1bin, mutation (0.5, 1) dithered per generation,
 * recombination 0.8, P = max(5, popsize * R, n_init) members, re-draw of a component that leaves [-pi, pi], stop when
 * std(E) <= tol * |mean(E)|; tol = 0 never stops early), with three deliberate differences: updating is generation-synchronous
 * (scipy's updating='deferred': every trial is built from the previous generation), row 0 of the initial population is all zeros when
 * the caller gives no rows (the result is never worse than the unmatched conformer), and there is no L-BFGS-B polish.
 * Draws: the library's Philox4x32-10 block with key = seed and counter (job id low word, job id high word, generation, c3):
 *   generation 0xffffffff (no generation has it), c3 = i << 6 | (j >> 2), word j & 3   angle j of member i of the initial population:
 *                                                         u = ((word >> 8) + 0.5) / 2^24, angle = (2u - 1) pi, as ddmi_randomize_position
 *   generation g = 1 .. maxiter, c3 = 0xffffffff, word 0          F = 0.5 + 0.5 (word >> 8) / 2^24
 *   generation g, c3 = i << 6                                      trial i: r1 = word 0 mod (P - 1), stepped over i; r2 = word 1 mod (P - 2),
 *                                                                  stepped over the lower, then the higher of (i, r1); jrand = word 2 mod R
 *   generation g, c3 = i << 6 | (1 + (j >> 2)), word j & 3         u_j = ((word >> 8) + 0.5) / 2^24: component j crosses where u_j < 0.8
 *   generation g, c3 = i << 6 | (17 + (j >> 2)), word j & 3        the re-draw of a component outside the box, the angle formula above
 * One kernel launch per call runs every generation: one workgroup per job, one wave per evaluation, no atomics, no host synchronisation
 * (the HOST arrays are consumed before the call returns); a job's result depends on its inputs, its job id and the seed alone.
 * Scratch belongs to the handle and only grows; the handle gives the device, the stream order and the error text.
 * Precondition: the rows of init_angles lie in [-pi, pi].  They enter the population as given (init_energy is E of exactly these rows)
 * and are neither clamped nor wrapped: a row outside the box may win and is then returned in `angles` outside the box.
 * Edge behaviour: a job with no rotatable bond is legal (rmsd = the plain fit of start on target, pos = the moved start, no
 * generations); maxiter = 0 returns the best of the initial population.  rot_u / rot_v outside a job are clamped into it.
 * DDMI_ERR_ARG: struct_size mismatch; NULL start / target / lig_ptr / tor_ptr; n_jobs < 1; a decreasing ptr or ptr[0] != 0; a job of 0
 * atoms; rotatable bonds without rot_u / rot_v / mask_rotate; popsize < 1; maxiter < 0; tol < 0 or NaN; n_init < 0 or n_init > 0 without
 * init_angles (a batch without any rotatable bond has no angles and needs none).  DDMI_ERR_CAPACITY: a job of more than 256 atoms or 64 rotatable bonds, a population above 2^20 members. */
typedef struct ddmi_match_cfg {
  uint32_t struct_size;        /* sizeof(ddmi_match_cfg) the caller was built against                                            */
  int32_t n_jobs;              /* J                                                                                              */
  int32_t popsize;             /* evaluate.py: 40, confidence/dataset.py and training: 20, the reference function's default: 15 */
  int32_t maxiter;             /* generations; 40 / 20 / 500 as above                                                            */
  int32_t n_init;              /* rows of init_angles per job; 0 without                                                         */
  float tol;                   /* scipy's default 0.01                                                                           */
  uint64_t seed;
  const int32_t* lig_ptr;      /* HOST [J + 1]                                                                                   */
  const int32_t* tor_ptr;      /* HOST [J + 1]                                                                                   */
  const int64_t* mask_off;     /* HOST [J]: byte offset of job j's [R_j, n_j] block in mask_rotate, or NULL (blocks in job order) */
  const int64_t* job_ids;      /* HOST [J] or NULL (= 0..J-1): the job's word of the draw counter                                */
  const float* start;          /* device [sum n, 3]                                                                              */
  const float* target;         /* device [sum n, 3]                                                                              */
  const int32_t* rot_u;        /* device [sum R]: job-local atom indices of the bond (u, v); the mask row turns about v          */
  const int32_t* rot_v;        /* device [sum R]                                                                                 */
  const uint8_t* mask_rotate;  /* device bytes: every job's [R_j, n_j] block                                                     */
  const float* init_angles;    /* device: job j's [n_init, R_j] block at n_init * tor_ptr[j], the first rows of its population    */
  float* angles;               /* device [sum R]: the best member                                                                */
  float* rmsd;                 /* device [J]: E of the best member                                                               */
  float* pos;                  /* device [sum n, 3]: torsions(start, angles) moved onto target by the rotation and translation
                                  of its fit -- what AlignMolConformers leaves in mol_rdkit (process_mols.py:356-360)            */
  float* init_energy;          /* device [J, n_init]: E of the caller's rows, as evaluated                                       */
  float* best_history;         /* device [J, maxiter + 1]: the best E after the initial population and after every generation;
                                  the final value is repeated after an early stop                                               */
  int32_t* n_generations;      /* device [J]: generations run                                                                    */
} ddmi_match_cfg;
int ddmi_match_conformer(ddmi_model* m, const ddmi_match_cfg* cfg, ddmi_stream stream);

/* Introspection for tests and profiling: copy a named internal buffer to the host.
 * ddmi_debug_shape returns the element count and up to 4 dims; names are listed in DESIGN.md. */
int ddmi_debug_shape(ddmi_model* m, const char* name, int64_t shape[4], int* ndim, int* is_int);
int ddmi_debug_read(ddmi_model* m, const char* name, void* host_dst, size_t bytes, ddmi_stream stream);
/* Real-basis Wigner-3j tensor used for weight pre-packing (host double [(2l1+1)(2l2+1)(2l3+1)]). */
int ddmi_wigner_3j(int l1, int l2, int l3, double* host_out);
/* The in-library noise generator of ddmi_sample / ddmi_perturb (noise pointers NULL), exposed for tests: the DEVICE code's
 * Philox4x32-10 block for `n` (counter[4], key[2]) pairs (host arrays in, host uint32 [n][4] out; Random123 known-answer
 * vectors), and the standard-normal draws of samples [sample0, sample0 + n_samples) x components [0, n_comp) at one step, as
 * ddmi_perturb keys them (seed, sample id, step, component) -> device float [n_samples][n_comp].
 * Replaces torch.normal at utils/sampling.py:140-154 when the caller supplies no draws. */
int ddmi_debug_philox(const uint32_t* counters, const uint32_t* keys, int n, uint32_t* host_out);
int ddmi_debug_normal(uint64_t seed, int64_t sample0, int n_samples, int step, int n_comp, float* dev_out, ddmi_stream stream);
/* The node update of the legacy all-atom class (k_reduce_bn_sum), exposed for tests.  All pointers are device pointers, node tables
 * and message rows have the library's row stride of 160 floats:
 *   x_out[i] = pad(x_in[i][:d_in]) + sum over g < n_groups of BN_g(mean of msg rows [toff[g][i], toff[g][i + 1])),  i < n_nodes,
 * toff int32 [n_groups][n_nodes + 1], bn_mean / bn_scale / bn_bias float [n_groups][d_out] (v -> (v - mean) * scale + bias).
 * ref_out (optional, n_groups == 1): the same rows from the joint node update of the other classes (k_reduce_bn with the residual),
 * which one group through this kernel equals bit for bit. */
int ddmi_debug_reduce_bn_sum(int n_groups, int n_nodes, int d_in, int d_out, const int32_t* toff, const float* msg, const float* bn_mean,
                             const float* bn_scale, const float* bn_bias, const float* x_in, float* x_out, float* ref_out,
                             ddmi_stream stream);
/* Name / duration table of the kernels launched by the last ddmi_forward when timing is on.  enabled: 0 = off, 1 = one row per
 * kernel name, 2 = k_conv_fused split per edge group, 3 = per (layer, edge group). */
int ddmi_set_kernel_timing(ddmi_model* m, int enabled);
int ddmi_kernel_timings(ddmi_model* m, int i, const char** name, double* ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* DDMI_H */
