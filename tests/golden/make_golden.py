"""Generate tests/golden/*.pt by EXECUTING the reference's own python.

Run in THIS container from the repo root (the reference is absent on the GPU box):
    python tests/golden/make_golden.py

The reference (gcorso/DiffDock @ /root/reference) cannot be imported as is: its
third-party deps e3nn / torch_scatter / torch_cluster / torch_geometric / rdkit / esm /
prody / Bio are not installed.  This script registers stand-ins for exactly those
third-party modules (e3nn + torch_cluster + torch_scatter -> oracle/e3nn_lite.py and
oracle/graph_ops.py, i.e. the restated third-party arithmetic; torch_geometric ->
diffdock_amd/hetero.py containers; rdkit/esm/prody/Bio -> MagicMock, never called) and
then runs the reference's OWN files unmodified:

    models/cg_model.py, models/tensor_layers.py, models/layers.py, utils/utils.py
    (get_model), utils/diffusion_utils.py, utils/torsion.py, utils/geometry.py,
    utils/sampling.py, utils/so3.py, utils/torus.py

One reference defect is patched: FasterTensorProduct has `out_irreps` but
tp_scatter_multigroup reads `tp.irreps_out` (models/tensor_layers.py:194), so
sh_lmax=1 + differentiate_convolutions crashes in the reference; an alias property is
added so that combination can be pinned too.

Fixtures hold inputs, weights, injected noise and the reference outputs, so the parity
tests need neither /root/reference nor this script.
"""
import argparse
import copy
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"


def install_stubs():
    from oracle import e3nn_lite, graph_ops
    from diffdock_amd import hetero

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    o3 = mod("e3nn.o3", Irreps=e3nn_lite.Irreps, Irrep=e3nn_lite.Irrep,
             spherical_harmonics=e3nn_lite.spherical_harmonics,
             FullyConnectedTensorProduct=e3nn_lite.FullyConnectedTensorProduct,
             FullTensorProduct=e3nn_lite.FullTensorProduct,
             TensorProduct=e3nn_lite.TensorProduct, Linear=e3nn_lite.Linear, wigner_3j=e3nn_lite.wigner_3j)
    enn = mod("e3nn.nn", BatchNorm=e3nn_lite.BatchNorm)
    mod("e3nn", o3=o3, nn=enn)
    mod("torch_scatter", scatter=graph_ops.scatter, scatter_mean=graph_ops.scatter_mean)
    mod("torch_cluster", radius=graph_ops.radius, radius_graph=graph_ops.radius_graph, knn_graph=MagicMock())

    def subgraph(subset, edge_index, relabel_nodes=False, **kw):
        keep = subset[edge_index[0]] & subset[edge_index[1]]
        ei = edge_index[:, keep]
        if relabel_nodes:
            remap = torch.cumsum(subset.long(), 0) - 1
            ei = remap[ei]
        return ei, None

    tg = mod("torch_geometric")
    tg.data = mod("torch_geometric.data", Batch=hetero.HeteroBatch, Data=MagicMock(), HeteroData=hetero.HeteroData,
                  Dataset=object)
    tg.loader = mod("torch_geometric.loader", DataLoader=hetero.DataLoader, DataListLoader=MagicMock())
    tg.utils = mod("torch_geometric.utils", subgraph=subgraph, degree=MagicMock(), to_networkx=MagicMock())
    tg.nn = mod("torch_geometric.nn")
    tg.nn.data_parallel = mod("torch_geometric.nn.data_parallel", DataParallel=MagicMock())
    for name in ["rdkit", "rdkit.Chem", "rdkit.Chem.rdchem", "rdkit.Geometry", "rdkit.Chem.AllChem",
                 "rdkit.Chem.rdMolTransforms", "rdkit.RDLogger", "esm", "esm.pretrained", "prody", "Bio", "Bio.PDB",
                 "spyrmsd"]:
        sys.modules[name] = MagicMock()
    sys.path.insert(0, REF)


def build_case(cfg, n_res, n_lig, n_samples, seed, t):
    from diffdock_amd.synth import make_complex, make_pose_list
    from diffdock_amd.weights import init_state_dict
    g = make_complex(seed=seed, n_res=n_res, n_lig=n_lig, all_atoms=cfg.all_atoms, atoms_per_res=(3, 7),
                     lm_dim=cfg.lm_embedding_dim)
    # all-atom cases start inside the pocket: the ligand<-atom group (5 A radius) must not be empty, FasterTensorProduct
    # cannot reshape an empty edge group (reference defect, see header)
    data_list = make_pose_list(g, n_samples, tr_sigma_max=cfg.tr_sigma_max, seed=seed + 100,
                               **(dict(initial_noise_std_proportion=0.05) if cfg.all_atoms else {}))
    sd = init_state_dict(cfg, seed=1234 + seed)
    return g, data_list, sd


def set_times_per_graph(batch, times, all_atoms):
    """utils/diffusion_utils.py:146-168 with one time per graph and noise type: complex_t[k] = times[k] ([B]) and
    node_t[k] = complex_t[k][node batch] for every node type."""
    ct = {k: torch.tensor(times[k], dtype=torch.float32) for k in ("tr", "rot", "tor")}
    for nt in ("ligand", "receptor") + (("atom",) if all_atoms else ()):
        batch[nt].node_t = {k: v[batch[nt].batch] for k, v in ct.items()}
    batch.complex_t = ct


def graph_to_dict(g):
    extra = {}
    if "atom" in g.node_types:   # all-atom graphs
        extra = {"atom_x": g["atom"].x, "atom_pos": g["atom"].pos, "atom_edge_index": g["atom", "atom"].edge_index,
                 "atom_rec_edge_index": g["atom", "receptor"].edge_index}
    return {**extra, "rec_x": g["receptor"].x, "rec_pos": g["receptor"].pos,
            "rec_edge_index": g["receptor", "receptor"].edge_index,
            "lig_x": g["ligand"].x, "lig_pos": g["ligand"].pos, "edge_mask": g["ligand"].edge_mask,
            "mask_rotate": torch.from_numpy(np.asarray(g["ligand"].mask_rotate[0])),
            "bond_index": g["ligand", "ligand"].edge_index, "bond_attr": g["ligand", "ligand"].edge_attr}


def main():
    scratch = os.path.join(ROOT, ".scratch", "tables")
    os.makedirs(scratch, exist_ok=True)
    os.chdir(scratch)           # utils/so3.py, utils/torus.py cache .npy in the CWD
    install_stubs()
    np.random.seed(0)           # utils/torus.py:72-76 Monte-Carlo at import
    from utils import so3, torus
    # the committed table fixtures must be the ones the reference modules hold right now
    assert np.array_equal(np.load(os.path.join(HERE, "so3_exp_score_norms.npy")), so3._exp_score_norms, equal_nan=True)
    assert np.array_equal(np.load(os.path.join(HERE, "torus_score_norm.npy")), torus.score_norm_)

    from functools import partial
    from models import tensor_layers
    tensor_layers.FasterTensorProduct.irreps_out = property(lambda self: self.out_irreps)  # reference defect, see header
    from utils.utils import get_model, crop_beyond
    from utils.diffusion_utils import t_to_sigma as t_to_sigma_compl, get_t_schedule, set_time
    from utils import sampling as ref_sampling
    from diffdock_amd.config import TINY
    from diffdock_amd.hetero import HeteroBatch
    from diffdock_amd.weights import state_dict_spec

    cases = {
        "tiny_l1": dict(cfg=TINY, n_res=40, n_lig=12, n_samples=3, seed=0, t=0.7),
        "tiny_l2": dict(cfg=TINY.replace(sh_lmax=2, tr_sigma_max=19.0), n_res=36, n_lig=14, n_samples=2, seed=1, t=0.35),
        "tiny_l1_1group_emb": dict(cfg=TINY.replace(differentiate_convolutions=False, num_prot_emb_layers=2,
                                                      num_conv_layers=3, smooth_edges=True),
                                   n_res=30, n_lig=10, n_samples=2, seed=2, t=0.9),
        "tiny_l2_fixedcenter": dict(cfg=TINY.replace(sh_lmax=2, fixed_center_conv=True, dynamic_max_cross=False,
                                                      cross_max_distance=30.0, reduce_pseudoscalars=True),
                                    n_res=32, n_lig=11, n_samples=2, seed=3, t=0.5),
        # per-step receptor cropping (utils/sampling.py:104-109): cutoff 3*sigma_tr + 6 A shrinks from 21 A to 7 A
        "tiny_l2_crop": dict(cfg=TINY.replace(sh_lmax=2, crop_beyond=6.0), n_res=44, n_lig=12, n_samples=3, seed=4, t=0.3),
        # all-atom score model (models/aa_model.py): receptor heavy atoms as a third node type, 9 edge groups per layer
        "tiny_aa_l1": dict(cfg=TINY.replace(all_atoms=True, num_conv_layers=3, lig_max_radius=10.0, tr_sigma_max=2.0),
                           n_res=24, n_lig=10, n_samples=2, seed=5, t=0.6),
        "tiny_aa_l2": dict(cfg=TINY.replace(all_atoms=True, num_conv_layers=4, sh_lmax=2, fixed_center_conv=True),
                           n_res=20, n_lig=9, n_samples=2, seed=6, t=0.4),
        # ... with embedding layers over the residue + atom graph (aa_model.py:296-318) and over the ligand graph
        "tiny_aa_l2_emb": dict(cfg=TINY.replace(all_atoms=True, num_conv_layers=2, num_prot_emb_layers=2, sh_lmax=2),
                               n_res=18, n_lig=9, n_samples=2, seed=7, t=0.5),
    }
    # confidence models (get_model(..., confidence_mode=True)): evaluated at t = 0 by sampling() (utils/sampling.py:220)
    cases["tiny_conf_l2"] = dict(cfg=TINY.replace(confidence_mode=True, sh_lmax=2, num_confidence_outputs=3), n_res=30, n_lig=11,
                                 n_samples=3, seed=8, t=0.0)
    cases["tiny_conf_aa_l1"] = dict(cfg=TINY.replace(confidence_mode=True, all_atoms=True, num_conv_layers=3, lig_max_radius=10.0), n_res=20, n_lig=9, n_samples=2, seed=9, t=0.25)
    # the legacy class the released DiffDock-L confidence checkpoint uses (get_model(old=True), models/old_cg_model.py)
    cases["tiny_oldconf"] = dict(cfg=TINY.replace(old=True, confidence_mode=True, sh_lmax=2, num_conv_layers=3), n_res=28, n_lig=10,
                                 n_samples=3, seed=10, t=0.0)
    cases["tiny_oldconf_2l"] = dict(cfg=TINY.replace(old=True, confidence_mode=True, sh_lmax=2, num_conv_layers=2,
                                                      lm_embedding_type=None, dynamic_max_cross=False, cross_max_distance=25.0),
                                    n_res=22, n_lig=9, n_samples=2, seed=11, t=0.3)
    # receptor identities switched off (no_aminoacid_identities: rec.x * 0 at the top of forward; needs no language model)
    cases["tiny_noaa"] = dict(cfg=TINY.replace(no_aminoacid_identities=True, lm_embedding_type=None, sh_lmax=1), n_res=22, n_lig=9,
                              n_samples=2, seed=14, t=0.5)
    # per-atom confidence predictor + affinity output (atom_confidence_loss_weight > 0, affinity_prediction; cg_model.py:184-207)
    cases["tiny_conf_atom"] = dict(cfg=TINY.replace(confidence_mode=True, sh_lmax=2, num_conv_layers=3, atom_confidence=True,
                                                     atom_num_confidence_outputs=2, affinity_prediction=True,
                                                     num_confidence_outputs=2), n_res=24, n_lig=9, n_samples=3, seed=13, t=0.0)
    # the same legacy class in score mode (get_model(old=True, confidence_mode=False)): read-outs old_cg_model.py:293-352
    cases["tiny_oldscore"] = dict(cfg=TINY.replace(old=True, confidence_mode=False, sh_lmax=2, num_conv_layers=3), n_res=26, n_lig=10,
                                  n_samples=3, seed=12, t=0.45)
    # second-order node features (use_second_order_repr: 2e / 2o blocks, models/tensor_layers.py:17-24), CGModel and AAModel
    cases["tiny_2nd"] = dict(cfg=TINY.replace(use_second_order_repr=True, sh_lmax=2, num_conv_layers=4), n_res=26, n_lig=10,
                             n_samples=2, seed=15, t=0.55)
    cases["tiny_aa_2nd"] = dict(cfg=TINY.replace(all_atoms=True, use_second_order_repr=True, sh_lmax=2, num_conv_layers=3,
                                                  reduce_pseudoscalars=True), n_res=16, n_lig=9, n_samples=2, seed=17, t=0.45)
    # get_timestep_embedding('fourier') (GaussianFourierProjection, utils/diffusion_utils.py:113-136): the frozen W is a state_dict key
    cases["tiny_fourier"] = dict(cfg=TINY.replace(embedding_type="fourier", sh_lmax=2), n_res=24, n_lig=10, n_samples=2, seed=18, t=0.65)
    # FCBlock with a hidden Linear layer (tp_weights_layers = 3, models/layers.py:10-17) in embedding and interaction layers
    cases["tiny_tpw3"] = dict(cfg=TINY.replace(tp_weights_layers=3, num_prot_emb_layers=1, num_conv_layers=3), n_res=22, n_lig=10,
                              n_samples=2, seed=19, t=0.5)
    # AAModel with receptor embedding layers and embed_also_ligand=False: ligand rows zero-padded (models/aa_model.py:351-357)
    cases["tiny_aa_emb_nolig"] = dict(cfg=TINY.replace(all_atoms=True, num_conv_layers=2, num_prot_emb_layers=2, sh_lmax=2,
                                                        embed_also_ligand=False), n_res=17, n_lig=9, n_samples=2, seed=20, t=0.5)
    # flags get_model passes through that had no reference-executed evidence until round 4 (third session): odd_parity (one 1o + 1e
    # read-out pair, ns x 0o torsion features: cg_model.py:223,244,251,377-378), batch_norm off and scale_by_sigma off (:393,421)
    cases["tiny_oddpar"] = dict(cfg=TINY.replace(odd_parity=True, sh_lmax=2, num_conv_layers=3), n_res=24, n_lig=11, n_samples=2, seed=21, t=0.45)
    cases["tiny_aa_oddpar"] = dict(cfg=TINY.replace(all_atoms=True, odd_parity=True, num_conv_layers=3, sh_lmax=2, fixed_center_conv=True),
                                   n_res=14, n_lig=9, n_samples=2, seed=22, t=0.3)
    cases["tiny_nobn_noscale"] = dict(cfg=TINY.replace(batch_norm=False, scale_by_sigma=False, num_conv_layers=3), n_res=26, n_lig=13,
                                      n_samples=2, seed=25, t=0.55)
    # round 5: sidechain_pred (sidechain_loss_weight > 0: an o3.Linear on the receptor rows of the last node table, the 4th element
    # of the forward tuple, models/cg_model.py:173-178,397-402).  o3.Linear itself is the oracle's restatement (oracle/e3nn_lite.py)
    cases["tiny_sidechain"] = dict(cfg=TINY.replace(sidechain_pred=True, num_conv_layers=3), n_res=23, n_lig=10, n_samples=2, seed=27, t=0.5)
    # depthwise_convolution (models/tensor_layers.py:248-290,324-325): 'uvu' TensorProduct + linear_2 in the embedding and interaction
    # layers; TensorProduct / Linear are the oracle's restatements of the e3nn classes (oracle/e3nn_lite.py)
    cases["tiny_depthwise"] = dict(cfg=TINY.replace(depthwise_convolution=True, num_conv_layers=3, num_prot_emb_layers=1), n_res=22, n_lig=10,
                                   n_samples=2, seed=28, t=0.5)
    cases["tiny_depthwise_l2"] = dict(cfg=TINY.replace(depthwise_convolution=True, sh_lmax=2, num_conv_layers=4), n_res=20, n_lig=9,
                                      n_samples=2, seed=29, t=0.4)
    # per-graph, per-noise-type times (complex_t[k][b], node_t[k] = complex_t[k][node batch]): B = 3 poses, all three times
    # different in every pose, so a time-dependent quantity read for the wrong graph or the wrong noise type changes the output.
    # The trajectory of each case runs three different decreasing schedules: tr linear, rot = tr ** 1.5, tor = sqrt(tr).
    mixt = {"tr": [0.95, 0.4, 0.05], "rot": [0.3, 0.85, 0.6], "tor": [0.55, 0.1, 0.9]}
    cases["tiny_l1_mixt"] = dict(cfg=TINY, n_res=40, n_lig=12, n_samples=3, seed=40, t=mixt)   # dynamic_max_cross: per-graph cutoff
    cases["tiny_l2_mixt"] = dict(cfg=TINY.replace(sh_lmax=2, tr_sigma_max=19.0), n_res=36, n_lig=14, n_samples=3, seed=41, t=mixt)
    cases["tiny_aa_l1_mixt"] = dict(cfg=TINY.replace(all_atoms=True, num_conv_layers=3, lig_max_radius=10.0, tr_sigma_max=2.0),
                                    n_res=24, n_lig=10, n_samples=3, seed=42, t=mixt)
    cases["tiny_oldscore_mixt"] = dict(cfg=TINY.replace(old=True, confidence_mode=False, sh_lmax=2, num_conv_layers=3), n_res=26,
                                       n_lig=10, n_samples=3, seed=43, t=mixt)   # legacy class: reads rec.node_t['tr']
    if len(sys.argv) > 1:
        cases = {k: v for k, v in cases.items() if k in sys.argv[1:]}
    for name, c in cases.items():
        print("case", name, flush=True)
        cfg = c["cfg"]
        args = cfg.to_namespace()
        if cfg.fixed_center_conv:
            args.not_fixed_center_conv = False
        t_to_sigma = partial(t_to_sigma_compl, args=args)
        model = get_model(args, torch.device("cpu"), t_to_sigma=t_to_sigma, no_parallel=True,
                          confidence_mode=cfg.confidence_mode, old=cfg.old)
        g, data_list, sd = build_case(cfg, c["n_res"], c["n_lig"], c["n_samples"], c["seed"], c["t"])
        ref_keys = {k for k in model.state_dict().keys() if not k.endswith("num_batches_tracked")}   # BatchNorm1d step counter
        assert ref_keys == set(state_dict_spec(cfg).keys()), (sorted(ref_keys ^ set(state_dict_spec(cfg).keys())))
        model.load_state_dict(sd, strict=False)   # strict=False only for the num_batches_tracked counters filtered above
        model.eval()

        # ---- single forward at time t, with per-layer node tables via hooks
        batch = HeteroBatch.from_data_list(copy.deepcopy(data_list))
        B = batch.num_graphs
        if isinstance(c["t"], dict):
            set_times_per_graph(batch, c["t"], cfg.all_atoms)
        else:
            set_time(batch, None, c["t"], c["t"], c["t"], B, cfg.all_atoms, torch.device("cpu"))
        layer_out = []
        hooks = [l.register_forward_hook(lambda m, i, o: layer_out.append(o.detach().clone()))
                 for l in (model.conv_layers if not cfg.old else [])]
        with torch.no_grad():
            out = model(batch)
        for h in hooks:
            h.remove()
        fixture = {"cfg": cfg.__dict__.copy(), "graph": graph_to_dict(g),
                   "poses": torch.stack([d["ligand"].pos for d in data_list]), "t": c["t"],
                   "state_dict": {k: v.clone() for k, v in sd.items()}}
        if cfg.confidence_mode:   # (confidence, atom_confidence), cg_model.py:353-366; no sampling loop of its own
            if cfg.old:   # legacy class returns the bare confidence tensor (old_cg_model.py:290-291)
                fixture["forward"] = {"confidence": out}
            else:
                fixture["forward"] = {"confidence": out[0], "atom_confidence": out[1], "conv_out": layer_out}
            torch.save(fixture, os.path.join(HERE, f"{name}.pt"))
            print(name, "confidence", fixture["forward"]["confidence"].tolist())
            continue
        tr, rot, tor = out[:3]   # the legacy class returns a 3-tuple
        fixture["forward"] = {"tr": tr, "rot": rot, "tor": tor, "conv_out": layer_out}
        if cfg.sidechain_pred:
            fixture["forward"]["sidechain"] = out[3]

        # ---- reference sampling() with recorded Gaussian draws
        steps = 4
        draws = []
        real_normal = torch.normal

        def rec_normal(*a, **kw):
            z = real_normal(*a, **kw)
            draws.append(z.clone())
            return z
        torch.manual_seed(7)
        ref_sampling.torch.normal = rec_normal
        sched = get_t_schedule("expbeta", steps)
        scheds = (sched, sched ** 1.5, np.sqrt(sched)) if isinstance(c["t"], dict) else (sched, sched, sched)
        dl = copy.deepcopy(data_list)
        temp = dict(temp_sampling=[1.17, 2.06, 7.04], temp_psi=[0.73, 0.90, 0.59], temp_sigma_data=[0.93, 0.75, 0.69]) \
            if name == "tiny_l1" else {}
        try:
            out_list, _ = ref_sampling.sampling(dl, model, steps, *scheds, torch.device("cpu"), t_to_sigma, args,
                                                batch_size=B, no_final_step_noise=True, **temp)
        finally:
            ref_sampling.torch.normal = real_normal
        fixture["sampling"] = {"steps": steps, "temp": temp, "draws": draws,
                               "final_pos": torch.stack([d["ligand"].pos for d in out_list])}
        if isinstance(c["t"], dict):
            fixture["sampling"]["schedules"] = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).clone()
                                                for k, v in zip(("tr", "rot", "tor"), scheds)}
        torch.save(fixture, os.path.join(HERE, f"{name}.pt"))
        print(name, "tr", tr[0].tolist(), "tor", tor[:3].tolist(), "n_draws", len(draws))

    if len(sys.argv) == 1 or "conf_crop" in sys.argv[1:]:
        # ---- sampling() with a confidence model whose args carry crop_beyond (utils/sampling.py:208-227): the confidence graphs
        # are cropped around the final poses before the confidence model sees them.  Score model = tiny_l1, confidence = tiny_conf_l2.
        from tests_util_shim import fixture_case_shim
        fs, cfg_s, dl_s = fixture_case_shim(HERE, "tiny_l1")
        fc, cfg_c, _ = fixture_case_shim(HERE, "tiny_conf_l2")
        args_s, args_c = cfg_s.to_namespace(), cfg_c.to_namespace()
        args_c.crop_beyond = 18.0
        tts = partial(t_to_sigma_compl, args=args_s)
        score = get_model(args_s, torch.device("cpu"), t_to_sigma=tts, no_parallel=True)
        score.load_state_dict(fs["state_dict"], strict=False); score.eval()
        confm = get_model(args_c, torch.device("cpu"), t_to_sigma=partial(t_to_sigma_compl, args=args_c), no_parallel=True,
                          confidence_mode=True)
        confm.load_state_dict(fc["state_dict"], strict=False); confm.eval()
        steps, draws, real_normal = 3, [], torch.normal

        def rec_normal2(*a, **kw):
            z = real_normal(*a, **kw)
            draws.append(z.clone())
            return z
        torch.manual_seed(11)
        ref_sampling.torch.normal = rec_normal2
        kept = []
        real_crop = ref_sampling.crop_beyond

        def rec_crop(g_, cutoff, aa):
            real_crop(g_, cutoff, aa)
            kept.append(int(g_["receptor"].pos.shape[0]))
        ref_sampling.crop_beyond = rec_crop
        sched = get_t_schedule("expbeta", steps)
        try:
            out_list, conf = ref_sampling.sampling(copy.deepcopy(dl_s), score, steps, sched, sched, sched, torch.device("cpu"), tts,
                                                   args_s, confidence_model=confm, confidence_data_list=copy.deepcopy(dl_s),
                                                   confidence_model_args=args_c, batch_size=len(dl_s), no_final_step_noise=True)
        finally:
            ref_sampling.torch.normal = real_normal
            ref_sampling.crop_beyond = real_crop
        assert 0 < min(kept) < dl_s[0]["receptor"].pos.shape[0], kept
        torch.save({"steps": steps, "draws": draws, "crop_beyond": 18.0, "kept_residues": kept, "confidence": conf,
                    "final_pos": torch.stack([d["ligand"].pos for d in out_list])}, os.path.join(HERE, "conf_crop.pt"))
        print("conf_crop kept", kept, "confidence", conf.tolist())
    if len(sys.argv) == 1 or "crop_aa" in sys.argv[1:]:
        # ---- crop_beyond (utils/utils.py:388-413) with all_atoms: residues AND their atoms, atom-atom / atom-residue relations remapped
        from diffdock_amd.synth import make_complex as mk, make_pose_list as mp
        ga = mk(seed=31, n_res=40, n_lig=9, all_atoms=True, atoms_per_res=(3, 7))
        da = mp(ga, 1, seed=32, initial_noise_std_proportion=0.05)[0]
        dc = copy.deepcopy(da)
        crop_beyond(dc, 8.0, True)
        assert 0 < dc["receptor"].pos.shape[0] < da["receptor"].pos.shape[0]
        torch.save({"graph": graph_to_dict(da), "cutoff": 8.0, "rec_pos": dc["receptor"].pos, "rec_x": dc["receptor"].x,
                    "rec_edge_index": dc["receptor", "receptor"].edge_index, "atom_pos": dc["atom"].pos, "atom_x": dc["atom"].x,
                    "atom_edge_index": dc["atom", "atom"].edge_index, "atom_rec_edge_index": dc["atom", "receptor"].edge_index},
                   os.path.join(HERE, "crop_aa.pt"))
        print("crop_aa kept residues", dc["receptor"].pos.shape[0], "of", da["receptor"].pos.shape[0], "atoms", dc["atom"].pos.shape[0])
    if len(sys.argv) > 1:
        return
    # ---- crop_beyond (utils/utils.py:388-413) on one complex
    from diffdock_amd.synth import make_complex, make_pose_list
    g = make_complex(seed=5, n_res=60, n_lig=10)
    d = make_pose_list(g, 1, seed=11)[0]
    dd = copy.deepcopy(d)
    crop_beyond(dd, 9.0, False)
    torch.save({"graph": graph_to_dict(d), "cutoff": 9.0, "rec_pos": dd["receptor"].pos,
                "rec_edge_index": dd["receptor", "receptor"].edge_index}, os.path.join(HERE, "crop_beyond.pt"))

    # ---- geometry / torsion / FasterTensorProduct unit fixtures straight from the reference
    from utils.geometry import axis_angle_to_matrix, rigid_transform_Kabsch_3D_torch_batch
    from utils.diffusion_utils import modify_conformer_batch, sinusoidal_embedding
    from models.layers import GaussianSmearing
    gen = torch.Generator().manual_seed(3)
    aa = torch.randn(16, 3, generator=gen)
    aa[0] = 0
    aa[1] = 1e-7
    A = torch.randn(5, 9, 3, generator=gen)
    Bm = torch.randn(5, 9, 3, generator=gen)
    R, tt = rigid_transform_Kabsch_3D_torch_batch(A, Bm)
    dl = make_pose_list(g, 4, seed=12)
    batch = HeteroBatch.from_data_list(copy.deepcopy(dl))
    nb = batch.num_graphs
    Rr = int(batch["ligand"].edge_mask.sum()) // nb
    tru, rou, tou = torch.randn(nb, 3, generator=gen), torch.randn(nb, 3, generator=gen) * 0.3, torch.randn(nb * Rr, generator=gen)
    mask_rotate = torch.from_numpy(dl[0]["ligand"].mask_rotate[0])
    newpos = modify_conformer_batch(batch["ligand"].pos, batch, tru, rou, tou, mask_rotate)
    ftp = tensor_layers.FasterTensorProduct("8x0e + 3x1o + 3x1e + 8x0o", "1x0e+1x1o", "8x0e + 3x1o + 3x1e + 8x0o")
    x = torch.randn(7, 8 + 9 + 9 + 8, generator=gen)
    sh = torch.randn(7, 4, generator=gen)
    w = torch.randn(7, ftp.weight_numel, generator=gen)
    ts = torch.tensor([0.0, 0.05, 0.5, 1.0])
    gs = GaussianSmearing(0.0, 5.0, 16)
    dist = torch.rand(9, generator=gen) * 6
    torch.save({"axis_angle": aa, "rot_mats": axis_angle_to_matrix(aa), "kabsch_A": A, "kabsch_B": Bm, "kabsch_R": R,
                "kabsch_t": tt, "mc_graph": graph_to_dict(g), "mc_pos_in": batch["ligand"].pos.clone(), "mc_tr": tru,
                "mc_rot": rou, "mc_tor": tou, "mc_pos_out": newpos,
                "ftp_x": x, "ftp_sh": sh, "ftp_w": w, "ftp_out": ftp(x, sh, w),
                "sin_t": ts, "sin_emb": sinusoidal_embedding(1000.0 * ts, 16),
                "gs_dist": dist, "gs_out": gs(dist), "t_schedule_20": torch.from_numpy(get_t_schedule("expbeta", 20))},
               os.path.join(HERE, "units.pt"))
    for f in (".p.npy", ".score.npy"):      # 0.4 GB of torus caches: do not leave them in the tree
        if os.path.exists(f):
            os.remove(f)
    print("done")


if __name__ == "__main__":
    main()
