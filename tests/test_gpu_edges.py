"""Edge shapes and forced kernel routes on the MI355X against the oracle.

The shared cases of tests/cases.py that tests/test_emu_parity.py runs on the CPU emulation build, here on cuda:0: the
emulator runs each thread as a fiber up to the next barrier and ignores the range of a buffer resource, so barriers, LDS
races, lane layouts, buffer ranges and zero-size / partial launches are only proven on the hardware.  And a tile-boundary
sweep (GPU only): every ligand-atom x residue pair is a cross edge, so the shape alone fixes how many virtual nodes each
edge group has and where its 16-virtual-node tiles end; each case asserts the counts it claims and compares the scores and
the node tables element by element with the float64 oracle."""
import math

import pytest
import torch

import cases
from diffdock_amd.config import DDL_SYNTH
from diffdock_amd.hetero import HeteroBatch, set_time
from diffdock_amd.model import MIScoreModel
from diffdock_amd.synth import make_complex, make_pose_list
from diffdock_amd.weights import init_state_dict
from util import assert_scores_close, elem_excess, oracle_model, rel_err, tables

pytestmark = pytest.mark.gpu


def gpu_model(cfg, sd):
    assert torch.cuda.is_available(), "these tests need an MI355X (pytest -m gpu)"
    m = MIScoreModel(cfg, device="cuda:0")     # raises DdmiError if libddmi.so is not built: no fallback
    m.load_state_dict(sd)
    m.set_tables(*tables())
    return m


def to_gpu(x):
    return x.to("cuda:0")


# ---- the shared cases ----

def test_no_cross_edges_and_ragged_batch():
    cases.no_cross_edges_and_ragged_batch_case(gpu_model, to_gpu)


@pytest.mark.parametrize("no_torsion", [False, True])
def test_rigid_ligand_and_no_torsion_early_out(no_torsion):
    cases.rigid_ligand_case(gpu_model, to_gpu, no_torsion)


@pytest.mark.parametrize("n_res,n_lig,B", [(20, 8, 1), (3, 4, 2), (40, 2, 3)])
def test_degenerate_sizes(n_res, n_lig, B):
    cases.degenerate_sizes_case(gpu_model, to_gpu, n_res, n_lig, B)


@pytest.mark.parametrize("lmax,edge_product", [(1, "f32"), (1, "bf16x4"), (2, "f32")])
def test_fused_conv_full_width_matches_oracle(lmax, edge_product, monkeypatch):
    cases.fused_conv_full_width_case(gpu_model, to_gpu, monkeypatch.setenv, lmax, edge_product)


@pytest.mark.parametrize("ns", [16, 32])
def test_packing_is_dropped_in_layers_with_generic_granules(ns, monkeypatch, capfd):
    cases.packing_dropped_case(gpu_model, to_gpu, monkeypatch.setenv, ns, listing=lambda: capfd.readouterr().err)


@pytest.mark.parametrize("edge_product", ["f32", "bf16x4"])
def test_shared_node_contraction_matches_oracle(edge_product, monkeypatch):
    cases.shared_node_contraction_case(gpu_model, to_gpu, monkeypatch.setenv, edge_product)


@pytest.mark.parametrize("edge_product", ["f32", "bf16x4"])
def test_in_tile_pre_reduction_of_lig_rec_messages(edge_product, monkeypatch):
    cases.in_tile_pre_reduction_case(gpu_model, to_gpu, monkeypatch.setenv, edge_product)


@pytest.mark.parametrize("name", ["tiny_l1", "tiny_l2"])
def test_readout_tensor_product_forms_agree(name, monkeypatch):
    cases.readout_tensor_product_forms_case(gpu_model, to_gpu, monkeypatch.setenv, name)


def test_ligand_atoms_with_many_receptor_neighbours():
    cases.many_receptor_neighbours_case(gpu_model, to_gpu)


@pytest.mark.parametrize("edge_product", ["f32", "bf16x4"])
def test_fused_node_update_matches_separate_launches(edge_product):
    """node_update 1 (the shape picked by size), 2 and 3 (the two workgroup shapes forced)."""
    cases.fused_node_update_case(gpu_model, to_gpu, modes=(1, 2, 3), edge_product=edge_product)


def test_all_atom_ragged_batch_and_empty_ligand_atom_group():
    cases.all_atom_ragged_batch_case(gpu_model, to_gpu)


def test_crop_with_embedding_layers_matches_oracle():
    cases.crop_with_embedding_layers_case(gpu_model, to_gpu)


def test_sidechain_pred_under_a_device_crop_and_after_other_passes():
    cases.sidechain_pred_under_crop_case(gpu_model, to_gpu)


# ---- tile-boundary sweep against the float64 oracle ----
# With a static 80 A cross cutoff every (ligand atom, residue) pair of a pose is an edge, so a residue has n_lig edges in the
# rec<-lig group and a ligand atom n_res edges in the lig<-rec group.  A virtual node holds at most 32 edges, FC_VN = 16 virtual
# nodes form a tile:  rec-gather virtual nodes = B * n_res * ceil(n_lig / 32),  lig-gather = B * n_lig * ceil(n_res / 32).
# The shapes put 15 (partial tile), 16 (exact), 17 (tile + 1) or 33 (two tiles + 1) virtual nodes into one of the groups, 1 / 2 / 3
# virtual nodes per node (31, 32, 33, 65 edges: last virtual node full, exact, 1 edge), and B = 3 makes tiles straddle poses.

VARIANTS = {
    "l1": dict(ns=48, nv=10, sh_lmax=1),                               # static main loop of k_conv_fused
    "l1bf": dict(ns=48, nv=10, sh_lmax=1, edge_product="bf16x4"),     # the same loops with the split-bf16 edge product
    "l2": dict(ns=48, nv=10, sh_lmax=2),                               # generic (compiler-scheduled) variant
    "ns16": dict(ns=16, nv=10, sh_lmax=1),                             # predicated generic variant (4-step scalar chains)
}
SWEEP = {   # (n_res, n_lig, B): variants         rec-gather vn / lig-gather vn
    (15, 31, 1): ["l1", "l1bf"],                  # 15 / 31
    (16, 32, 1): ["l2", "l1bf"],                  # 16 / 32
    (8, 33, 1): ["ns16", "l2", "l1", "l1bf"],     # 16 (second virtual node of each residue: 1 edge) / 33
    (5, 65, 1): ["ns16", "l2", "l1"],             # 15 (3 per residue) / 65
    (11, 65, 1): ["l1bf"],                        # 33 / 65
    (31, 17, 1): ["ns16", "l2", "l1", "l1bf"],    # 31 / 17
    (32, 16, 1): ["ns16", "l2", "l1"],            # 32 / 16
    (33, 8, 1): ["ns16", "l1", "l1bf"],           # 33 / 16 (2 per ligand atom)
    (65, 5, 1): ["ns16", "l1", "l1bf"],           # 65 / 15 (3 per ligand atom)
    (65, 11, 1): ["l2"],                          # 65 / 33
    (5, 31, 3): ["ns16", "l2"],                   # 15 / 93
    (11, 32, 3): ["ns16", "l1"],                  # 33 / 96
    (31, 5, 3): ["l1", "l1bf"],                   # 93 / 15
    (32, 11, 3): ["l2", "l1bf"],                  # 96 / 33
    (33, 17, 1): ["ns16", "l2"],                  # 33 / 34
}
SWEEP_CASES = [(r, l, B, v) for (r, l, B), vs in SWEEP.items() for v in vs]


@pytest.mark.parametrize("n_res,n_lig,B,variant", SWEEP_CASES, ids=[f"r{r}-l{l}-B{B}-{v}" for r, l, B, v in SWEEP_CASES])
def test_tile_boundary_sweep_matches_float64_oracle(n_res, n_lig, B, variant):
    cfg = DDL_SYNTH.replace(num_conv_layers=4, lm_embedding_type=None, dynamic_max_cross=False, cross_max_distance=80.0,
                            tr_sigma_max=5.0, **VARIANTS[variant])
    sd = init_state_dict(cfg, seed=7)
    g = make_complex(seed=100 + n_res, n_res=n_res, n_lig=n_lig, lm_dim=0)
    dl = make_pose_list(g, B, tr_sigma_max=cfg.tr_sigma_max, seed=n_lig, initial_noise_std_proportion=0.3)
    batch = HeteroBatch.from_data_list(dl)
    set_time(batch, 0.6, 0.6, 0.6, B)
    tr, rot, tor, _, inter = oracle_model(cfg, sd, dtype=torch.float64)(batch, return_intermediates=True)
    m = gpu_model(cfg, sd)
    out = m(to_gpu(batch))[:3]
    # the boundary this case claims is the one the kernels saw
    assert inter["edge_counts"][1] == B * n_lig * n_res == int(m.debug_buffer("offs_l")[-1])
    assert int(m.debug_buffer("vn_off_cross")[-1]) == B * n_res * math.ceil(n_lig / 32)
    assert int(m.debug_buffer("vn_off_rl")[-1]) == B * n_lig * math.ceil(n_res / 32)
    R = int(g["ligand"].edge_mask.sum())
    assert tor.shape == out[2].shape == (B * R,)
    assert_scores_close(out[:2 + (R > 0)], (tr, rot, tor)[:2 + (R > 0)], what=f"{n_res}/{n_lig}/{B}/{variant}")
    for l in range(1, cfg.num_conv_layers):   # node tables after every layer that updates all rows: ligand atoms, then residues
        ref = inter[f"node_attr{l}"]
        mine = torch.from_numpy(m.debug_buffer(f"x{l}"))[:ref.shape[0], :ref.shape[1]]
        assert rel_err(mine, ref) < 1e-4 and elem_excess(mine, ref) <= 1.0, (l, rel_err(mine, ref), elem_excess(mine, ref))
