"""One time per graph and per noise type on the MI355X against the float64 oracle.

ddmi_forward takes t_tr[B], t_rot[B] and t_tor[B]; ddmi_sample takes three schedules.  With one shared t, a time-dependent
quantity taken from the wrong graph (time embedding, hidden-row bias W1e . sig, receptor sigma rows, dynamic cross cutoff, the
score heads' sigma and table lookups) or from the wrong noise type gives exactly the right answer.  Here every pose has its own
three times: tiles that straddle poses in every kernel variant, every selectable route, the discrete score-norm lookups next to
their rounding boundaries and at the clip ends, crops and step coefficients under three schedules, the all-atom model.
The bodies live in tests/cases.py; tests/test_emu_parity.py runs them on the CPU emulation build."""
import pytest
import torch

import cases
from diffdock_amd.config import DDL_SYNTH, TINY
from diffdock_amd.hetero import HeteroBatch
from diffdock_amd.model import MIScoreModel
from diffdock_amd.synth import make_complex, make_pose_list
from diffdock_amd.weights import init_state_dict
from util import elem_excess, oracle_model, rel_err, set_times, tables

pytestmark = pytest.mark.gpu


def gpu_model(cfg, sd):
    assert torch.cuda.is_available(), "these tests need an MI355X (pytest -m gpu)"
    m = MIScoreModel(cfg, device="cuda:0")     # raises DdmiError if libddmi.so is not built: no fallback
    m.load_state_dict(sd)
    m.set_tables(*tables())
    return m


def to_gpu(x):
    return x.to("cuda:0")


# the B = 3 shapes of the tile-boundary sweep (tests/test_gpu_edges.py): 15 / 93, 33 / 96, 93 / 15, 96 / 33 virtual nodes
VARIANTS = {
    "l1": dict(ns=48, nv=10, sh_lmax=1),
    "l1bf": dict(ns=48, nv=10, sh_lmax=1, edge_product="bf16x4"),
    "l2": dict(ns=48, nv=10, sh_lmax=2),
    "ns16": dict(ns=16, nv=10, sh_lmax=1),
}
SHAPES = [(5, 31), (11, 32), (31, 5), (32, 11)]
TILE_CASES = [(r, l, v, False) for r, l in SHAPES for v in VARIANTS] + [(32, 11, "l2", True), (11, 32, "l1", True)]


@pytest.mark.parametrize("n_res,n_lig,variant,dynamic", TILE_CASES,
                         ids=[f"r{r}-l{l}-{v}" + ("-dyncross" if d else "") for r, l, v, d in TILE_CASES])
def test_straddling_tiles_with_per_graph_times(n_res, n_lig, variant, dynamic):
    cases.mixed_times_tile_case(gpu_model, to_gpu, n_res, n_lig, VARIANTS[variant], dynamic)


@pytest.fixture(scope="module")
def width48_mixed_case():
    """test_gpu_parity.py's width48_case with one time per graph and noise type (3 poses)."""
    cfg = DDL_SYNTH
    sd = init_state_dict(cfg, seed=1234)
    g = make_complex(seed=5, n_res=100, n_lig=40)        # 40-atom ligand: receptor residues with two virtual nodes
    batch = HeteroBatch.from_data_list(make_pose_list(g, 3, tr_sigma_max=cfg.tr_sigma_max, seed=6, initial_noise_std_proportion=0.6))
    set_times(batch, *cases._times(cases.MIXED_T, 3))
    ref = oracle_model(cfg, sd, dtype=torch.float64)(batch)[:3]
    return cfg, sd, batch, ref


@pytest.mark.parametrize("env", [{}, {"DDMI_FUSED_PACK": "0"}, {"DDMI_FUSED_DENSE": "0"},
                                 {"DDMI_FUSED_DENSE": "2"}, {"DDMI_FUSED_MM": "0"}, {"DDMI_STREAMS": "1"}, {"DDMI_FUSED_YS": "3"},
                                 {"DDMI_FUSED_SHARED": "0"}, {"DDMI_FUSED_SHARED": "2", "DDMI_FUSED_DENSE": "2"}, {"DDMI_FC1_BATCH": "0"}, {"DDMI_FUSED_TRI": "0"}, {"DDMI_FUSED_PRERED": "0"},
                                 {"DDMI_GROUPED": "1"}, {"DDMI_GROUPED": "2"}, {"DDMI_GROUPED": "2", "DDMI_GROUPED_YS": "3"},
                                 {"DDMI_GROUPED": "2", "DDMI_FUSED_PRERED": "0", "DDMI_FUSED_SHARED": "0"},
                                 {"DDMI_NODE_UPDATE": "1"}, {"DDMI_VN_BUILD": "1"}, {"DDMI_LIST_CAPS": "1"}, {"DDMI_YS_RULE": "1"}, {"DDMI_TIME_TERMS": "1"}, {"DDMI_GROUP_ORDER": "3", "DDMI_FUSED_YS_LAST": "2"}, {"DDMI_NODE_UPDATE": "1", "DDMI_VN_BUILD": "1", "DDMI_GROUPED": "2"},
                                 {"DDMI_TILE_PER_POSE": "1"}, {"DDMI_LAYER_OVERLAP": "2"}, {"DDMI_TIME_TERMS": "1", "DDMI_NODE_UPDATE": "1"}],
                         ids=lambda e: ",".join(f"{k[5:]}={v}" for k, v in e.items()) or "default")
def test_every_route_with_per_graph_times_matches_oracle(env, width48_mixed_case, monkeypatch):
    """Each route of test_selectable_kernel_paths_agree_on_the_gpu (and tile_per_pose, layer_overlap) against the float64
    oracle itself, element by element, not against the default route, which could share a per-graph indexing bug."""
    cfg, sd, batch, ref = width48_mixed_case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = gpu_model(cfg, sd)
    out = m(to_gpu(batch))[:3]
    for o, r, n in zip(out, ref, ("tr", "rot", "tor")):
        o = o.cpu()
        assert rel_err(o, r) < 1e-4 and elem_excess(o, r) <= 1.0, (n, rel_err(o, r), elem_excess(o, r))


def test_score_norm_bins_next_to_rounding_boundaries():
    t_rot, t_tor = cases.score_norm_times(TINY)
    cases.score_norm_bins_case(gpu_model, to_gpu, TINY, t_rot, t_tor)


def test_score_norm_bins_at_the_clip_ends_and_nan_rows():
    cfg, t_rot, t_tor = cases.clip_end_config()
    nan_rows = cases.score_norm_bins_case(gpu_model, to_gpu, cfg, t_rot, t_tor)
    assert nan_rows.any()


def test_crop_under_three_schedules_matches_oracle():
    cases.crop_under_three_schedules_case(gpu_model, to_gpu)


def test_three_schedules_native_and_stepwise():
    cases.three_schedules_loops_case(gpu_model, to_gpu, "cuda:0")


def test_all_atom_ddl_width_with_per_graph_times():
    cases.all_atom_mixed_times_case(gpu_model, to_gpu)
