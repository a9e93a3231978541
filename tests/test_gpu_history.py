"""A reused model handle gives the results of a fresh one, on the MI355X: the history scripts of tests/history_cases.py at their full
sizes and at the DDL width (ns = 48, nv = 10), where the fused routes, the in-tile pre-reduction and the tile_per_pose padding keep
lists of their own.  tests/test_emu_history.py runs the same scripts, reduced, on the CPU emulation build."""
import pytest
import torch

from diffdock_amd.config import DDL_SYNTH, TINY
from diffdock_amd.model import MIScoreModel
from util import tables
import history_cases as H

pytestmark = pytest.mark.gpu
S = H.GPU_SIZES


def make(cfg, sd):     # (reads the DDMI_* route variables of the moment: lib.make_config)
    assert torch.cuda.is_available(), "these tests need the MI355X (-m gpu)"
    m = MIScoreModel(cfg, device="cuda:0")     # raises DdmiError if libddmi.so is not built: no fallback
    m.load_state_dict(sd)
    m.set_tables(*tables())
    return m


def place(x):
    return x.to("cuda:0")


SIZES_CFGS = {"tiny": lambda: TINY, "w48_l1": lambda: H.width48(3, 1), "w48_l2": lambda: H.width48(3, 2),
              "w48_bf16x4": lambda: H.width48(3, 1, edge_product="bf16x4"),
              "w48_tile_per_pose": lambda: H.width48(3, 1, exec_options=(("tile_per_pose", 1),))}


@pytest.mark.parametrize("name", list(SIZES_CFGS))
def test_sizes_script(name):
    H.run_script(make, place, SIZES_CFGS[name](), H.sizes_script(S), f"sizes {name}")


def test_sizes_script_on_forced_routes(monkeypatch):
    for k, v in (("DDMI_FUSED_PRERED", "0"), ("DDMI_FUSED_SHARED", "2"), ("DDMI_FUSED_DENSE", "2")):
        monkeypatch.setenv(k, v)
    H.run_script(make, place, H.width48(3, 1), H.sizes_script(S), "sizes forced routes")


ROUTES = [None, ("DDMI_REC_SHARE", "1"), ("DDMI_REC_SHARE", "0"), ("DDMI_LAYER_OVERLAP", "1"), ("DDMI_GROUPED", "1"), ("DDMI_GROUPED", "2"),
          ("DDMI_NODE_UPDATE", "1"), ("DDMI_VN_BUILD", "1"), ("DDMI_STREAMS", "1"), ("DDMI_TILE_PER_POSE", "1")]


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: "default" if r is None else "=".join(r))
def test_live_batch_script(route, monkeypatch, capfd):
    if route:
        monkeypatch.setenv(*route)
    monkeypatch.setenv("DDMI_DEBUG_GRAN", "1")
    # the fused node update and the grouped dispatch keep the full rec-rec group (conv_layers.cpp: run_cg_layers)
    share = False if route in (("DDMI_REC_SHARE", "0"), ("DDMI_GROUPED", "2"), ("DDMI_NODE_UPDATE", "1")) else "auto"
    cfg = H.calm(H.width48(3, 1, sidechain_pred=True))
    H.run_script(make, place, cfg, H.live_batch_script(S, sidechain=True), f"live batch {route}", share=share,
                 route_lines=route != ("DDMI_GROUPED", "2"), listing=lambda: capfd.readouterr().err)


@pytest.mark.parametrize("cfg", [TINY, H.width48(3, 1, lm_embedding_type="precomputed")], ids=["tiny", "w48"])
def test_guard_groups_and_layouts_script(cfg):
    H.run_script(make, place, cfg, H.guard_groups_script(S), "guard groups")


def test_in_place_edits_script_at_the_ddl_width():
    H.run_script(make, place, H.width48(3, 1), H.edits_script(S), "edits")


@pytest.mark.parametrize("cfg", [H.TINY_AA, DDL_SYNTH.replace(all_atoms=True, num_conv_layers=3, lm_embedding_type=None)], ids=["tiny_aa", "w48_aa"])
def test_all_atom_sizes_script(cfg):
    H.run_script(make, place, cfg, H.sizes_script(S, all_atoms=True), "all-atom sizes", share=None)


@pytest.mark.parametrize("old", [False, True], ids=["new_class", "legacy_class"])
def test_confidence_and_score_handles_alternate(old):
    H.confidence_and_score_case(make, place, S, old=old)


def test_two_handles_interleaved():
    H.two_handles_case(make, place, S, H.width48(3, 1), H.width48(3, 1))
    H.two_handles_case(make, place, S, H.width48(3, 1), TINY.replace(lm_embedding_type=None))


@pytest.mark.parametrize("cfg", [TINY, H.width48(3, 1)], ids=["tiny", "w48"])
def test_long_loop_equals_the_step_wise_loop(cfg):
    H.long_loop_case(make, place, S, cfg=cfg)
