"""A reused model handle gives the results of a fresh one: the history scripts of tests/history_cases.py on the CPU emulation build
(tests/hipemu), at reduced sizes.  The full matrix runs at TINY; at the DDL width (ns = 48, nv = 10) scripts 1 and 2 at the smallest
sizes with two layers -- one emulator step at that width takes tens of seconds -- and the rest of the width-48 matrix runs on the
MI355X only (tests/test_gpu_history.py).  DDMI_STREAMS=1 runs here too, although the emulator executes every stream in launch order:
the host-side bookkeeping of the one-stream route is the same code."""
import os
import subprocess

import pytest

from diffdock_amd.config import TINY
from diffdock_amd.model import MIScoreModel
from util import tables
import history_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "hipemu", "libddmi_emu.so")
S = H.EMU_SIZES


@pytest.fixture(scope="module")
def make():
    r = subprocess.run(["make", "-j8", "-C", os.path.join(ROOT, "diffdock_amd", "csrc"), "emu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def mk(cfg, sd):     # (reads the DDMI_* route variables of the moment: lib.make_config)
        m = MIScoreModel(cfg, device="cpu", lib_path=EMU)
        m.load_state_dict(sd)
        m.set_tables(*tables())
        return m
    return mk


def place(x):
    return x


FORCED = (("DDMI_FUSED_PRERED", "0"), ("DDMI_FUSED_SHARED", "2"), ("DDMI_FUSED_DENSE", "2"))


@pytest.mark.parametrize("variant", [{}, dict(sh_lmax=2, edge_product="bf16x4"), dict(exec_options=(("tile_per_pose", 1),)), "forced"],
                         ids=["default", "lmax2_bf16x4", "tile_per_pose", "forced_routes"])
def test_sizes_script(make, variant, monkeypatch):
    if variant == "forced":     # in-tile pre-reduction off, the shared-node kernel on every group
        for k, v in FORCED:
            monkeypatch.setenv(k, v)
        variant = {}
    H.run_script(make, place, TINY.replace(**variant), H.sizes_script(S), f"sizes {variant}")


def test_sizes_script_at_the_ddl_width(make):
    H.run_script(make, place, H.width48(layers=2), H.sizes_script(H.EMU_SIZES_48), "sizes ns=48")


ROUTES = [None, ("DDMI_REC_SHARE", "1"), ("DDMI_LAYER_OVERLAP", "1"), ("DDMI_GROUPED", "1"), ("DDMI_GROUPED", "2"), ("DDMI_NODE_UPDATE", "1"),
          ("DDMI_VN_BUILD", "1"), ("DDMI_STREAMS", "1"), ("DDMI_TILE_PER_POSE", "1")]


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: "default" if r is None else "=".join(r))
def test_live_batch_script(make, route, monkeypatch, capfd):
    if route:
        monkeypatch.setenv(*route)
    monkeypatch.setenv("DDMI_DEBUG_GRAN", "1")
    grouped = route == ("DDMI_GROUPED", "2")     # the grouped dispatch keeps the full rec-rec group (conv_layers.cpp: run_cg_layers)
    cfg = H.calm(TINY.replace(sidechain_pred=True))
    sizes = S if route is None else H.EMU_SIZES_ROUTES
    H.run_script(make, place, cfg, H.live_batch_script(sizes, sidechain=True), f"live batch {route}", share=False if grouped else "auto",
                 route_lines=None if grouped else True, listing=lambda: capfd.readouterr().err)


def test_live_batch_script_at_the_ddl_width(make):
    H.run_script(make, place, H.calm(H.width48(layers=2)), H.live_batch_script(H.EMU_SIZES_48), "live batch ns=48")


def test_guard_groups_and_layouts_script(make):
    H.run_script(make, place, TINY, H.guard_groups_script(S), "guard groups")


def test_in_place_edits_script(make):
    H.run_script(make, place, TINY.replace(lm_embedding_type=None), H.edits_script(S), "edits")


def test_all_atom_sizes_script(make):
    H.run_script(make, place, H.TINY_AA, H.sizes_script(S, all_atoms=True), "all-atom sizes", share=None)


@pytest.mark.parametrize("old", [False, True], ids=["new_class", "legacy_class"])
def test_confidence_and_score_handles_alternate(make, old):
    H.confidence_and_score_case(make, place, S, old=old)


def test_two_handles_interleaved(make):
    H.two_handles_case(make, place, S, TINY, TINY.replace(sh_lmax=2, num_conv_layers=3, lm_embedding_type=None))


def test_long_loop_equals_the_step_wise_loop(make):
    H.long_loop_case(make, place, S, cfg=TINY.replace(num_conv_layers=2))
