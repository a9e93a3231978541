"""Conformer matching (ddmi_match_conformer, MIScoreModel.match_conformer, diffdock_amd.matching, io.complex_graph(conformers=...)) on
the CPU emulation build (tests/hipemu), plus the ABI of ddmi_match_cfg.  Case bodies live in tests/matching_cases.py;
tests/test_gpu_matching.py runs them on the MI355X.  The quality cases against the host route run on the MI355X only: the emulator
needs minutes for their budgets (40 x 40 and 40 x 200 generations)."""
import ctypes
import os
import re
import subprocess

import pytest

import diffdock_amd.lib as L
from diffdock_amd.model import MIScoreModel
from util import tables
import matching_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "hipemu", "libddmi_emu.so")


@pytest.fixture(scope="module")
def emu_lib():
    r = subprocess.run(["make", "-j8", "-C", os.path.join(ROOT, "diffdock_amd", "csrc"), "emu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return EMU


@pytest.fixture(scope="module")
def make(emu_lib):
    def mk(cfg, sd):
        m = MIScoreModel(cfg, device="cpu", lib_path=emu_lib)
        m.load_state_dict(sd)
        m.set_tables(*tables())
        return m
    return mk


def place(x):
    return x


@pytest.mark.parametrize("n", M.OBJECTIVE_SHAPES)
def test_objective_matches_the_float64_restatement(make, n):
    M.objective_case(make, place, n)


@pytest.mark.parametrize("budget", [M.SMALL, M.ODD], ids=["popsize8", "popsize7"])
def test_results_do_not_depend_on_the_batch_and_repeat(make, budget):
    M.determinism_case(make, place, budget)


def test_edges(make):
    M.edges_case(make, place)


def test_errors(make):
    M.errors_case(make, place)


def test_tries_of_one_ligand_in_one_call(make):
    M.tries_case(make, place)


def test_complex_graph_with_conformers(make, tmp_path):
    M.complex_graph_case(make, place, tmp_path)


def test_complex_graph_with_conformers_host_route(tmp_path):
    M.complex_graph_case(None, place, tmp_path, device_route=False)


def test_host_route_reaches_the_generating_conformer():
    job = M.synth_job(1, 5, noise=0.0)
    res = M.match_conformers_host([((job["u"], job["v"], job["mask"]), job["start"], job["target"])], popsize=5, maxiter=10)[0]
    assert res["rmsd"] < 1e-3 and res["rmsds"].shape == (1,) and res["best"] == 0


def test_match_cfg_mirror_matches_the_header():
    header = open(os.path.join(ROOT, "include", "ddmi.h")).read()
    body = re.search(r"typedef struct ddmi_match_cfg \{(.*?)\} ddmi_match_cfg;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64, "ptr": ctypes.c_void_p}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.+)$", decl)
        assert m, decl
        for name in (n.strip() for n in m.group(4).split(",")):
            fields.append((name, ctype["ptr" if m.group(3) else m.group(2)]))
    assert fields == list(L.MatchCfg._fields_)
    assert ctypes.sizeof(L.MatchCfg) == 160 and L.MatchCfg.seed.offset == 24 and L.MatchCfg.lig_ptr.offset == 32
    assert "ddmi_match_conformer" in L.EXPORTED_SYMBOLS
    assert re.search(r"int ddmi_match_conformer\(ddmi_model\* m, const ddmi_match_cfg\* cfg, ddmi_stream stream\);", header)
    # the neighbours are untouched
    assert ctypes.sizeof(L.PoseFitCfg) == 96 and ctypes.sizeof(L.PoseMetricsCfg) == 128 and ctypes.sizeof(L.NeighborGraphCfg) == 96
    assert ctypes.sizeof(L.RandomizeCfg) == 72
