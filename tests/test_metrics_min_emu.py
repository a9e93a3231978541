"""The minimised symmetric RMSD and the fitting transform (ddmi_pose_fit, MIScoreModel.pose_fit, evaluate_poses(minimize=True)) on
the CPU emulation build (tests/hipemu), plus the ABI of ddmi_pose_fit_cfg.  Case bodies live in tests/metrics_min_cases.py;
tests/test_gpu_metrics_min.py runs them on the MI355X."""
import ctypes
import os
import re
import subprocess

import pytest

import diffdock_amd.lib as L
from diffdock_amd.model import MIScoreModel
from util import tables
import metrics_min_cases as M

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


@pytest.mark.parametrize("name", ["1a0q", "sym576"])
def test_fixture_molecules_match_the_executed_spyrmsd(make, name):
    M.fixture_case(make, place, name)


@pytest.mark.parametrize("name", ["1a0q", "sym576"])
def test_rigid_copies_match_the_executed_spyrmsd(make, name):
    M.rigid_case(make, place, name)


@pytest.mark.parametrize("name", M.SMALL_SETS)
def test_small_sets_match_the_executed_spyrmsd(make, name):
    M.small_set_case(make, place, name)


@pytest.mark.parametrize("shape", M.EDGE_SHAPES)
def test_edge_shapes(make, shape):
    M.edge_shape_case(make, place, shape)


def test_values_do_not_depend_on_the_other_poses_references_or_permutations(make):
    M.independence_case(make, place)


def test_evaluate_poses_minimize_and_superpose(make):
    M.evaluate_case(make, place)


def test_errors(make):
    M.errors_case(make, place)


def test_pose_fit_cfg_mirror_matches_the_header():
    header = open(os.path.join(ROOT, "include", "ddmi.h")).read()
    body = re.search(r"typedef struct ddmi_pose_fit_cfg \{(.*?)\} ddmi_pose_fit_cfg;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "ptr": ctypes.c_void_p}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.+)$", decl)
        assert m, decl
        for name in (n.strip() for n in m.group(4).split(",")):
            fields.append((name, ctype["ptr" if m.group(3) else m.group(2)]))
    assert fields == list(L.PoseFitCfg._fields_)
    assert ctypes.sizeof(L.PoseFitCfg) == 96 and L.PoseFitCfg.pos.offset == 24
    assert "ddmi_pose_fit" in L.EXPORTED_SYMBOLS
    assert re.search(r"int ddmi_pose_fit\(ddmi_model\* m, const ddmi_pose_fit_cfg\* cfg, ddmi_stream stream\);", header)
    # the neighbour is untouched
    assert ctypes.sizeof(L.PoseMetricsCfg) == 128
