"""Pose metrics on the device (ddmi_pose_metrics, MIScoreModel.pose_metrics, diffdock_amd.metrics) on the CPU emulation build
(tests/hipemu), plus the ABI of ddmi_pose_metrics_cfg.  Case bodies live in tests/metrics_cases.py; tests/test_gpu_metrics.py runs
them on the MI355X."""
import ctypes
import os
import re
import subprocess

import pytest

import diffdock_amd.lib as L
from diffdock_amd.model import MIScoreModel
from util import tables
import metrics_cases as M

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


@pytest.mark.parametrize("shape", M.EDGE_SHAPES)
def test_edge_shapes(make, shape):
    M.edge_shape_case(make, place, shape)


def test_atom_index_and_exact_ties_fall_to_the_lowest_index(make):
    M.atom_index_ties_case(make, place)


def test_values_do_not_depend_on_the_other_poses_references_or_permutations(make):
    M.independence_case(make, place)


def test_evaluate_poses(make):
    M.evaluate_case(make, place)


def test_errors(make):
    M.errors_case(make, place)


def test_pose_metrics_cfg_mirror_matches_the_header():
    header = open(os.path.join(ROOT, "include", "ddmi.h")).read()
    body = re.search(r"typedef struct ddmi_pose_metrics_cfg \{(.*?)\} ddmi_pose_metrics_cfg;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "ptr": ctypes.c_void_p}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.+)$", decl)
        assert m, decl
        for name in (n.strip() for n in m.group(4).split(",")):
            fields.append((name, ctype["ptr" if m.group(3) else m.group(2)]))
    assert fields == list(L.PoseMetricsCfg._fields_)
    assert ctypes.sizeof(L.PoseMetricsCfg) == 128 and L.PoseMetricsCfg.pos.offset == 32
    assert "ddmi_pose_metrics" in L.EXPORTED_SYMBOLS
    assert re.search(r"int ddmi_pose_metrics\(ddmi_model\* m, const ddmi_pose_metrics_cfg\* cfg, ddmi_stream stream\);", header)
