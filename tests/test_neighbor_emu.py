"""Neighbour lists on the device (ddmi_neighbor_graph, MIScoreModel.neighbor_graph, diffdock_amd.io.neighbor_graph) on the CPU
emulation build (tests/hipemu), plus the ABI of ddmi_neighbor_graph_cfg.  Case bodies live in tests/neighbor_cases.py;
tests/test_gpu_neighbor.py runs them on the MI355X."""
import ctypes
import os
import re
import subprocess

import pytest

import diffdock_amd.lib as L
from diffdock_amd.model import MIScoreModel
from util import tables
import neighbor_cases as N

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


@pytest.mark.parametrize("name", list(N.INPUTS))
def test_1a0q_rows_equal_the_float64_oracle(make, name):
    N.exact_case(make, place, name)


@pytest.mark.parametrize("name", ["atoms_5_8", "atoms_5_uncapped"])
def test_1a0q_atom_graph_against_the_executed_reference(make, name):
    N.fixture_case(make, place, name)


@pytest.mark.parametrize("name", list(N.SHAPES))
def test_small_shapes(make, name):
    N.shape_case(make, place, name)


def test_rows_do_not_depend_on_the_other_sets(make):
    N.independence_case(make, place)


def test_abi_and_errors(make):
    N.abi_case(make, place)


def test_neighbor_graph_cfg_mirror_matches_the_header():
    header = open(os.path.join(ROOT, "include", "ddmi.h")).read()
    body = re.search(r"typedef struct ddmi_neighbor_graph_cfg \{(.*?)\} ddmi_neighbor_graph_cfg;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
             "ptr": ctypes.c_void_p}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.+)$", decl)
        assert m, decl
        for name in (n.strip() for n in m.group(4).split(",")):
            fields.append((name, ctype["ptr" if m.group(3) else m.group(2)]))
    assert fields == list(L.NeighborGraphCfg._fields_)
    assert ctypes.sizeof(L.NeighborGraphCfg) == 96 and L.NeighborGraphCfg.capacity.offset == 24 and L.NeighborGraphCfg.pos.offset == 32
    assert "ddmi_neighbor_graph" in L.EXPORTED_SYMBOLS
    assert re.search(r"int ddmi_neighbor_graph\(ddmi_model\* m, const ddmi_neighbor_graph_cfg\* cfg, ddmi_stream stream\);", header)
