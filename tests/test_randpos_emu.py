"""Initial poses on the device (ddmi_randomize_position, HeteroBatch.replicate, sampling.sample_poses) on the CPU emulation build
(tests/hipemu), plus the ABI of ddmi_randomize_cfg.  Case bodies live in tests/randpos_cases.py; tests/test_gpu_randpos.py runs
them on the MI355X."""
import ctypes
import os
import re
import subprocess

import pytest

import diffdock_amd.lib as L
from diffdock_amd.model import MIScoreModel
from util import tables
import randpos_cases as P

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


def test_injected_draws_reproduce_the_reference_execution(make):
    P.fixture_case_injected(make, place)


def test_library_draws_match_the_float64_restatement(make):
    P.generator_path_case(make, place)


def test_poses_do_not_depend_on_batching_or_sharding(make):
    P.shard_invariance_case(make, place)


def test_edge_shapes(make):
    P.edge_shapes_case(make, place)


def test_ragged_layout_equals_each_graph_alone(make):
    P.ragged_case(make, place)


def test_replicate_equals_collated_clones():
    P.replicate_equals_collate_case()


def test_replicated_batch_runs_through_the_models_like_collated_clones(make):
    P.replicate_through_models_case(make, place)


@pytest.mark.parametrize("crop,trajectory", [(None, False), (4.0, False), (None, True)])
def test_sample_poses_equals_sampling_bit_for_bit(make, crop, trajectory):
    P.sample_poses_case(make, place, crop=crop, trajectory=trajectory)


def test_sample_poses_confidence(make):
    P.confidence_case(make, place)


def test_errors(make):
    P.errors_case(make, place)


def test_randomize_cfg_mirror_matches_the_header():
    header = open(os.path.join(ROOT, "include", "ddmi.h")).read()
    body = re.search(r"typedef struct ddmi_randomize_cfg \{(.*?)\} ddmi_randomize_cfg;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
             "ptr": ctypes.c_void_p}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.+)$", decl)
        assert m, decl
        for name in (n.strip() for n in m.group(4).split(",")):
            fields.append((name, ctype["ptr" if m.group(3) else m.group(2)]))
    assert fields == list(L.RandomizeCfg._fields_)
    assert ctypes.sizeof(L.RandomizeCfg) == 72
    assert "ddmi_randomize_position" in L.EXPORTED_SYMBOLS
    assert re.search(r"int ddmi_randomize_position\(ddmi_model\* m, float\* lig_pos, const ddmi_randomize_cfg\* cfg, ddmi_stream stream\);", header)
