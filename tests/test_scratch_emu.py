"""The handle's staged uploads and grow-only scratch on the CPU emulation build (tests/hipemu): ownership and sizes.  Case bodies live
in tests/scratch_cases.py; tests/test_gpu_scratch.py runs them on the MI355X, where the stagings' event waits matter."""
import os
import subprocess

import pytest

from diffdock_amd.model import MIScoreModel
from util import tables
import scratch_cases as S

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


def test_neighbor_table_and_scratch_grow_and_are_reused(make):
    S.neighbor_case(make, place)


def test_pose_metrics_and_fit_share_one_growing_scratch(make):
    S.metrics_case(make, place)


def test_matching_tables_grow_and_a_population_moves_into_the_scratch(make):
    S.matching_case(make, place)


def test_stagings_of_the_complex_are_replaced_with_it(make):
    S.complex_stagings_case(make, place)
