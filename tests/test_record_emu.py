"""The per-step record of the device loop on the CPU emulation build (tests/hipemu): the indexing of the record stores of
k_perturb, k_perturb_grouped and the conformer kernels at the shapes tests/test_gpu_record.py runs on the MI355X, and the ABI of
ddmi_sample_record.  Case bodies live in tests/record_cases.py."""
import ctypes
import os
import subprocess

import pytest

import diffdock_amd.lib as L
from diffdock_amd.model import MIScoreModel
from util import tables
import record_cases as R
from test_pack_emu import header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "hipemu", "libddmi_emu.so")


@pytest.fixture(scope="module")
def make():
    r = subprocess.run(["make", "-j8", "-C", os.path.join(ROOT, "diffdock_amd", "csrc"), "emu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def mk(cfg, sd):
        m = MIScoreModel(cfg, device="cpu", lib_path=EMU)
        m.load_state_dict(sd)
        m.set_tables(*tables())
        return m
    return mk


def place(x):
    return x


def test_uniform_batch_record_is_teacher_forced_exact(make):
    R.uniform_case(make, place)


def test_ragged_batch_record_equals_each_complex_alone(make):
    R.ragged_case(make, place)


def test_nan_counts_and_warnings(make, caplog):
    R.nan_case(make, place, caplog)


def test_record_arguments_are_checked(make):
    R.argument_case(make, place)


def test_sample_record_mirror_matches_the_header():
    ctype = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "ptr": ctypes.c_void_p}
    assert [(n, ctype[t]) for n, t in header_fields("ddmi_sample_record")] == list(L.SampleRecord._fields_)
    assert "ddmi_set_sample_record" in L.EXPORTED_SYMBOLS
