"""The per-step record of the device loop on the MI355X (ddmi_set_sample_record, MIScoreModel.sample_batch(record=...)).
Case bodies live in tests/record_cases.py (the emulator runs the indexing cases in tests/test_record_emu.py)."""
import pytest
import torch

from diffdock_amd.model import MIScoreModel
from util import tables
import record_cases as R

pytestmark = pytest.mark.gpu


def make(cfg, sd):
    assert torch.cuda.is_available(), "these tests need the MI355X (-m gpu)"
    m = MIScoreModel(cfg, device="cuda:0")     # raises DdmiError if libddmi.so is not built: no fallback
    m.load_state_dict(sd)
    m.set_tables(*tables())
    return m


def place(x):
    return x.to("cuda:0")


def test_uniform_batch_record_is_teacher_forced_exact():
    R.uniform_case(make, place)


def test_wide_uniform_batch_record_rows():
    R.wide_case(make, place)


def test_ragged_batch_record_equals_each_complex_alone():
    R.ragged_case(make, place)


def test_nan_counts_and_warnings(caplog):
    R.nan_case(make, place, caplog)


def test_record_arguments_are_checked():
    R.argument_case(make, place)
