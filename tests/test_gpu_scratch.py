"""The handle's staged uploads and grow-only scratch on the MI355X: a staging buffer is refilled only after the previous upload has
left it, buffers grow under work in flight, and the stagings of a complex go with it.  Case bodies live in tests/scratch_cases.py
(the emulator runs them in tests/test_scratch_emu.py)."""
import pytest
import torch

from diffdock_amd.model import MIScoreModel
from util import tables
import scratch_cases as S

pytestmark = pytest.mark.gpu


def make(cfg, sd):
    assert torch.cuda.is_available(), "these tests need the MI355X (-m gpu)"
    m = MIScoreModel(cfg, device="cuda:0")     # raises DdmiError if libddmi.so is not built: no fallback
    m.load_state_dict(sd)
    m.set_tables(*tables())
    return m


def place(x):
    return x.to("cuda:0")


def test_neighbor_table_and_scratch_grow_and_are_reused():
    S.neighbor_case(make, place)


def test_pose_metrics_and_fit_share_one_growing_scratch():
    S.metrics_case(make, place)


def test_matching_tables_grow_and_a_population_moves_into_the_scratch():
    S.matching_case(make, place)


def test_stagings_of_the_complex_are_replaced_with_it():
    S.complex_stagings_case(make, place)
