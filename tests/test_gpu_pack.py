"""The ragged step loop on the MI355X: batches that pack the poses of several complexes (ddmi_set_batch_layout,
sampling.sample_complexes).  Case bodies live in tests/pack_cases.py (the emulator runs them in tests/test_pack_emu.py)."""
import pytest
import torch

from diffdock_amd.model import MIScoreModel
from util import tables
import pack_cases as P

pytestmark = pytest.mark.gpu


def make(cfg, sd):
    assert torch.cuda.is_available(), "these tests need the MI355X (-m gpu)"
    m = MIScoreModel(cfg, device="cuda:0")     # raises DdmiError if libddmi.so is not built: no fallback
    m.load_state_dict(sd)
    m.set_tables(*tables())
    return m


def place(x):
    return x.to("cuda:0")


def test_ragged_conformer_update_matches_oracle_per_graph():
    P.conformer_update_case(make, place)


def test_nan_guard_runs_per_group():
    P.grouped_nan_guard_case(make, place)


@pytest.mark.parametrize("all_atoms", [False, True])
def test_packed_complexes_equal_sampling_alone(all_atoms):
    P.packed_equals_alone_case(make, place, all_atoms=all_atoms)


def test_packed_batch_on_the_default_routes():
    """DDL-synth width, 4 complexes x 10 poses: scores per graph against the float64 oracle, 20 finite steps, step-wise = device loop."""
    P.default_route_case(make, place)
