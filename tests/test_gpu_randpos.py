"""Initial poses on the MI355X: ddmi_randomize_position, HeteroBatch.replicate through the models, sampling.sample_poses.
Case bodies live in tests/randpos_cases.py (the emulator runs them in tests/test_randpos_emu.py)."""
import pytest
import torch

from diffdock_amd.model import MIScoreModel
from util import tables
import randpos_cases as P

pytestmark = pytest.mark.gpu


def make(cfg, sd):
    assert torch.cuda.is_available(), "these tests need the MI355X (-m gpu)"
    m = MIScoreModel(cfg, device="cuda:0")     # raises DdmiError if libddmi.so is not built: no fallback
    m.load_state_dict(sd)
    m.set_tables(*tables())
    return m


def place(x):
    return x.to("cuda:0")


def test_injected_draws_reproduce_the_reference_execution():
    P.fixture_case_injected(make, place)


def test_library_draws_match_the_float64_restatement():
    P.generator_path_case(make, place)


def test_poses_do_not_depend_on_batching_or_sharding():
    P.shard_invariance_case(make, place)


def test_edge_shapes():
    P.edge_shapes_case(make, place)


def test_ragged_layout_equals_each_graph_alone():
    P.ragged_case(make, place)


def test_replicated_batch_runs_through_the_models_like_collated_clones():
    P.replicate_through_models_case(make, place)


@pytest.mark.parametrize("crop,trajectory", [(None, False), (4.0, False), (None, True)])
def test_sample_poses_equals_sampling_bit_for_bit(crop, trajectory):
    P.sample_poses_case(make, place, crop=crop, trajectory=trajectory)


def test_sample_poses_confidence():
    P.confidence_case(make, place)


def test_errors():
    P.errors_case(make, place)
