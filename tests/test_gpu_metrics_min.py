"""The minimised symmetric RMSD and the fitting transform on the MI355X: ddmi_pose_fit, MIScoreModel.pose_fit,
diffdock_amd.metrics.evaluate_poses(minimize=True) and superpose.  Case bodies live in tests/metrics_min_cases.py (the emulator runs
them in tests/test_metrics_min_emu.py)."""
import pytest
import torch

from diffdock_amd.model import MIScoreModel
from util import tables
import metrics_min_cases as M

pytestmark = pytest.mark.gpu


def make(cfg, sd):
    assert torch.cuda.is_available(), "these tests need the MI355X (-m gpu)"
    m = MIScoreModel(cfg, device="cuda:0")     # raises DdmiError if libddmi.so is not built: no fallback
    m.load_state_dict(sd)
    m.set_tables(*tables())
    return m


def place(x):
    return x.to("cuda:0")


@pytest.mark.parametrize("name", ["1a0q", "sym576"])
def test_fixture_molecules_match_the_executed_spyrmsd(name):
    M.fixture_case(make, place, name)


@pytest.mark.parametrize("name", ["1a0q", "sym576"])
def test_rigid_copies_match_the_executed_spyrmsd(name):
    M.rigid_case(make, place, name)


@pytest.mark.parametrize("name", M.SMALL_SETS)
def test_small_sets_match_the_executed_spyrmsd(name):
    M.small_set_case(make, place, name)


@pytest.mark.parametrize("shape", M.EDGE_SHAPES)
def test_edge_shapes(shape):
    M.edge_shape_case(make, place, shape)


def test_values_do_not_depend_on_the_other_poses_references_or_permutations():
    M.independence_case(make, place)


def test_evaluate_poses_minimize_and_superpose():
    M.evaluate_case(make, place)


def test_errors():
    M.errors_case(make, place)


def test_recorded_trajectory_through_pose_fit():
    M.recorded_trajectory_case(make, place)
