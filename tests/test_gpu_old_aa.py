"""The legacy all-atom class (AAOldModel, get_model(old=True) with all_atoms) on the MI355X.  Case bodies live in
tests/old_aa_cases.py; tests/test_old_aa_emu.py runs them on the CPU emulation build."""
import ctypes

import pytest
import torch

from diffdock_amd import lib as L
from diffdock_amd.model import MIScoreModel
from util import tables
import old_aa_cases as A

pytestmark = pytest.mark.gpu


def make(cfg, sd):
    assert torch.cuda.is_available(), "these tests need the MI355X (-m gpu)"
    m = MIScoreModel(cfg, device="cuda:0")     # raises DdmiError if libddmi.so is not built: no fallback
    m.load_state_dict(sd)
    m.set_tables(*tables())
    return m


def place(x):
    return x.to("cuda:0")


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_get_model_builds_the_legacy_all_atom_class():
    A.factory_case(None, "cuda:0")


@pytest.mark.parametrize("name", A.TINY_FIXTURES[:2] + A.TINY_FIXTURES[3:])
def test_matches_reference_fixture(name):
    A.fixture_parity_case(make, place, name)


def test_full_width_matches_reference_fixture():
    A.fixture_parity_case(make, place, "fwd_oldaa_full")


def test_pose_without_atoms_in_reach_takes_the_batchnorm_of_zero():
    A.far_pose_case(make, place)


def test_batch_of_one_pose():
    A.single_pose_case(make, place)


@pytest.mark.parametrize("name", ["tiny_oldaa_conf", "tiny_oldaa_score"])
def test_device_crop_equals_host_cropped_graphs(name):
    A.crop_case(make, place, name)


def test_reused_handle_equals_fresh_handles():
    A.reused_handle_case(make, place)


def test_sampling_scores_final_poses_with_the_legacy_all_atom_confidence_model():
    A.sampling_confidence_case(make, place)


def test_stepwise_loop_reaches_the_reference_trajectory():
    A.stepwise_loop_case(make, place)


def test_reduce_bn_sum_with_one_group_equals_reduce_bn_bit_for_bit():
    A.reduce_one_group_case(L.load(), place, stream())


def test_reduce_bn_sum_adds_three_separately_normalised_groups():
    A.reduce_three_groups_case(L.load(), place, stream())
