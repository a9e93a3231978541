"""The legacy all-atom class (AAOldModel, get_model(old=True) with all_atoms) on the CPU emulation build (tests/hipemu).  Case bodies
live in tests/old_aa_cases.py; tests/test_gpu_old_aa.py runs them on the MI355X."""
import os
import subprocess

import pytest

from diffdock_amd import lib as L
from diffdock_amd.model import MIScoreModel
from util import tables
import old_aa_cases as A

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


def test_get_model_builds_the_legacy_all_atom_class(make):
    A.factory_case(EMU, "cpu")


@pytest.mark.parametrize("name", A.TINY_FIXTURES[:2] + A.TINY_FIXTURES[3:] + ["fwd_oldaa_full"])
def test_matches_reference_fixture(make, name):
    A.fixture_parity_case(make, place, name)


def test_pose_without_atoms_in_reach_takes_the_batchnorm_of_zero(make):
    A.far_pose_case(make, place)


def test_batch_of_one_pose(make):
    A.single_pose_case(make, place)


@pytest.mark.parametrize("name", ["tiny_oldaa_conf", "tiny_oldaa_score"])
def test_device_crop_equals_host_cropped_graphs(make, name):
    A.crop_case(make, place, name)


def test_reused_handle_equals_fresh_handles(make):
    A.reused_handle_case(make, place)


def test_sampling_scores_final_poses_with_the_legacy_all_atom_confidence_model(make):
    A.sampling_confidence_case(make, place)


def test_stepwise_loop_reaches_the_reference_trajectory(make):
    A.stepwise_loop_case(make, place)


def test_reduce_bn_sum_with_one_group_equals_reduce_bn_bit_for_bit(make):
    A.reduce_one_group_case(L.load(EMU), place)


def test_reduce_bn_sum_adds_three_separately_normalised_groups(make):
    A.reduce_three_groups_case(L.load(EMU), place)
