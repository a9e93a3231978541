"""The per-step receptor crop of the all-atom model on the CPU emulation build (tests/hipemu).  Case bodies live in
tests/aa_crop_cases.py; tests/test_gpu_aa_crop.py runs them on the MI355X, the width-48 case at its full size and the packed case
also with the library's own draws."""
import os
import subprocess

import pytest

from diffdock_amd.model import MIScoreModel
from util import tables
import aa_crop_cases as A

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


def test_forward_under_crop_cutoff(make):
    A.forward_case(make, place)


@pytest.mark.parametrize("tile_per_pose", [False, True], ids=["default", "tile_per_pose"])
def test_forward_under_crop_cutoff_at_the_ddl_width(make, tile_per_pose):
    A.width48_case(make, place, tile_per_pose, n_res=24, n_lig=10)


def test_embedding_layers_run_on_the_cropped_graph(make):
    A.embedding_layers_case(make, place)


def test_confidence_under_crop_cutoff(make):
    A.confidence_case(make, place)


def test_device_loop_crops_every_step(make):
    A.device_loop_case(make, place)


def test_packed_all_atom_complexes_under_crop_equal_sampling_alone(make):
    A.packed_case(make, place, noises=(True,))


def test_one_handle_toggles_the_crop(make):
    A.toggled_case(make, place)


def test_permuted_atom_residue_relation_is_refused_under_crop(make):
    A.refusal_case(make, place)


def test_cutoff_that_keeps_everything(make):
    A.everything_kept_case(make, place)
