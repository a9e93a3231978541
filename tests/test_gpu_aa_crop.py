"""The per-step receptor crop of the all-atom model on the MI355X.  Case bodies live in tests/aa_crop_cases.py;
tests/test_aa_crop_emu.py runs them on the CPU emulation build."""
import pytest
import torch

from diffdock_amd.model import MIScoreModel
from util import tables
import aa_crop_cases as A

pytestmark = pytest.mark.gpu


def make(cfg, sd):
    assert torch.cuda.is_available(), "these tests need the MI355X (-m gpu)"
    m = MIScoreModel(cfg, device="cuda:0")     # raises DdmiError if libddmi.so is not built: no fallback
    m.load_state_dict(sd)
    m.set_tables(*tables())
    return m


def place(x):
    return x.to("cuda:0")


def test_forward_under_crop_cutoff():
    A.forward_case(make, place)


@pytest.mark.parametrize("tile_per_pose", [False, True], ids=["default", "tile_per_pose"])
def test_forward_under_crop_cutoff_at_the_ddl_width(tile_per_pose):
    A.width48_case(make, place, tile_per_pose)


def test_embedding_layers_run_on_the_cropped_graph():
    A.embedding_layers_case(make, place)


def test_confidence_under_crop_cutoff():
    A.confidence_case(make, place)


def test_device_loop_crops_every_step():
    A.device_loop_case(make, place)


def test_packed_all_atom_complexes_under_crop_equal_sampling_alone():
    A.packed_case(make, place)


def test_one_handle_toggles_the_crop():
    A.toggled_case(make, place)


def test_permuted_atom_residue_relation_is_refused_under_crop():
    A.refusal_case(make, place)


def test_cutoff_that_keeps_everything():
    A.everything_kept_case(make, place)
