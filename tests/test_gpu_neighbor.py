"""Neighbour lists on the MI355X: ddmi_neighbor_graph, MIScoreModel.neighbor_graph, diffdock_amd.io.neighbor_graph(model=...) and
complex_graph(all_atoms=True, model=...).  Case bodies live in tests/neighbor_cases.py (the emulator runs them in
tests/test_neighbor_emu.py)."""
import pytest
import torch

from diffdock_amd.model import MIScoreModel
from util import tables
import neighbor_cases as N

pytestmark = pytest.mark.gpu


def make(cfg, sd):
    assert torch.cuda.is_available(), "these tests need the MI355X (-m gpu)"
    m = MIScoreModel(cfg, device="cuda:0")     # raises DdmiError if libddmi.so is not built: no fallback
    m.load_state_dict(sd)
    m.set_tables(*tables())
    return m


def place(x):
    return x.to("cuda:0")


@pytest.mark.parametrize("name", list(N.INPUTS))
def test_1a0q_rows_equal_the_float64_oracle(name):
    N.exact_case(make, place, name)


@pytest.mark.parametrize("name", ["atoms_5_8", "atoms_5_uncapped"])
def test_1a0q_atom_graph_against_the_executed_reference(name):
    N.fixture_case(make, place, name)


@pytest.mark.parametrize("name", list(N.SHAPES))
def test_small_shapes(name):
    N.shape_case(make, place, name)


def test_rows_do_not_depend_on_the_other_sets():
    N.independence_case(make, place)


def test_abi_and_errors():
    N.abi_case(make, place)


def test_complex_graph_all_atoms_on_the_device_equals_the_host_path(tmp_path):
    N.end_to_end_case(make, place, tmp_path)
