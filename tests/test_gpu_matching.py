"""Conformer matching on the MI355X: ddmi_match_conformer, MIScoreModel.match_conformer, diffdock_amd.matching and
io.complex_graph(conformers=...).  Case bodies live in tests/matching_cases.py (the emulator runs them in tests/test_matching_emu.py,
without the two quality cases)."""
import pytest
import torch

from diffdock_amd.model import MIScoreModel
from util import tables
import matching_cases as M

pytestmark = pytest.mark.gpu


def make(cfg, sd):
    assert torch.cuda.is_available(), "these tests need the MI355X (-m gpu)"
    m = MIScoreModel(cfg, device="cuda:0")     # raises DdmiError if libddmi.so is not built: no fallback
    m.load_state_dict(sd)
    m.set_tables(*tables())
    return m


def place(x):
    return x.to("cuda:0")


@pytest.mark.parametrize("n", M.OBJECTIVE_SHAPES)
def test_objective_matches_the_float64_restatement(n):
    M.objective_case(make, place, n)


@pytest.mark.parametrize("budget", [M.SMALL, M.ODD], ids=["popsize8", "popsize7"])
def test_results_do_not_depend_on_the_batch_and_repeat(budget):
    M.determinism_case(make, place, budget)


def test_edges():
    M.edges_case(make, place)


def test_errors():
    M.errors_case(make, place)


def test_quality_same_budget_against_the_host_route():
    M.quality_same_budget_case(make, place)


def test_quality_long_budget_against_the_host_route():
    M.quality_long_budget_case(make, place)


def test_tries_of_one_ligand_in_one_call():
    M.tries_case(make, place)


def test_complex_graph_with_conformers(tmp_path):
    M.complex_graph_case(make, place, tmp_path)
