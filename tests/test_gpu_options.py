"""Model options at the DDL-synth widths on the MI355X against the float64 oracle (bodies: tests/option_cases.py).

Each option case runs on a 100-residue complex with a 40-atom ligand and one (tr, rot, tor) time per pose, asserts the
kernel route it was written for (k_conv_fused, the hidden-row route and the granule loops of every interaction layer) and
compares the scores with the float64 oracle at the default tolerances.  The smooth-edges and nv = 9 configurations also run
under the non-default exec routes that touch the edge weight or the granules; four options run a short device-loop trajectory.
Combinations the library refuses are asserted with their exact message."""
import pytest
import torch

import option_cases as oc
from diffdock_amd.model import MIScoreModel
from util import tables

pytestmark = pytest.mark.gpu


def gpu_model(cfg, sd):
    assert torch.cuda.is_available(), "these tests need an MI355X (pytest -m gpu)"
    m = MIScoreModel(cfg, device="cuda:0")     # raises DdmiError if libddmi.so is not built: no fallback
    m.load_state_dict(sd)
    m.set_tables(*tables())
    return m


def to_gpu(x):
    return x.to("cuda:0")


@pytest.fixture(scope="module")
def inputs():
    """Each option's inputs and float64 oracle outputs, computed once for the module."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = oc.option_inputs(name)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(oc.OPTIONS))
def test_option_at_width_matches_oracle(name, inputs, monkeypatch, capfd):
    oc.option_forward_case(gpu_model, to_gpu, monkeypatch.setenv, lambda: capfd.readouterr().err, inputs(name))


@pytest.mark.parametrize("name", list(oc.REFUSED))
def test_refused_option_combination(name):
    oc.refused_case(gpu_model, *oc.REFUSED[name])


ROUTES = [{"DDMI_FUSED_PACK": "0"}, {"DDMI_FUSED_DENSE": "0"}, {"DDMI_FUSED_PRERED": "0"}, {"DDMI_GROUPED": "2"},
          {"DDMI_NODE_UPDATE": "1"}]
ROUTE_CASES = [(n, e) for n in ("smooth_dyn", "nv9") for e in ROUTES]


@pytest.mark.parametrize("name,env", ROUTE_CASES, ids=[n + "-" + ",".join(f"{k[5:]}={v}" for k, v in e.items()) for n, e in ROUTE_CASES])
def test_option_under_exec_route_matches_oracle(name, env, inputs, monkeypatch, capfd):
    oc.option_forward_case(gpu_model, to_gpu, monkeypatch.setenv, lambda: capfd.readouterr().err, inputs(name), env)


@pytest.mark.parametrize("name", ["smooth_dyn", "smooth_static", "reduce_ps", "odd_parity", "nv9"])
def test_option_trajectory_matches_oracle(name, inputs):
    """4 steps of ddmi_sample (smooth_static: with the per-step crop of crop_beyond) against oracle.sampling."""
    inp = inputs(name)
    oc.trajectory_case(gpu_model, to_gpu, inp["cfg"], inp["sd"], inp["dl"])
