"""Model options at the DDL-synth widths on the CPU emulation build (tests/hipemu) against the float64 oracle.

tests/test_gpu_options.py runs the whole option matrix on the MI355X; here the smooth-edges (cosine weights under per-pose
cross cutoffs) and nv = 9 cases run with two interaction layers on a small complex, through the static loops of
k_conv_fused, with their route asserted.  The bodies live in tests/option_cases.py."""
import os
import subprocess

import pytest

import option_cases as oc
from diffdock_amd.model import MIScoreModel
from util import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "hipemu", "libddmi_emu.so")


@pytest.fixture(scope="module")
def emu_lib():
    r = subprocess.run(["make", "-j8", "-C", os.path.join(ROOT, "diffdock_amd", "csrc"), "emu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return EMU


def emu_model(emu_lib):
    def make(cfg, sd):
        m = MIScoreModel(cfg, device="cpu", lib_path=emu_lib)
        m.load_state_dict(sd)
        m.set_tables(*tables())
        return m
    return make


@pytest.mark.parametrize("name", ["smooth_dyn", "nv9"])
def test_option_at_width_matches_oracle(name, emu_lib, monkeypatch, capfd):
    inp = oc.option_inputs(name, n_res=16, n_lig=40, B=3, num_conv_layers=2)
    oc.option_forward_case(emu_model(emu_lib), lambda x: x, monkeypatch.setenv, lambda: capfd.readouterr().err, inp)
