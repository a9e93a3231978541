"""ddmi_exec_options.rec_share on the CPU emulation build (tests/hipemu): in the device step loop every pose of a batch of copies of
one complex has the same t, so the first interaction layer's rec-rec messages are the same for every graph; the library computes
them for graph 0 only and the node update reads graph 0's rows for every graph.  Same kernels, same arguments, same summation order:
trajectories are bit-identical to the forced-off route.  The shared list `vn_off_rr0` stays zero until the shared group has run."""
import os
import subprocess
from dataclasses import replace

import pytest
import torch

from diffdock_amd.config import DDL_SYNTH, TINY
from diffdock_amd.hetero import HeteroBatch, set_time
from diffdock_amd.lib import DdmiError
from diffdock_amd.model import MIScoreModel
from diffdock_amd.synth import make_complex, make_pose_list
from diffdock_amd.weights import init_state_dict
from oracle.conformer import get_t_schedule
from util import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "hipemu", "libddmi_emu.so")


@pytest.fixture(scope="module")
def emu_lib():
    r = subprocess.run(["make", "-j8", "-C", os.path.join(ROOT, "diffdock_amd", "csrc"), "emu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return EMU


def make_model(cfg, sd, lib, rec_share):
    m = MIScoreModel(cfg.replace(exec_options=(("rec_share", rec_share),)), device="cpu", lib_path=lib)
    m.load_state_dict(sd)
    m.set_tables(*tables())
    return m


def shared_list(m):
    return m.debug_buffer("vn_off_rr0")   # voff of the graph-0 rec-rec list: [residues of one copy + 1]


def poses(n):
    g = make_complex(seed=4, n_res=16, n_lig=10, lm_dim=0)
    return make_pose_list(g, n, tr_sigma_max=5.0, seed=6, initial_noise_std_proportion=0.3)


def sample(m, lst, steps, **kw):
    sched = get_t_schedule(steps)
    return m.sample_batch(HeteroBatch.from_data_list(lst), steps, (sched, sched, sched), seed=11, sample_ids=list(range(len(lst))),
                          no_final_step_noise=True, **kw).clone()


def test_rec_share_is_bit_identical_in_the_step_loop(emu_lib):
    """TINY (ns = 8: first-Linear GEMMs + k_edge_hidden), B = 3, 4 steps: shared against forced off, and the cases that must not share."""
    cfg = TINY.replace(lm_embedding_type=None)
    sd = init_state_dict(cfg, seed=3)
    dl = poses(3)
    auto, off = make_model(cfg, sd, emu_lib, 0), make_model(cfg, sd, emu_lib, 1)

    # ddmi_forward keeps t on the device: never shared
    b = HeteroBatch.from_data_list(dl)
    set_time(b, 0.6, 0.6, 0.6, 3)
    assert all(torch.equal(x, y) for x, y in zip(auto(b)[:3], off(b)[:3]))
    assert not shared_list(auto).any()

    ta, to = sample(auto, dl, 4), sample(off, dl, 4)
    assert torch.equal(ta, to)
    assert shared_list(auto)[-1] > 0          # the shared route ran
    assert not shared_list(off).any()         # rec_share = 1: never
    assert torch.isfinite(ta).all()

    # one residue of graph 1 moved: not a batch of copies, the full group runs
    moved = [d.clone() for d in dl]
    moved[1]["receptor"].pos[5, 0] += 0.25
    ma, mo = sample(auto, moved, 4), sample(off, moved, 4)
    assert torch.equal(ma, mo)
    assert not shared_list(auto).any()
    assert not torch.equal(ma, ta)

    # per-step receptor crop: the contact graph changes per step, the full group runs
    ca, co = sample(auto, dl, 4, crop_beyond=3.0), sample(off, dl, 4, crop_beyond=3.0)
    assert torch.equal(ca, co)
    assert not shared_list(auto).any()

    # one pose: nothing to share, no list
    assert torch.equal(sample(auto, dl[:1], 4), sample(off, dl[:1], 4))
    with pytest.raises(DdmiError):
        shared_list(auto)


def test_rec_share_with_fused_hidden_rows(emu_lib):
    """ns = 48 (k_edge_hidden_mm, the benchmark's route), B = 3, one step."""
    cfg = replace(DDL_SYNTH, num_conv_layers=3, lm_embedding_type=None, dynamic_max_cross=False, tr_sigma_max=5.0)
    sd = init_state_dict(cfg, seed=3)
    dl = poses(3)
    auto, off = make_model(cfg, sd, emu_lib, 0), make_model(cfg, sd, emu_lib, 1)
    assert torch.equal(sample(auto, dl, 1), sample(off, dl, 1))
    assert shared_list(auto)[-1] > 0
