"""ddmi_exec_options.rec_share on the MI355X at BASELINE configs[2] shapes (300 residues, 30 ligand atoms; 40 poses, and 5 = one GPU's
share of configs[3]): in the device step loop the first interaction layer computes the rec-rec messages of graph 0 only and the node
update reads them for every pose.  Same kernels and arguments as the full group, same summation order: the trajectories equal the
forced-off route bit for bit.  With the per-step receptor crop the route must not run.  `vn_off_rr0` (the graph-0 list) is zero until
the shared group has run: it tells which route ran."""
import pytest
import torch

from diffdock_amd.config import DDL_SYNTH
from diffdock_amd.hetero import HeteroBatch
from diffdock_amd.model import MIScoreModel
from diffdock_amd.synth import make_complex, make_pose_list
from diffdock_amd.weights import init_state_dict
from oracle.conformer import get_t_schedule
from util import tables

pytestmark = pytest.mark.gpu


def gpu_model(cfg, sd):
    assert torch.cuda.is_available(), "these tests need the MI355X (-m gpu)"
    m = MIScoreModel(cfg, device="cuda:0")     # raises DdmiError if libddmi.so is not built: no fallback
    m.load_state_dict(sd)
    m.set_tables(*tables())
    return m


@pytest.mark.parametrize("B", [40, 5])
def test_rec_share_is_bit_identical_at_full_size(B):
    sd = init_state_dict(DDL_SYNTH, seed=1234)
    g = make_complex(seed=4, n_res=300, n_lig=30)
    dl = make_pose_list(g, B, tr_sigma_max=DDL_SYNTH.tr_sigma_max, seed=5, initial_noise_std_proportion=0.6)
    sched = get_t_schedule(5)
    res = {}
    for share in (0, 1):
        m = gpu_model(DDL_SYNTH.replace(exec_options=(("rec_share", share),)), sd)
        run = lambda **kw: m.sample_batch(HeteroBatch.from_data_list(dl).to("cuda:0"), 5, (sched, sched, sched), seed=123,
                                          sample_ids=list(range(B)), no_final_step_noise=True, **kw).clone()
        crop = run(crop_beyond=20.0)
        assert not m.debug_buffer("vn_off_rr0").any(), share     # per-step crop: the full group
        full = run()
        voff = m.debug_buffer("vn_off_rr0")
        assert (voff[-1] > 0) == (share == 0), (share, voff[-1])   # the shared route ran exactly when it is on
        assert torch.isfinite(full).all()
        res[share] = (full, crop)
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
