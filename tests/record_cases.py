"""Cases of the per-step record of the device loop (ddmi_set_sample_record, MIScoreModel.sample_batch(record=...)).  Run on the
MI355X by tests/test_gpu_record.py and on the CPU emulation build by tests/test_record_emu.py through the same C ABI.
`make(cfg, sd)` returns a loaded MIScoreModel, `place` moves a batch or tensor to the model's device.

The record makes TEACHER-FORCED checks of the loop possible: step k's scores are compared with the float64 oracle evaluated on the
poses the device loop itself had at step k (rec.pos[k - 1]), and step k's poses with the oracle's update of those poses by the
recorded scores -- no compounding drift, so the one-forward / one-update bounds of the suite apply to every step."""
import ctypes

import numpy as np
import torch

import diffdock_amd.lib as L
from diffdock_amd.config import TINY
from diffdock_amd.hetero import HeteroBatch, set_time
from diffdock_amd.synth import make_complex, make_pose_list
from diffdock_amd.weights import init_state_dict
from oracle.conformer import get_t_schedule, modify_conformer_batch
from oracle.sampling import nan_guard, perturbations, rot_edges_of
from util import assert_scores_close, fixture_case, graph_from_dict, oracle_model
import pack_cases as P

STEPS = 4
INVARIANT = dict(fixed_center_conv=True, exec_options=(("tile_per_pose", 1),))   # scores of a pose do not depend on its batch


def tiny_l1_inputs(B, steps=STEPS):
    """Weights and complex of the tiny_l1 fixture, B initial poses (the fixture's three, shifted a little more for every further
    pose) and injected draws; the first poses and draws are the same for every B."""
    fx, cfg, _ = fixture_case("tiny_l1")
    poses = [fx["poses"][p % 3] + 0.02 * (p // 3) for p in range(B)]
    dl = [graph_from_dict(fx["graph"], pos=p.clone()) for p in poses]
    R = int(dl[0]["ligand"].edge_mask.sum())
    gen = torch.Generator().manual_seed(31)
    z = torch.randn(steps, 128, 6 + R, generator=gen)[:, :B]
    noise = (z[..., :3].contiguous(), z[..., 3:6].contiguous(), z[..., 6:].reshape(steps, B * R).contiguous())
    return fx, cfg, dl, noise, fx["sampling"]["temp"]


def teacher_forced_checks(cfg, sd, dl, rec_pos, rec_scores, noise, temp, steps, poses):
    """For the poses `poses` of a batch of copies: every step's recorded scores against the float64 oracle on the recorded input
    poses (the suite's forward bounds: max-norm relative 1e-4, element-wise excess <= 1), and every step's recorded poses against
    the oracle's perturbations + modify_conformer_batch of the recorded input poses by the recorded scores (5e-5 Angstrom, the
    bound of the conformer-update parity tests)."""
    B, b = len(dl), len(poses)
    n = dl[0]["ligand"].pos.shape[0]
    R = int(dl[0]["ligand"].edge_mask.sum())
    s = get_t_schedule(steps)
    oracle = oracle_model(cfg, sd, dtype=torch.float64)
    pos_in = torch.stack([dl[p]["ligand"].pos for p in poses]).double()
    rec_pos = rec_pos.cpu().reshape(steps, B, n, 3)
    tr, rot, tor = (x.cpu() for x in rec_scores)
    tor = tor.reshape(steps, B, R)
    batch = HeteroBatch.from_data_list([dl[p].clone() for p in poses])
    rot_edges = rot_edges_of(batch, b)
    mask = torch.from_numpy(np.asarray(dl[0]["ligand"].mask_rotate[0]).astype(bool))
    for k in range(steps):
        batch["ligand"].pos = pos_in.reshape(b * n, 3).float()
        set_time(batch, s[k], s[k], s[k], b)
        want = oracle(batch)[:3]
        got = (tr[k, poses], rot[k, poses], tor[k, poses].reshape(-1))
        assert_scores_close(got, want, what=f"step {k}")
        zs = (noise[0][k, poses].double(), noise[1][k, poses].double(), noise[2][k].reshape(B, R)[poses].reshape(-1).double())
        trp, rotp, torp = perturbations(cfg, k, steps, (s, s, s), tuple(x.double() for x in got), zs, no_final_step_noise=True, **temp)
        want_pos = modify_conformer_batch(pos_in.reshape(b * n, 3), b, rot_edges, mask, trp, rotp, torp if R else None)
        err = (rec_pos[k, poses].double().reshape(b * n, 3) - want_pos).abs().max().item()
        assert err < 5e-5, (k, err)
        pos_in = rec_pos[k, poses].double()


def run_uniform(make, place, cfg, fx, dl, noise, temp, steps=STEPS, **kw):
    m = make(cfg, fx["state_dict"])
    batch = place(HeteroBatch.from_data_list([g.clone() for g in dl]))
    out = m.sample_batch(batch, steps, (get_t_schedule(steps),) * 3, noise=noise, no_final_step_noise=True, **temp, **kw)
    return m, batch, out


def uniform_case(make, place):
    """2 poses, 4 steps, injected noise: teacher-forced parity of every step; the record changes no pose; partial records."""
    fx, cfg, dl, noise, temp = tiny_l1_inputs(2)
    m, batch, (pos, rec) = run_uniform(make, place, cfg, fx, dl, noise, temp, record=True)
    assert rec.pos.shape == (STEPS, 24, 3) and rec.tr.shape == rec.rot.shape == (STEPS, 2, 3) and rec.tor.shape == (STEPS, 8)
    assert rec.nan_count.shape == (STEPS, 1) and rec.nan_count.dtype == torch.int32 and not rec.nan_count.any()
    teacher_forced_checks(cfg, fx["state_dict"], dl, rec.pos, (rec.tr, rec.rot, rec.tor), noise, temp, STEPS, [0, 1])
    assert torch.equal(rec.pos[-1], pos)
    sched = (get_t_schedule(STEPS),) * 3
    off = m.sample_batch(batch, STEPS, sched, noise=noise, no_final_step_noise=True, **temp)
    assert torch.is_tensor(off) and torch.equal(off, pos)                      # the return type without `record`, the same poses
    pos2, only = m.sample_batch(batch, STEPS, sched, noise=noise, no_final_step_noise=True, record={"pos"}, **temp)
    assert torch.equal(pos2, pos) and torch.equal(only.pos, rec.pos)
    assert only.tr is None and only.rot is None and only.tor is None and only.nan_count is None
    # rows >= inference_steps stay as they were: capacity_steps = steps + 2 through the C ABI, buffers pre-filled
    dev = pos.device
    fill = lambda *shape: torch.full(shape, -77.0, device=dev)
    bufs = dict(pos=fill(STEPS + 2, 24, 3), tr=fill(STEPS + 2, 2, 3), rot=fill(STEPS + 2, 2, 3), tor=fill(STEPS + 2, 8),
                nan_count=torch.full((STEPS + 2, 1), -77, dtype=torch.int32, device=dev))
    sc, keep = m._sample_cfg(STEPS, sched, noise, 0, None, False, False, True, temp["temp_sampling"], temp["temp_psi"],
                             temp["temp_sigma_data"], None)
    p3 = batch["ligand"].pos.clone()
    L.set_sample_record(m.lib, m._h, STEPS + 2, **bufs)
    try:
        L.check(m.lib, m.lib.ddmi_sample(m._h, ctypes.c_void_p(p3.data_ptr()), ctypes.byref(sc), m._stream()))
    finally:
        L.set_sample_record(m.lib, m._h, off=True)
    assert torch.equal(p3, pos)
    for name, t in bufs.items():
        assert torch.equal(t[:STEPS], getattr(rec, name)), name
        assert (t[STEPS:] == -77).all(), name
    return rec


def wide_case(make, place, B=90):
    """3 * B > the 256 threads of k_perturb: pose p's rows of the wide run equal, bit for bit, its rows of the 2-pose run (scores
    made batch-invariant by fixed_center_conv + tile_per_pose); teacher-forced parity of the first and the last pose.

    The read-out tensor product is chosen by launch size (launch_tp_apply: a wave per (edge, item) pair up to 32768 pairs, a
    workgroup per edge beyond), and the two forms sum in another order.  The torsion read-out of 90 poses is past that size and
    the one of 2 poses is not, so the form is pinned (tp_apply = 1, the wave form) for both runs: without it a torsion score
    of the wide run is one ulp off now and then, whatever the record does."""
    steps = 3
    fx, cfg, dl, noise, temp = tiny_l1_inputs(B, steps)
    cfg = cfg.replace(**dict(INVARIANT, exec_options=INVARIANT["exec_options"] + (("tp_apply", 1),)))
    R, n = 4, 12
    _, _, (pos, rec) = run_uniform(make, place, cfg, fx, dl, noise, temp, steps, record=True)
    z2 = (noise[0][:, :2].contiguous(), noise[1][:, :2].contiguous(), noise[2][:, :2 * R].contiguous())
    _, _, (pos_s, rec_s) = run_uniform(make, place, cfg, fx, dl[:2], z2, temp, steps, record=True)
    assert torch.equal(pos[:2 * n], pos_s)
    assert torch.equal(rec.pos[:, :2 * n], rec_s.pos) and torch.equal(rec.tr[:, :2], rec_s.tr)
    assert torch.equal(rec.rot[:, :2], rec_s.rot) and torch.equal(rec.tor[:, :2 * R], rec_s.tor)
    assert torch.equal(rec.pos[-1], pos) and not rec.nan_count.any()
    teacher_forced_checks(cfg, fx["state_dict"], dl, rec.pos, (rec.tr, rec.rot, rec.tor), noise, temp, steps, [0, B - 1])
    # the routes the library chooses by itself at this size (workgroup-per-edge read-out, dense tiles): teacher-forced parity
    # (fixed_center_conv stays: the oracle batch of poses 0 and B - 1 numbers its graphs 0 and 1)
    cfg_d = cfg.replace(exec_options=())
    _, _, (pos_d, rec_d) = run_uniform(make, place, cfg_d, fx, dl, noise, temp, steps, record=True)
    assert torch.equal(rec_d.pos[-1], pos_d) and not rec_d.nan_count.any()
    teacher_forced_checks(cfg_d, fx["state_dict"], dl, rec_d.pos, (rec_d.tr, rec_d.rot, rec_d.tor), noise, temp, steps, [0, B - 1])


def ragged_case(make, place):
    """Two complexes with different Nl and R (9 atoms / no torsion, 13 atoms / 2 torsions), 2 + 1 poses = two NaN-guard groups,
    3 steps, tile_per_pose = 1: every graph's slice of the record equals the record of its complex sampled alone."""
    steps = 3
    cfg = TINY.replace(**INVARIANT)
    sd = init_state_dict(cfg, seed=4)
    gs = P.ragged_complexes()[:2]
    n_poses = [2, 1]
    lists = [make_pose_list(c, k, tr_sigma_max=cfg.tr_sigma_max, seed=10 + i, initial_noise_std_proportion=0.4)
             for i, (c, k) in enumerate(zip(gs, n_poses))]
    m = make(cfg, sd)
    s = (get_t_schedule(steps),) * 3
    run = lambda graphs, ids, groups: m.sample_batch(place(HeteroBatch.from_data_list([g.clone() for g in graphs])), steps, s, seed=7,
                                                     sample_ids=ids, no_final_step_noise=True, groups=groups, record=True, **P.TEMP)
    pos, rec = run(lists[0] + lists[1], [0, 1, 2], n_poses)
    assert rec.nan_count.shape == (steps, 2) and not rec.nan_count.any()
    assert rec.pos.shape == (steps, 2 * 9 + 13, 3) and rec.tor.shape == (steps, 2)
    a = b = t = 0
    for k, dl in enumerate(lists):
        n, r = dl[0]["ligand"].pos.shape[0] * len(dl), int(dl[0]["ligand"].edge_mask.sum()) * len(dl)
        pos_k, rec_k = run(dl, list(range(b, b + len(dl))), None)
        assert torch.equal(pos[a:a + n], pos_k)
        assert torch.equal(rec.pos[:, a:a + n], rec_k.pos), k
        assert torch.equal(rec.tr[:, b:b + len(dl)], rec_k.tr) and torch.equal(rec.rot[:, b:b + len(dl)], rec_k.rot), k
        assert rec_k.tor.shape == (steps, r) and torch.equal(rec.tor[:, t:t + r], rec_k.tor), k
        a, b, t = a + n, b + len(dl), t + r
    assert rec.pos[-1].equal(pos)


def nan_case(make, place, caplog):
    """A NaN coordinate in one pose of group 1 of 2: the recorded counts equal those of the oracle loop run per group, and
    sampling() logs the reference's warning for every (step, batch) whose guard fired."""
    import logging
    from diffdock_amd.sampling import sampling
    steps, cfg = 3, TINY
    sd = init_state_dict(cfg, seed=3)
    g = make_complex(seed=41, n_res=20, n_lig=9)
    dl = make_pose_list(g, 4, tr_sigma_max=cfg.tr_sigma_max, seed=42)
    dl[3]["ligand"].pos[0, 0] = float("nan")
    s = get_t_schedule(steps)
    m = make(cfg, sd)
    _, rec = m.sample_batch(place(HeteroBatch.from_data_list([x.clone() for x in dl])), steps, (s, s, s), no_random=True,
                            groups=[2, 2], record={"nan"})
    # the oracle loop, one sampling() batch per group
    oracle = oracle_model(cfg, sd)
    mask = torch.from_numpy(np.asarray(dl[0]["ligand"].mask_rotate[0]).astype(bool))
    want = torch.zeros(steps, 2, dtype=torch.int32)
    for grp in range(2):
        batch = HeteroBatch.from_data_list([x.clone() for x in dl[2 * grp:2 * grp + 2]])
        rot_edges = rot_edges_of(batch, 2)
        for k in range(steps):
            set_time(batch, s[k], s[k], s[k], 2)
            tr, rot, tor = oracle(batch)[:3]
            want[k, grp] = int(torch.isnan(tr.mean(-1)).sum())
            trp, rotp, torp = perturbations(cfg, k, steps, (s, s, s), nan_guard(tr, rot, tor), (None, None, None), no_random=True)
            # (the oracle's Kabsch step is an SVD, which refuses non-finite input: a pose with a NaN coordinate is all NaN after
            # any rigid update -- its centre is NaN -- so it is set to NaN here and the finite poses are updated on their own)
            pos = batch["ligand"].pos.reshape(2, -1, 3)
            ok = torch.isfinite(pos).all(-1).all(-1)
            new = torch.full_like(pos, float("nan"))
            if ok.any():
                R_ = tor.numel() // 2
                new[ok] = modify_conformer_batch(pos[ok].reshape(-1, 3), int(ok.sum()), rot_edges, mask, trp[ok], rotp[ok],
                                                 torp.reshape(2, R_)[ok].reshape(-1) if R_ else None).reshape(-1, pos.shape[1], 3)
            batch["ligand"].pos = new.reshape(-1, 3)
    assert want[:, 1].tolist() == [1] * steps                # (the inputs do what the case is about)
    assert torch.equal(rec.nan_count.cpu(), want)
    assert not rec.nan_count[:, 0].any()
    dev = place(torch.zeros(1)).device
    with caplog.at_level(logging.WARNING, logger="diffdock_amd.sampling"):
        sampling([x.clone() for x in dl], m, steps, s, s, s, device=dev, no_random=True, batch_size=2)
    msgs = [r.getMessage() for r in caplog.records if r.name == "diffdock_amd.sampling"]
    assert msgs == [f"Complex {g.name} Batch 2 Inference Iteration {k}: 1 / 2 samples failed" for k in range(steps)]


def argument_case(make, place):
    """ddmi_set_sample_record / ddmi_sample error returns, and ddmi_set_complex clearing the record."""
    fx, cfg, dl, noise, temp = tiny_l1_inputs(2)
    m = make(cfg, fx["state_dict"])
    batch = place(HeteroBatch.from_data_list(dl))
    dev = batch["ligand"].pos.device
    buf = torch.full((STEPS, 24, 3), -77.0, device=dev)

    def record(struct_size=None, capacity=STEPS):
        r = L.SampleRecord(ctypes.sizeof(L.SampleRecord) if struct_size is None else struct_size, capacity, buf.data_ptr())
        return m.lib.ddmi_set_sample_record(m._h, ctypes.byref(r))
    assert ctypes.sizeof(L.SampleRecord) == 48
    assert record() == -2                                     # no complex yet: DDMI_ERR_STATE
    assert m.lib.ddmi_set_sample_record(m._h, None) == 0      # switching off is always fine
    m._ensure_complex(batch)
    assert record(struct_size=40) == -1 and record(capacity=0) == -1
    sched = (get_t_schedule(STEPS),) * 3
    sc, keep = m._sample_cfg(STEPS, sched, noise, 0, None, False, False, True, 1.0, 0.0, 0.5, None)
    pos = batch["ligand"].pos.clone()
    sample = lambda: m.lib.ddmi_sample(m._h, ctypes.c_void_p(pos.data_ptr()), ctypes.byref(sc), m._stream())
    assert record(capacity=STEPS - 1) == 0
    assert sample() == -1 and "capacity_steps" in m.lib.ddmi_last_error().decode()
    assert torch.equal(pos, batch["ligand"].pos) and (buf == -77).all()     # nothing was enqueued
    assert record() == 0 and sample() == 0
    assert not (buf == -77).any() and torch.equal(buf[-1], pos)
    # a new ddmi_set_complex clears the record: the next loop writes nothing into the old buffer
    buf.fill_(-77.0)
    m.invalidate_complex()
    m._ensure_complex(batch)
    assert sample() == 0
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert (buf == -77).all()
    # so does ddmi_set_batch_layout (G changes, and with it the row length of nan_count): here two NaN-guard groups
    assert record() == 0
    m._ensure_layout([1, 1])
    assert sample() == 0
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert (buf == -77).all()
