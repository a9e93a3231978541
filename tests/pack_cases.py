"""Cases of the ragged step loop (ddmi_set_batch_layout, sampling.sample_complexes): batches that pack the poses of several
complexes.  Run on the CPU emulation build by tests/test_pack_emu.py and on the MI355X by tests/test_gpu_pack.py through the same
C ABI.  `make(cfg, sd)` returns a loaded MIScoreModel, `place` moves a batch to the model's device.  The references are the
oracle's single-complex functions applied to each graph (or each NaN-guard group) on its own."""
import numpy as np
import torch

from diffdock_amd.config import TINY
from diffdock_amd.hetero import HeteroBatch, set_time
from diffdock_amd.sampling import sample_complexes, sampling
from diffdock_amd.synth import make_complex, make_pose_list
from diffdock_amd.weights import init_state_dict
from oracle.conformer import get_t_schedule, modify_conformer_batch
from oracle.sampling import nan_guard, perturbations
from util import assert_scores_close, oracle_model

TEMP = dict(temp_sampling=[1.17, 2.06, 7.04], temp_psi=[0.73, 0.90, 0.59], temp_sigma_data=[0.93, 0.75, 0.69])


def with_torsions(g, r):
    """Keep the first r rotatable bonds of a synth complex (edge_mask and mask_rotate rows in edge order)."""
    em = g["ligand"].edge_mask.clone()
    idx = torch.nonzero(em).flatten()
    assert idx.numel() >= r, (g.name, idx.numel(), r)
    em[idx[r:]] = False
    g["ligand"].edge_mask = em
    g["ligand"].mask_rotate = [np.asarray(g["ligand"].mask_rotate[0])[:r]]
    return g


def ragged_complexes(all_atoms=False):
    """Three complexes with R_b = 0, 2, 5 and different atom counts, plus a fourth with the atom and torsion counts of the
    second but another molecule (other masks).  Receptor features with the ESM columns TINY reads."""
    kw = dict(all_atoms=all_atoms, atoms_per_res=(2, 5)) if all_atoms else {}
    gs = [with_torsions(make_complex(seed=71, n_res=18, n_lig=9, **kw), 0),
          with_torsions(make_complex(seed=72, n_res=22, n_lig=13, **kw), 2),
          with_torsions(make_complex(seed=76, n_res=26, n_lig=17, **kw), 5),
          with_torsions(make_complex(seed=75, n_res=20, n_lig=13, **kw), 2)]
    m1, m3 = np.asarray(gs[1]["ligand"].mask_rotate[0]), np.asarray(gs[3]["ligand"].mask_rotate[0])
    assert m1.shape == m3.shape and not np.array_equal(m1, m3)
    return gs


def rot_edges(g):
    return g["ligand", "ligand"].edge_index.T[g["ligand"].edge_mask]


def conformer_update_case(make, place):
    """ddmi_modify_conformer on one batch of four different ligands (R_b = 0, 2, 5, 2; two with equal counts and different
    masks) against oracle.conformer.modify_conformer_batch applied to each graph with its own mask."""
    sd = init_state_dict(TINY, seed=3)
    gs = [make_pose_list(g, 1, tr_sigma_max=TINY.tr_sigma_max, seed=5 + i, initial_noise_std_proportion=0.3)[0]
          for i, g in enumerate(ragged_complexes())]
    batch = HeteroBatch.from_data_list(gs)
    B = len(gs)
    gen = torch.Generator().manual_seed(17)
    tr, rot = torch.randn(B, 3, generator=gen), torch.randn(B, 3, generator=gen) * 0.7
    R = [int(g["ligand"].edge_mask.sum()) for g in gs]
    tor = torch.randn(sum(R), generator=gen)
    m = make(TINY, sd)
    got = m.modify_conformer_batch(batch["ligand"].pos, place(batch), tr, rot, tor).cpu()
    a = t = 0
    for b, g in enumerate(gs):
        n = g["ligand"].pos.shape[0]
        mask = torch.from_numpy(np.asarray(g["ligand"].mask_rotate[0]).astype(bool))
        want = modify_conformer_batch(g["ligand"].pos.double(), 1, rot_edges(g), mask, tr[b:b + 1].double(), rot[b:b + 1].double(),
                                      tor[t:t + R[b]].double()[None] if R[b] else None)
        err = (got[a:a + n].double() - want).abs().max().item()
        assert err < 5e-5, (b, R[b], err)
        a, t = a + n, t + R[b]
    # a ligand of the batch moved by another graph's mask would be off by whole angstroms: the two equal-count ligands really
    # need their own masks (graph 3 with graph 1's mask is far from the reference)
    g = gs[3]
    wrong = modify_conformer_batch(g["ligand"].pos.double(), 1, rot_edges(gs[1]), torch.from_numpy(np.asarray(gs[1]["ligand"].mask_rotate[0])),
                                   tr[3:4].double(), rot[3:4].double(), tor[t - R[3]:t].double()[None])
    assert (got[a - g["ligand"].pos.shape[0]:a].double() - wrong).abs().max() > 1e-2
    return got


def grouped_nan_guard_case(make, place, cfg=TINY):
    """ddmi_perturb with two NaN-guard groups (3 poses of one complex, 2 of another): NaN in group 1's scores.  Group 0 equals
    the NaN-free run bit for bit (its +inf torsion score stays: the guard does not fire for group 0); group 1 equals the
    oracle's nan_guard + perturbations applied to group 1 alone."""
    sd = init_state_dict(cfg, seed=3)
    c0, c1 = make_complex(seed=41, n_res=20, n_lig=9), make_complex(seed=43, n_res=24, n_lig=12)
    dl = make_pose_list(c0, 3, tr_sigma_max=cfg.tr_sigma_max, seed=42) + make_pose_list(c1, 2, tr_sigma_max=cfg.tr_sigma_max, seed=44)
    batch = place(HeteroBatch.from_data_list(dl))
    B = 5
    R0, R1 = int(c0["ligand"].edge_mask.sum()), int(c1["ligand"].edge_mask.sum())
    n0 = 3 * R0
    steps = 5
    s = get_t_schedule(steps)
    gen = torch.Generator().manual_seed(8)
    noise = (torch.randn(steps, B, 3, generator=gen), torch.randn(steps, B, 3, generator=gen),
             torch.randn(steps, 3 * R0 + 2 * R1, generator=gen))
    tr, rot, tor = torch.randn(B, 3, generator=gen), torch.randn(B, 3, generator=gen), torch.randn(3 * R0 + 2 * R1, generator=gen)
    tor[1] = float("inf")                      # group 0: left alone by group 1's guard
    dirty = (tr.clone(), rot.clone(), tor.clone())
    dirty[0][3, 1] = float("nan")
    dirty[1][4, 0] = float("nan")
    dirty[2][n0 + 1] = float("nan")
    m = make(cfg, sd)
    for k in (0, steps - 1):
        run = lambda sc: [x.cpu() for x in m.perturb(batch, *sc, k, steps, (s, s, s), noise=noise, no_final_step_noise=True,
                                                      groups=[3, 2], **TEMP)]
        clean, got = run((tr, rot, tor)), run(dirty)
        assert torch.equal(got[0][:3], clean[0][:3]) and torch.equal(got[1][:3], clean[1][:3]) and torch.equal(got[2][:n0], clean[2][:n0])
        assert torch.isinf(got[2][1])
        want = perturbations(cfg, k, steps, (s, s, s), nan_guard(dirty[0][3:].clone(), dirty[1][3:].clone(), dirty[2][n0:].clone()),
                             (noise[0][k, 3:], noise[1][k, 3:], noise[2][k, n0:]), no_final_step_noise=True, **TEMP)
        for a, b, name in zip((got[0][3:], got[1][3:], got[2][n0:]), want, ("tr", "rot", "tor")):
            a, b = a.double(), b.double()
            assert torch.isfinite(a).all() and torch.isfinite(b).all(), (k, name)
            assert (a - b).abs().max() <= 1e-6 * b.abs().max(), (k, name)
        # one group for the whole batch (one sampling() batch): eps = 0.01 nanmean|x| is then taken over all five poses
        whole = [x.cpu() for x in m.perturb(batch, *dirty, k, steps, (s, s, s), noise=noise, no_final_step_noise=True, **TEMP)]
        assert not torch.equal(whole[0][3:], got[0][3:])


def packed_run(make, place, cfg, complexes, n_poses, noise, crop, native_loop=True, steps=3, batch_size=2, max_batch_graphs=5, **kw):
    """sample_complexes over the complexes against sampling() of each complex alone (sample ids offset_k + i)."""
    sd = init_state_dict(cfg, seed=4)
    m = make(cfg, sd)
    margs = cfg.replace(crop_beyond=crop)
    s = get_t_schedule(steps)
    lists = [make_pose_list(c, n, tr_sigma_max=cfg.tr_sigma_max, seed=10 + k, initial_noise_std_proportion=0.4)
             for k, (c, n) in enumerate(zip(complexes, n_poses))]
    zs = None
    if noise:
        gen = torch.Generator().manual_seed(23)
        zs = [(torch.randn(steps, n, 3, generator=gen), torch.randn(steps, n, 3, generator=gen),
               torch.randn(steps, n * int(c["ligand"].edge_mask.sum()), generator=gen)) for c, n in zip(complexes, n_poses)]
    dev = place(torch.zeros(1)).device
    common = dict(model_args=margs, seed=7, no_final_step_noise=True, batch_size=batch_size, device=dev, **TEMP, **kw)
    packed = sample_complexes([[g.clone() for g in dl] for dl in lists], m, steps, s, s, s, noise=zs,
                              max_batch_graphs=max_batch_graphs, native_loop=native_loop, **common)
    offset = 0
    for k, dl in enumerate(lists):
        alone, _ = sampling([g.clone() for g in dl], m, steps, s, s, s, noise=None if zs is None else zs[k], sample_id_offset=offset,
                            **common)
        for i, (a, b) in enumerate(zip(packed[k][0], alone)):
            pa, pb = a["ligand"].pos.cpu(), b["ligand"].pos.cpu()
            assert torch.isfinite(pa).all()
            assert torch.equal(pa, pb), (k, i, (pa - pb).abs().max().item())
        offset += len(dl)
    return packed


def packed_equals_alone_case(make, place, all_atoms=False):
    """With fixed_center_conv and tile_per_pose = 1 each complex's final poses from sample_complexes are bit-identical to
    sampling() of that complex alone: library draws and injected noise, with and without the per-step crop (CG)."""
    cfg = TINY.replace(fixed_center_conv=True, exec_options=(("tile_per_pose", 1),))
    if all_atoms:
        cfg = cfg.replace(all_atoms=True, sh_lmax=2, num_conv_layers=3, dynamic_max_cross=False, cross_max_distance=60.0)
    gs = ragged_complexes(all_atoms=all_atoms)[1:]
    n_poses = [3, 2, 4]                      # chunks of 2: [2, 1] [2] [2, 2] -> device batches of <= 5 graphs: [2 1 2] [2 2]
    for noise in (False, True):
        for crop in ((None,) if all_atoms else (None, 4.0)):
            packed_run(make, place, cfg, gs, n_poses, noise, crop)


def default_route_case(make, place, n_res=(60, 90, 75, 110), n_lig=(14, 22, 18, 30), n_poses=10, steps=20):
    """DDL-synth width, 4 complexes x 10 poses in one packed batch with the default kernel routes: one-step scores against the
    float64 oracle per graph, the 20-step loop stays finite, and the step-wise loop equals the device loop."""
    from diffdock_amd.config import DDL_SYNTH
    cfg = DDL_SYNTH.replace(lm_embedding_type=None, tr_sigma_max=5.0)
    sd = init_state_dict(cfg, seed=1234)
    m = make(cfg, sd)
    complexes = [make_complex(seed=90 + k, n_res=r, n_lig=n, lm_dim=0) for k, (r, n) in enumerate(zip(n_res, n_lig))]
    lists = [make_pose_list(c, n_poses, tr_sigma_max=cfg.tr_sigma_max, seed=k, initial_noise_std_proportion=0.5)
             for k, c in enumerate(complexes)]
    graphs = [g for dl in lists for g in dl]
    batch = HeteroBatch.from_data_list(graphs)
    set_time(batch, 0.6, 0.6, 0.6, len(graphs))
    ref = oracle_model(cfg, sd, dtype=torch.float64)(batch)[:3]     # (before `place`, which may move the batch in place)
    out = [o.cpu() for o in m(place(batch))[:3]]
    a = t = 0
    for b, g in enumerate(graphs):
        r = int(g["ligand"].edge_mask.sum())
        assert_scores_close((out[0][b:b + 1], out[1][b:b + 1], out[2][t:t + r]), (ref[0][b:b + 1], ref[1][b:b + 1], ref[2][t:t + r]),
                            what=f"packed graph {b}")
        t += r
    s = get_t_schedule(steps)
    dev = place(torch.zeros(1)).device
    run = lambda native: sample_complexes([[g.clone() for g in dl] for dl in lists], m, steps, s, s, s, device=dev, seed=3,
                                          batch_size=10, max_batch_graphs=40, no_final_step_noise=True, native_loop=native,
                                          **TEMP)
    native, stepwise = run(True), run(False)
    for (dn, _), (ds, _) in zip(native, stepwise):
        for a_, b_ in zip(dn, ds):
            assert torch.isfinite(a_["ligand"].pos).all()
            assert torch.equal(a_["ligand"].pos.cpu(), b_["ligand"].pos.cpu())
    return native
