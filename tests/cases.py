"""Backend-independent parity cases, run by tests/test_emu_parity.py / tests/test_boundary.py on the CPU emulation build
and by the `-m gpu` tests on the MI355X through the same C ABI.  `make(cfg, sd)` returns a loaded MIScoreModel, `place`
moves a batch to the model's device."""
import copy
import math

import numpy as np
import pytest
import torch

from diffdock_amd.config import TINY
from diffdock_amd.hetero import HeteroBatch, set_time
from diffdock_amd.synth import make_complex, make_pose_list
from diffdock_amd.weights import init_state_dict
from oracle.conformer import get_t_schedule
from oracle.sampling import nan_guard, perturbations
from util import assert_scores_close, oracle_model, rel_err

TEMP = dict(temp_sampling=[1.17, 2.06, 7.04], temp_psi=[0.73, 0.90, 0.59], temp_sigma_data=[0.93, 0.75, 0.69])


def nan_guard_case(make, place, cfg=TINY):
    """utils/sampling.py:117-131 + :133-186 through ddmi_perturb: scores with NaN / +inf / -inf in some poses against the
    oracle's nan_guard + perturbations; a batch without a NaN mean must pass through the guard untouched (infinities too)."""
    sd = init_state_dict(cfg, seed=3)
    g = make_complex(seed=41, n_res=20, n_lig=9)
    B = 6
    dl = make_pose_list(g, B, tr_sigma_max=cfg.tr_sigma_max, seed=42)
    batch = place(HeteroBatch.from_data_list(dl))
    m = make(cfg, sd)
    R = int(dl[0]["ligand"].edge_mask.sum())
    steps = 5
    s = get_t_schedule(steps)
    gen = torch.Generator().manual_seed(8)
    noise = (torch.randn(steps, B, 3, generator=gen), torch.randn(steps, B, 3, generator=gen), torch.randn(steps, B * R, generator=gen))
    for variant in ("nan", "inf_only", "clean"):
        tr, rot, tor = torch.randn(B, 3, generator=gen), torch.randn(B, 3, generator=gen), torch.randn(B * R, generator=gen)
        if variant == "nan":
            tr[1, 0] = float("nan")
            tr[4] = float("nan")
            rot[1, 2] = float("nan")
            rot[2, 1] = float("inf")          # eps of rot becomes inf (nanmean keeps infinities), as in the reference
            tor[R] = float("nan")
            tor[2 * R + 1] = float("-inf")
        elif variant == "inf_only":           # the mean of pose 3 is inf, not NaN: the guard does not fire
            tr[3, 1] = float("inf")
        for k in (0, steps - 1):
            want_scores = nan_guard(tr.clone(), rot.clone(), tor.clone())
            want = perturbations(cfg, k, steps, (s, s, s), want_scores, (noise[0][k], noise[1][k], noise[2][k]),
                                 no_final_step_noise=True, **TEMP)
            got = m.perturb(batch, tr, rot, tor, k, steps, (s, s, s), noise=noise, no_final_step_noise=True, **TEMP)
            for a, b, name in zip(got, want, ("tr", "rot", "tor")):
                a, b = a.cpu().double(), b.double()
                assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b)), (variant, k, name)
                fin = torch.isfinite(b)
                assert torch.equal(torch.sign(a[~fin & ~torch.isnan(b)]), torch.sign(b[~fin & ~torch.isnan(b)]))
                assert (a[fin] - b[fin]).abs().max() <= 1e-6 * b[fin].abs().max(), (variant, k, name)
    # and inside the device loop: a NaN in the initial coordinates of one pose must not leak into the other poses
    dl2 = copy.deepcopy(dl)
    clean = m.sample_batch(place(HeteroBatch.from_data_list(dl2)), 2, (s[:2], s[:2], s[:2]), no_random=True).cpu().reshape(B, -1, 3)
    dl2[2]["ligand"].pos[0, 0] = float("nan")
    dirty = m.sample_batch(place(HeteroBatch.from_data_list(dl2)), 2, (s[:2], s[:2], s[:2]), no_random=True).cpu().reshape(B, -1, 3)
    keep = [i for i in range(B) if i != 2]
    assert torch.isfinite(dirty[keep]).all() and not torch.isfinite(dirty[2]).all()
    return clean, dirty


def neighbour_cap_case(make, place, cfg=TINY):
    """A compact 40-atom ligand: more than 32 atoms within lig_max_radius of most atoms and of every rotatable-bond
    midpoint, so the neighbour caps of radius_graph (32 + self, cg_model.py:477) and of the bond-graph radius search
    (32, cg_model.py:630) bind; which neighbours survive = first by ascending index (torch-cluster's device kernel)."""
    sd = init_state_dict(cfg, seed=5)
    g = make_complex(seed=51, n_res=24, n_lig=40)
    g["ligand"].pos = g["ligand"].pos * 0.33
    dl = make_pose_list(g, 2, tr_sigma_max=cfg.tr_sigma_max, seed=52, initial_noise_std_proportion=0.2)
    batch = HeteroBatch.from_data_list(dl)
    set_time(batch, 0.4, 0.4, 0.4, 2)
    pos = batch["ligand"].pos.reshape(2, 40, 3)
    within = (torch.cdist(pos, pos) < cfg.lig_max_radius).sum(-1)          # includes the atom itself
    assert int((within > 33).sum()) > 20, "the radius-graph cap must bind in this case"
    ref = oracle_model(cfg, sd)(batch, return_intermediates=True)
    m = make(cfg, sd)
    out = m(place(batch))
    assert int(m.debug_buffer("goff_ll")[-1]) == ref[4]["edge_counts"][0]
    n_bond = batch["ligand", "ligand"].edge_index.shape[1]
    uncapped = int((within - 1).sum()) + n_bond
    assert ref[4]["edge_counts"][0] < uncapped                             # edges were really dropped
    assert int(m.debug_buffer("tor_cnt").max()) == 32                      # bond-graph cap reached
    assert_scores_close(out[:3], ref[:3], what="neighbour caps")
    return out


def same_shape_complexes_case(make, place, cfg=TINY):
    """inference.py:224-303 reuses one model over many complexes.  Two DIFFERENT complexes with identical tensor shapes
    (same topology, other residue / atom / bond features), the second collated after the first batch was freed (the
    allocator may hand out the same addresses) and, separately, written INTO the storage of the live batch object: the
    scores must equal those of a fresh handle every time."""
    sd = init_state_dict(cfg, seed=9)
    ga = make_complex(seed=61, n_res=22, n_lig=11)
    other = make_complex(seed=62, n_res=22, n_lig=11)
    gb = ga.clone()
    gb["receptor"].x = other["receptor"].x.clone()
    gb["ligand"].x = ga["ligand"].x.flip(0).clone()
    gb["ligand", "ligand"].edge_attr = ga["ligand", "ligand"].edge_attr.roll(1, dims=1).clone()
    m = make(cfg, sd)

    def run(model, g):
        b = HeteroBatch.from_data_list(make_pose_list(g, 2, tr_sigma_max=cfg.tr_sigma_max, seed=1))
        set_time(b, 0.5, 0.5, 0.5, 2)
        b = place(b)
        return b, [o.cpu().clone() for o in model(b)[:3]]
    batch_a, out_a = run(m, ga)
    del batch_a
    batch_b, out_b = run(m, gb)
    _, fresh_b = run(make(cfg, sd), gb)
    assert all(torch.equal(x, y) for x, y in zip(out_b, fresh_b)), "stale ddmi_set_complex reused for a same-shaped complex"
    assert not torch.equal(out_a[0], out_b[0])
    # in-place overwrite of the static tensors of the live batch object (same object, same addresses)
    src = HeteroBatch.from_data_list(make_pose_list(ga, 2, tr_sigma_max=cfg.tr_sigma_max, seed=1))
    batch_b["receptor"].x.copy_(src["receptor"].x)
    batch_b["ligand"].x.copy_(src["ligand"].x)
    batch_b["ligand", "ligand"].edge_attr.copy_(src["ligand", "ligand"].edge_attr)
    again_a = [o.cpu() for o in m(batch_b)[:3]]
    assert all(torch.equal(x, y) for x, y in zip(again_a, out_a)), "in-place edit of the batch features went undetected"
    m.invalidate_complex()
    assert all(torch.equal(x.cpu(), y) for x, y in zip(m(batch_b)[:3], out_a))
    return out_a, out_b


def config0_case(make, place, cfg, tol_pos=2e-3, steps=4):
    """BASELINE configs[0]: the reference's example complex data/1a0q (416 residues / 23 heavy atoms, read by
    diffdock_amd.io -> tests/golden/1a0q_graph.pt), 4 inference steps x 2 samples: the device loop against the oracle's
    loop on the real geometry (language-model embeddings and RDKit atom features are external inputs: seeded stand-ins)."""
    from oracle.sampling import sampling as oracle_sampling
    from util import graph_from_dict, load_fixture, rmsd
    d = dict(load_fixture("1a0q_graph"))
    rng = np.random.default_rng(3)
    if cfg.lm_embedding_type:
        d["rec_x"] = torch.cat([d["rec_x"], torch.from_numpy((rng.normal(size=(416, cfg.lm_embedding_dim)) * 0.2).astype(np.float32))], 1)
    from diffdock_amd.config import LIG_FEATURE_DIMS
    feats = d["lig_x"].clone()
    for c in range(1, 16):
        feats[:, c] = torch.from_numpy(rng.integers(0, LIG_FEATURE_DIMS[c], size=23))
    d["lig_x"] = feats
    g = graph_from_dict(d)
    sd = init_state_dict(cfg, seed=17)
    B = 2
    dl = make_pose_list(g, B, tr_sigma_max=cfg.tr_sigma_max, seed=5, initial_noise_std_proportion=0.2)
    R = int(d["edge_mask"].sum())
    gen = torch.Generator().manual_seed(4)
    noise = (torch.randn(steps, B, 3, generator=gen), torch.randn(steps, B, 3, generator=gen), torch.randn(steps, B * R, generator=gen))
    s = get_t_schedule(steps)
    batch = HeteroBatch.from_data_list(dl)
    set_time(batch, s[0], s[0], s[0], B)
    om = oracle_model(cfg, sd)
    ref0 = om(batch)[:3]
    m = make(cfg, sd)
    assert_scores_close(m(place(batch))[:3], ref0, what="1a0q step 0")
    ref = oracle_sampling([x.clone() for x in dl], om, steps, cfg, noise, schedules=(s, s, s), batch_size=B,
                          no_final_step_noise=True, **TEMP)
    ref_pos = torch.stack([x["ligand"].pos for x in ref])
    pos = m.sample_batch(place(HeteroBatch.from_data_list(dl)), steps, (s, s, s), noise=noise, no_final_step_noise=True,
                         **TEMP).cpu().reshape(B, -1, 3)
    r = rmsd(pos, ref_pos)
    assert float(r.max()) < tol_pos, r
    return r


# ---- edge shapes and forced kernel routes (tests/test_emu_parity.py on the emulator, tests/test_gpu_edges.py on the MI355X) ----
# `setenv(name, value)` sets a DDMI_* route variable (monkeypatch.setenv): diffdock_amd/lib.py reads it when a
# model handle is created, so every handle below is made after its variables are set.  The reference is the float64 oracle.
F64 = torch.float64

def _synth(cfg, n_res, n_lig, B, seed, pose_seed, t, noise=0.3):
    from diffdock_amd.synth import make_pose_list as mpl
    g = make_complex(seed=seed, n_res=n_res, n_lig=n_lig, lm_dim=0)
    b = HeteroBatch.from_data_list(mpl(g, B, tr_sigma_max=cfg.tr_sigma_max, seed=pose_seed, initial_noise_std_proportion=noise))
    set_time(b, t, t, t, B)
    return b


def _ddl(**kw):
    from diffdock_amd.config import DDL_SYNTH
    base = dict(lm_embedding_type=None, dynamic_max_cross=False, cross_max_distance=80.0, tr_sigma_max=5.0)
    base.update(kw)
    return DDL_SYNTH.replace(**base)


def no_cross_edges_and_ragged_batch_case(make, place):
    """Edge cases the reference handles (with e3nn tensor products): a ligand out of cross-graph range (empty cross groups)
    and a batch of two DIFFERENT complexes (ragged sizes); then no cross edge in the whole batch."""
    cfg = TINY.replace(sh_lmax=2)
    sd = init_state_dict(cfg, seed=5)
    g1, g2 = make_complex(seed=11, n_res=24, n_lig=9), make_complex(seed=12, n_res=31, n_lig=13)
    g1["ligand"].pos = g1["ligand"].pos + torch.tensor([[500.0, 0.0, 0.0]])   # far away: no cross edges for graph 0
    for all_far in (False, True):
        if all_far:
            g2["ligand"].pos = g2["ligand"].pos + torch.tensor([[0.0, 700.0, 0.0]])    # now NO cross edges at all
        batch = HeteroBatch.from_data_list([g1, g2])
        set_time(batch, 0.4, 0.4, 0.4, 2)
        # (float32 oracle: the ligand 500 A away carries float32 coordinates, and on this input the float32 oracle itself is
        # 1.4e-4 of max|tr| away from the float64 one -- the input's rounding, shared by every float32 form)
        ref = oracle_model(cfg, sd)(batch, return_intermediates=True)
        m = make(cfg, sd)
        out = m(place(batch))
        n_cross = int(m.debug_buffer("offs_l")[-1])
        assert n_cross == ref[4]["edge_counts"][1] and (n_cross == 0) == all_far
        assert_scores_close(out[:3], ref[:3], what=f"no cross edges (all={all_far})")


def rigid_ligand_case(make, place, no_torsion):
    """cg_model.py:404: a ligand without rotatable bonds, or `no_torsion`, returns (tr, rot, empty(0), None); the device loop
    then runs the rigid-body update only (modify_conformer_batch with zero torsions)."""
    cfg = TINY.replace(no_torsion=no_torsion)
    sd = init_state_dict(cfg, seed=5)
    g = make_complex(seed=11, n_res=20, n_lig=8)
    if not no_torsion:
        g["ligand"].edge_mask = torch.zeros_like(g["ligand"].edge_mask)
        g["ligand"].mask_rotate = [g["ligand"].mask_rotate[0][:0]]
    dl = make_pose_list(g, 2, tr_sigma_max=cfg.tr_sigma_max, seed=3, no_torsion=no_torsion)
    b = HeteroBatch.from_data_list(dl)
    set_time(b, 0.5, 0.5, 0.5, 2)
    ref = oracle_model(cfg, sd, dtype=F64)(b)
    m = make(cfg, sd)
    tr, rot, tor, none = m(place(b))
    assert none is None and ref[3] is None and tor.shape == (0,) and ref[2].shape == (0,)
    assert_scores_close((tr, rot), ref[:2], what="rigid ligand")
    sched = get_t_schedule(3)
    start = b["ligand"].pos.cpu().clone()
    pos = m.sample_batch(place(b), 3, (sched, sched, sched), seed=1, no_final_step_noise=True).cpu()
    assert pos.shape == start.shape and torch.isfinite(pos).all()
    assert (pos - start).abs().max() > 1e-3                                 # the poses did move
    # rigid motion only: the intramolecular distances of every pose are those of the start conformer
    for k in range(2):
        a0, a1 = start.reshape(2, -1, 3)[k], pos.reshape(2, -1, 3)[k]
        assert (torch.cdist(a0, a0) - torch.cdist(a1, a1)).abs().max() < 1e-3


def degenerate_sizes_case(make, place, n_res, n_lig, B):
    """A batch of one pose, a 3-residue receptor (fewer neighbours than the 24-nearest graph asks for), a 2-atom ligand:
    forward against the oracle, and the device loop stays finite."""
    cfg = TINY
    sd = init_state_dict(cfg, seed=5)
    g = make_complex(seed=11, n_res=n_res, n_lig=n_lig)
    b = HeteroBatch.from_data_list(make_pose_list(g, B, tr_sigma_max=cfg.tr_sigma_max, seed=3))
    set_time(b, 0.5, 0.5, 0.5, B)
    ref = oracle_model(cfg, sd, dtype=F64)(b)
    m = make(cfg, sd)
    out = m(place(b))
    for o, r, name in zip(out[:3], ref[:3], ("tr", "rot", "tor")):
        assert o.shape == r.shape, name
        if r.numel():
            assert_scores_close((o,), (r,), names=(name,), what=f"{n_res}/{n_lig}/{B}")
    sched = get_t_schedule(3)
    pos = m.sample_batch(place(b), 3, (sched, sched, sched), seed=1, no_final_step_noise=True)
    assert pos.shape == b["ligand"].pos.shape and torch.isfinite(pos).all()


def fused_conv_full_width_case(make, place, setenv, lmax, edge_product="f32"):
    """DDL-synth channel widths (ns=48, nv=10) on a small complex: the statically-shaped main loop of k_conv_fused
    (chain shapes (12,3,3,3)/(3,3,3,3)/(12,-,-,-) and the packed 12|3x3 granule of the second layer), the generic variant at
    sh_lmax=2, receptor residues with more than 32 ligand neighbours (two virtual nodes per residue), against the oracle, with
    the dense-row and the sparse-row loop; at sh_lmax=1 also the merged first-layer granule against the separate granules."""
    cfg = _ddl(num_conv_layers=2, sh_lmax=lmax, edge_product=edge_product)
    sd = init_state_dict(cfg, seed=3)
    b = _synth(cfg, 12, 40, 2, seed=1, pose_seed=5, t=0.6)
    ref = oracle_model(cfg, sd, dtype=F64)(b)[:3]
    outs = {}
    for dense in ("1", "0"):          # dense-row and sparse-row loops (lmax 2: the generic, compiler-scheduled variant both times)
        setenv("DDMI_FUSED_DENSE", dense)
        m = make(cfg, sd)
        m.set_kernel_timing(True)
        outs[dense] = [o.cpu() for o in m(place(b))[:3]]
        assert "k_conv_fused" in m.kernel_timings()
        assert int(m.debug_buffer("vn_off_cross")[-1]) == 2 * b["receptor"].pos.shape[0]   # 40 neighbours -> 2 virtual nodes
        assert_scores_close(outs[dense], ref, what=f"dense={dense}")
    for a_, b_ in zip(outs["1"], outs["0"]):
        assert rel_err(a_, b_) < 1e-5
    if lmax == 1:   # the merged first-layer granule (three scalar channel tiles in one) against the separate granules
        setenv("DDMI_FUSED_TRI", "0")
        sep = [o.cpu() for o in make(cfg, sd)(place(b))[:3]]
        assert_scores_close(sep, ref, what="tri=0")
        for a_, b_ in zip(outs["0"], sep):
            assert rel_err(a_, b_) < 1e-5


def packing_dropped_case(make, place, setenv, ns, listing=None):
    """ns = 16 / 32 with nv = 10: the 4- / 8-step scalar chains are outside the static shape set, so every layer with a scalar
    input path runs the predicated kernel variant, which walks classic 4-slot granules only.  Such a layer must not contain a
    packed granule (round-3 defect: its slots 4..6 were dropped, 1 % error in the 1e block); packing on / off must agree.
    `listing()` (optional) returns the granule listing printed while a handle was created under DDMI_DEBUG_GRAN."""
    cfg = _ddl(ns=ns, nv=10, num_conv_layers=4)
    sd = init_state_dict(cfg, seed=3)
    b = _synth(cfg, 10, 12, 2, seed=1, pose_seed=5, t=0.6)
    ref = oracle_model(cfg, sd, dtype=F64)(b)[:3]
    outs = {}
    if listing is not None:
        setenv("DDMI_DEBUG_GRAN", "1")
        listing()
    for pack in ("1", "0"):
        setenv("DDMI_FUSED_PACK", pack)
        m = make(cfg, sd)
        if listing is not None:
            lines = [ln for ln in listing().splitlines() if ln.startswith("ddmi granules")]
            assert lines
            for line in lines:
                if "[shape 0 " in line:
                    assert not any(f"[shape {s} " in line for s in (4, 5, 6, 7)), line
        outs[pack] = [o.cpu() for o in m(place(b))[:3]]
        assert_scores_close(outs[pack], ref, what=f"pack={pack}")
        for o, r in zip(outs[pack], ref):
            assert rel_err(o, r) < 1e-5
    for a_, b_ in zip(outs["1"], outs["0"]):
        assert rel_err(a_, b_) < 1e-5


def shared_node_contraction_case(make, place, setenv, edge_product="f32"):
    """Shared-node tiles of k_conv_fused (MODE 4: the x tile holds the distinct gather nodes of the 16 virtual nodes, classic
    granules contract them on the 4x4x1 MFMA, packed granules read their rows through the slot map), forced onto EVERY edge
    group (DDMI_FUSED_SHARED=2 with dense rows): tiles with 16 distinct nodes (four passes), tiles that mix nodes with one and
    several virtual nodes, the bias row, against the oracle and against the per-virtual-node form."""
    cfg = _ddl(num_conv_layers=4, edge_product=edge_product)
    sd = init_state_dict(cfg, seed=3)
    b = _synth(cfg, 75, 7, 2, seed=2, pose_seed=5, t=0.6)     # 75 receptor neighbours per ligand atom: 32 + 32 + 11 edges
    ref = oracle_model(cfg, sd, dtype=F64)(b)[:3]
    setenv("DDMI_FUSED_DENSE", "2")
    outs = {}
    for shared in ("2", "1", "0"):
        setenv("DDMI_FUSED_SHARED", shared)
        m = make(cfg, sd)
        outs[shared] = [o.cpu() for o in m(place(b))[:3]]
        assert int(m.debug_buffer("vn_off_rl")[-1]) == 3 * b["ligand"].pos.shape[0]
        assert_scores_close(outs[shared], ref, what=f"shared={shared}")
    for k in ("2", "1"):
        for a_, b_ in zip(outs[k], outs["0"]):
            assert rel_err(a_, b_) < 1e-5


def in_tile_pre_reduction_case(make, place, setenv, edge_product="f32"):
    """lig<-rec group: the 16 residues of a tile send to the same <= 32 ligand atoms, so a tile sums its message rows per target in
    LDS (per wave, then the eight partial sums in wave order) and ONE row per (tile, target) leaves it; k_reduce_bn reads only the
    rows flagged live (tensor_layers.py:144,220-221: the scatter-mean itself is unchanged -- counts are the true edge counts).
    3 poses x 12 residues x 20 atoms: tiles 0 and 1 straddle two poses (targets span 40 rows: one row per edge as before), tile 2
    is pre-reduced.  Against the oracle and against the per-edge route (DDMI_FUSED_PRERED=0)."""
    cfg = _ddl(num_conv_layers=4, edge_product=edge_product)
    sd = init_state_dict(cfg, seed=3)
    b = _synth(cfg, 12, 20, 3, seed=1, pose_seed=5, t=0.6)
    ref = oracle_model(cfg, sd, dtype=F64)(b)[:3]
    outs = {}
    for pre in ("1", "0"):
        setenv("DDMI_FUSED_PRERED", pre)
        m = make(cfg, sd)
        outs[pre] = [o.cpu() for o in m(place(b))[:3]]
        if pre == "1":
            hdr = m.debug_buffer("prered_tile_hdr")
            assert hdr[:3, 0].tolist() == [0, 0, 1] and hdr[2, 1:3].tolist() == [40, 20]   # (mode, first target row, span)
            assert (hdr[2, 4:24] >= 0).all() and (hdr[2, 24:36] == -1).all()            # one message row per target of the tile
        assert_scores_close(outs[pre], ref, what=f"prered={pre}")
    for a_, b_ in zip(outs["1"], outs["0"]):
        assert rel_err(a_, b_) < 1e-5


def readout_tensor_product_forms_case(make, place, setenv, name):
    """final_conv / tor_bond_conv in the direct (per-edge-weight) form: the wave-per-item, thread-per-item and
    workgroup-per-edge kernels (k_readout.hip; picked by launch size in production, forced here) against the reference fixture."""
    from util import fixture_case
    fx, cfg, data_list = fixture_case(name)
    batch = HeteroBatch.from_data_list(data_list)
    set_time(batch, fx["t"], fx["t"], fx["t"], batch.num_graphs)
    ref = fx["forward"]
    for form in ("edge", "thread", "wave"):
        setenv("DDMI_TP_APPLY", form)
        tr, rot, tor, _ = make(cfg, fx["state_dict"])(place(batch))
        assert_scores_close((tr, rot, tor), (ref["tr"], ref["rot"], ref["tor"]), what=form)


def many_receptor_neighbours_case(make, place):
    """Ligand-gather groups through the fused kernel with several virtual nodes per ligand atom (70 receptor neighbours ->
    32 + 32 + 6 edges: the node term is repeated per virtual node, the last one is a sparse tile) at a width the MFMA first
    layer and the dense-row loop accept (ns = 16), against the oracle."""
    cfg = TINY.replace(ns=16, nv=4, sh_lmax=1, num_conv_layers=3, dynamic_max_cross=False, cross_max_distance=200.0,
                       lm_embedding_type=None)
    sd = init_state_dict(cfg, seed=9)
    g = make_complex(seed=21, n_res=70, n_lig=5, lm_dim=0)
    b = HeteroBatch.from_data_list(make_pose_list(g, 2, tr_sigma_max=cfg.tr_sigma_max, seed=4))
    set_time(b, 0.5, 0.5, 0.5, 2)
    ref = oracle_model(cfg, sd, dtype=F64)(b)[:3]
    m = make(cfg, sd)
    m.set_kernel_timing(True)
    out = m(place(b))[:3]
    assert "k_conv_fused" in m.kernel_timings()
    assert int(m.debug_buffer("vn_off_rl")[-1]) == 3 * b["ligand"].pos.shape[0]     # ceil(70 / 32) virtual nodes per ligand atom
    assert int(m.debug_buffer("vn_off_cross")[-1]) == b["receptor"].pos.shape[0]    # 5 ligand neighbours: one sparse tile each
    assert_scores_close(out, ref, what="many receptor neighbours")


def fused_node_update_case(make, place, modes=(1, 2), edge_product="f32"):
    """ddmi_exec_options.node_update = 1: k_node_update (a layer's node rows AND the next layer's per-node first-Linear terms P / Q in
    one kernel, the per-graph sigma terms of every layer from one batched launch) against k_reduce_bn + k_gemm_nt_batch launches:
    the node tables are the same sums in the same order -- layer 1's table, which no fused P / Q has touched yet, is bit-identical --
    and the scores agree at rounding level (P / Q take a 48-term fp32 sum in another order) and with the oracle.  With the per-step
    crop (its own reduce-group list), sidechain rows (the last layer reduces every row), a ragged batch of two complexes.
    node_update 2 / 3 force the workgroup shapes (sixteen nodes per workgroup / four waves per node)."""
    cfg = _ddl(num_conv_layers=3, tr_sigma_min=0.1, tr_sigma_max=0.5, sidechain_pred=True, edge_product=edge_product)
    sd = init_state_dict(cfg, seed=3)
    g1 = make_complex(seed=4, n_res=19, n_lig=10, lm_dim=0)
    g2 = make_complex(seed=5, n_res=13, n_lig=7, lm_dim=0)
    dl = make_pose_list(g1, 2, tr_sigma_max=5.0, seed=6, initial_noise_std_proportion=0.3) + make_pose_list(g2, 1, tr_sigma_max=5.0, seed=7, initial_noise_std_proportion=0.3)
    sched = get_t_schedule(1)
    res = {}
    for mode in (0,) + tuple(modes):
        m = make(cfg.replace(exec_options=(("node_update", mode),) if mode else ()), sd)
        b = HeteroBatch.from_data_list(dl)
        set_time(b, 0.6, 0.6, 0.6, b.num_graphs)
        m.set_kernel_timing(True)
        out = [o.cpu().clone() for o in m(place(b))]
        timers = m.kernel_timings()
        m.set_kernel_timing(False)
        x1 = torch.from_numpy(m.debug_buffer("x1").copy())
        cropped, traj = None, None
        if mode in (0, 1):
            m.set_crop_cutoff(6.0)
            cropped = [o.cpu().clone() for o in m(place(b))]
            m.set_crop_cutoff(None)
            traj = m.sample_batch(place(HeteroBatch.from_data_list(dl[:2])), 1, (sched, sched, sched), seed=11, sample_ids=[0, 1],
                                  no_final_step_noise=True).cpu().clone()
        res[mode] = (out, x1, cropped, traj, timers)
    # launches of the first-Linear GEMMs per forward: per layer and group before, the first layer's batch + the sigma batch now
    assert res[0][4]["conv_fc1_gemms"][1] > 2
    b = HeteroBatch.from_data_list(dl)
    set_time(b, 0.6, 0.6, 0.6, b.num_graphs)
    ref = oracle_model(cfg, sd, dtype=F64)(b)
    for mode in modes:
        assert res[mode][4]["conv_fc1_gemms"][1] == 2
        if mode != 1 and 1 in res:   # same sums, same MFMA chains whichever workgroup shape
            assert torch.equal(res[mode][0][0], res[1][0][0]) and torch.equal(res[mode][0][2], res[1][0][2]), mode
        assert torch.equal(res[mode][1], res[0][1])          # first interaction layer's node table
        for a_, b_ in zip(res[mode][0], res[0][0]):
            assert rel_err(a_, b_) < 1e-5
        if res[mode][2] is not None:
            for a_, b_ in zip(res[mode][2], res[0][2]):
                assert a_.shape == b_.shape and rel_err(a_, b_) < 1e-5
            assert (res[mode][3] - res[0][3]).abs().max() < 1e-4
        assert_scores_close(res[mode][0][:3], ref[:3], what=f"node_update={mode}")
    return res


def all_atom_ragged_batch_case(make, place):
    """AAModel on a batch of two DIFFERENT complexes (residue / atom / ligand counts differ), first with one ligand out of
    reach of every receptor atom, then with the ligand<->atom group completely empty (the reference's FasterTensorProduct
    cannot run that; sh_lmax = 2 can), against the oracle."""
    cfg = TINY.replace(all_atoms=True, sh_lmax=2, num_conv_layers=3, dynamic_max_cross=False, cross_max_distance=60.0)
    sd = init_state_dict(cfg, seed=2)
    g1 = make_complex(seed=31, n_res=14, n_lig=7, all_atoms=True, atoms_per_res=(2, 5))
    g2 = make_complex(seed=32, n_res=19, n_lig=11, all_atoms=True, atoms_per_res=(2, 5))
    d1 = make_pose_list(g1, 1, tr_sigma_max=5.0, seed=1, initial_noise_std_proportion=0.05)[0]
    d2 = make_pose_list(g2, 1, tr_sigma_max=5.0, seed=2, initial_noise_std_proportion=0.05)[0]
    d2["ligand"].pos = d2["ligand"].pos + torch.tensor([30.0, 0.0, 0.0])
    m = make(cfg, sd)
    for empty in (False, True):
        if empty:
            d1["ligand"].pos = d1["ligand"].pos + torch.tensor([0.0, 40.0, 0.0])
        batch = HeteroBatch.from_data_list([d1, d2])
        set_time(batch, 0.5, 0.5, 0.5, 2)
        ref = oracle_model(cfg, sd, dtype=F64)(batch, return_intermediates=True)
        assert (ref[4]["edge_counts"][2] == 0) == empty
        out = m(place(batch))
        assert int(m.debug_buffer("offs_la_l")[-1]) == ref[4]["edge_counts"][2]
        assert_scores_close(out[:3], ref[:3], what=f"all-atom ragged (empty={empty})")


def crop_with_embedding_layers_case(make, place):
    """crop_beyond + receptor embedding layers: the reference re-embeds the CROPPED receptor each step."""
    from oracle.sampling import sampling as oracle_sampling
    from util import fixture_case
    fx, cfg, data_list = fixture_case("tiny_l1_1group_emb")
    cfg = cfg.replace(crop_beyond=9.0)
    B, R = len(data_list), int(data_list[0]["ligand"].edge_mask.sum())
    g = torch.Generator().manual_seed(1)
    steps = 3
    noise = (torch.randn(steps, B, 3, generator=g), torch.randn(steps, B, 3, generator=g), torch.randn(steps, B * R, generator=g))
    ref = oracle_sampling([d.clone() for d in data_list], oracle_model(cfg, fx["state_dict"]), steps, cfg, noise,
                          batch_size=B, no_final_step_noise=True)
    ref = torch.stack([d["ligand"].pos for d in ref])
    m = make(cfg, fx["state_dict"])
    sched = get_t_schedule(steps)
    pos = m.sample_batch(place(HeteroBatch.from_data_list(data_list)), steps, (sched, sched, sched), noise=noise,
                         no_final_step_noise=True, crop_beyond=cfg.crop_beyond).cpu()
    keep = m.debug_buffer("crop_keep")
    assert 0 < keep.sum() < keep.size
    assert (pos.reshape(B, -1, 3) - ref).abs().max() < 2e-3


def sidechain_pred_under_crop_case(make, place):
    """sidechain_pred with crop_beyond: the reference crops the graph first and returns rows for the KEPT residues only
    (utils/utils.py:388-413, models/cg_model.py:397-402); the library's node table still holds every residue, so
    MIScoreModel.__call__ compacts the rows through the device's crop mask.  And ddmi_sidechain_pred belongs to the ddmi_forward
    directly before it: after a sampling loop on the same handle it raises instead of reading that pass's table."""
    from diffdock_amd import lib as _l
    from diffdock_amd.lib import DdmiError
    from oracle.sampling import crop_beyond
    from util import fixture_case
    fs, cfg, data_list = fixture_case("tiny_sidechain")
    m = make(cfg, fs["state_dict"])
    d = torch.cdist(data_list[0]["ligand"].pos, data_list[0]["receptor"].pos).min(0).values
    cutoff = float(d.sort().values[len(d) // 2]) + 1e-3      # about half of the residues of pose 0 survive
    cropped = [crop_beyond(copy.deepcopy(g), cutoff) for g in data_list]
    n_keep = sum(int(c["receptor"].pos.shape[0]) for c in cropped)
    assert 0 < n_keep < sum(int(g["receptor"].pos.shape[0]) for g in data_list)
    ob = HeteroBatch.from_data_list(cropped)
    set_time(ob, 0.4, 0.4, 0.4, ob.num_graphs)
    ref = oracle_model(cfg, fs["state_dict"], dtype=F64)(ob)
    batch = HeteroBatch.from_data_list(data_list)
    set_time(batch, 0.4, 0.4, 0.4, batch.num_graphs)
    m.set_crop_cutoff(cutoff)
    out = m(place(batch))
    m.set_crop_cutoff(None)
    assert out[3].shape == ref[3].shape == (n_keep, 10)
    assert_scores_close(out[:4], ref[:4], names=("tr", "rot", "tor", "sidechain"), what="sidechain under crop")
    # a sampling loop in between: the table of its last step is not what ddmi_sidechain_pred may read
    sched = get_t_schedule(2)
    m.sample_batch(place(batch), 2, (sched, sched, sched), seed=1, sample_ids=list(range(batch.num_graphs)), no_final_step_noise=True)
    side = place(torch.empty(int(batch["receptor"].pos.shape[0]), 10))
    with pytest.raises(DdmiError):
        _l.check(m.lib, m.lib.ddmi_sidechain_pred(m._h, side.data_ptr(), None))


# ---- one time per graph and per noise type (ddmi_forward's t_tr[B] / t_rot[B] / t_tor[B], ddmi_sample's three schedules) ----
# Under one shared t a quantity read for the wrong graph (time embedding, hidden-row bias W1e . sig, receptor sigma rows, dynamic
# cross cutoff, the score heads' sigma) or for the wrong noise type gives exactly the right answer; these cases give every pose
# its own three times, far apart and permuted differently, and compare with the float64 oracle.

MIXED_T = {"tr": (0.95, 0.4, 0.05), "rot": (0.3, 0.85, 0.6), "tor": (0.55, 0.1, 0.9)}
MIXED_T_DYN = {"tr": (0.95, 0.6, 0.05), "rot": (0.3, 0.85, 0.6), "tor": (0.55, 0.1, 0.9)}   # cutoffs 3 sigma_tr + 20: 64 / 27 / 20 A


def _times(times, B):
    return [list(times[k]) * (B // len(times[k])) for k in ("tr", "rot", "tor")]


def mixed_times_tile_case(make, place, n_res, n_lig, variant, dynamic=False):
    """Tiles that straddle the three poses of a batch (the B = 3 shapes of the tile-boundary sweep): scores and the x{l} node
    tables element-wise against the float64 oracle.  With dynamic_max_cross each pose has its own cross cutoff; the cutoffs
    and the cross-edge count of every pose are checked against the oracle's, and the case asserts that graph 0's cutoff would
    have given other counts."""
    from oracle.conformer import t_to_sigma
    from oracle.graph_ops import radius
    from util import elem_excess, set_times
    B = 3
    cfg = _ddl(num_conv_layers=4, dynamic_max_cross=dynamic, tr_sigma_max=19.0 if dynamic else 5.0, **variant)
    sd = init_state_dict(cfg, seed=7)
    g = make_complex(seed=100 + n_res, n_res=n_res, n_lig=n_lig, lm_dim=0)
    from diffdock_amd.synth import make_pose_list as mpl
    dl = mpl(g, B, tr_sigma_max=5.0, seed=n_lig, initial_noise_std_proportion=0.3)
    if dynamic:   # the synthetic pocket fits inside 20 A: move the ligands 18 A out, so each cutoff keeps another set of pairs
        for d in dl:
            d["ligand"].pos = d["ligand"].pos + torch.tensor([18.0, 0.0, 0.0])
    batch = HeteroBatch.from_data_list(dl)
    times = MIXED_T_DYN if dynamic else MIXED_T
    set_times(batch, *_times(times, B))
    tr, rot, tor, _, inter = oracle_model(cfg, sd, dtype=F64)(batch, return_intermediates=True)
    R = int(g["ligand"].edge_mask.sum())
    what = f"{n_res}/{n_lig}/{B}/{variant}/{'dynamic' if dynamic else 'static'}"
    if dynamic:   # the oracle's cutoffs and per-pose cross-edge counts (before the batch moves to the model's device)
        sig_tr = t_to_sigma(cfg, batch.complex_t["tr"], batch.complex_t["rot"], batch.complex_t["tor"])[0]
        cut = (3 * sig_tr + 20).double()
        lig, rec = batch["ligand"], batch["receptor"]
        lpos, rpos, lb, rb = lig.pos.double(), rec.pos.double(), lig.batch.clone(), rec.batch.clone()

        def per_graph(c):
            src = radius(rpos / c[rb].unsqueeze(1), lpos / c[lb].unsqueeze(1), 1, rb, lb, max_num_neighbors=10000)[0]
            return torch.bincount(lb[src], minlength=B).tolist()
        want = per_graph(cut)
        assert sum(want) == inter["edge_counts"][1]
        assert per_graph(cut[:1].expand(B)) != want, "graph 0's cutoff gives the same counts: the case does not bite"
    m = make(cfg, sd)
    out = m(place(batch))[:3]
    assert_scores_close(out[:2 + (R > 0)], (tr, rot, tor)[:2 + (R > 0)], what=what)
    assert int(m.debug_buffer("offs_l")[-1]) == inter["edge_counts"][1]
    if dynamic:
        assert torch.allclose(torch.from_numpy(m.debug_buffer("cross_cutoff")).double(), cut, rtol=1e-6), what
        offs = m.debug_buffer("offs_l")
        ptr = [b * n_lig for b in range(B + 1)]   # ligand atoms of pose b: rows ptr[b] .. ptr[b+1]
        got = [int(offs[ptr[b + 1]]) - int(offs[ptr[b]]) for b in range(B)]
        assert got == want, (what, got, want)
    for l in range(1, cfg.num_conv_layers):   # node tables after every layer that updates all rows
        ref = inter[f"node_attr{l}"]
        mine = torch.from_numpy(m.debug_buffer(f"x{l}"))[:ref.shape[0], :ref.shape[1]]
        assert rel_err(mine, ref) < 1e-4 and elem_excess(mine, ref) <= 1.0, (what, l, rel_err(mine, ref), elem_excess(mine, ref))


# discrete score-norm tables (utils/so3.py:89-93, utils/torus.py:79-83): log-sigma rounded to the nearest bin
SO3_LO, SO3_HI, SO3_N = math.log10(0.0005), math.log10(4.0), 2000
TOR_LO, TOR_HI, TOR_N = math.log(3e-3), math.log(2.0), 5000


def _ref_bin_position(cfg, t_rot, t_tor):
    """Pre-round table positions the way the reference computes them: sigma in float32 torch, then numpy float32 logs."""
    t_rot, t_tor = torch.as_tensor(t_rot, dtype=torch.float32), torch.as_tensor(t_tor, dtype=torch.float32)
    eps = (cfg.rot_sigma_min ** (1 - t_rot) * cfg.rot_sigma_max ** t_rot).numpy()
    sig = (cfg.tor_sigma_min ** (1 - t_tor) * cfg.tor_sigma_max ** t_tor).numpy()
    so3 = (np.log10(eps) - np.log10(0.0005)) / (np.log10(4) - np.log10(0.0005)) * SO3_N
    tor = (np.log(sig / np.pi) - np.log(3e-3)) / (np.log(2) - np.log(3e-3)) * TOR_N
    return np.asarray(so3, dtype=np.float64), np.asarray(tor, dtype=np.float64)


def _t_at(smin, smax, log_target, log_fn):
    """t with log(sigma(t)) = log_target, sigma(t) = smin^(1-t) smax^t."""
    return (log_target - log_fn(smin)) / (log_fn(smax) - log_fn(smin))


def score_norm_times(cfg, n_bins=16, deltas=(0.02, 0.002)):
    """Per-graph (t_rot, t_tor) whose reference table positions sit at k + 0.5 +- delta for bins k spread over the reachable
    range, plus t = 0 and t = 1."""
    lo_r = math.ceil((math.log10(cfg.rot_sigma_min) - SO3_LO) / (SO3_HI - SO3_LO) * SO3_N)
    hi_r = math.floor((math.log10(cfg.rot_sigma_max) - SO3_LO) / (SO3_HI - SO3_LO) * SO3_N) - 1
    lo_t = math.ceil((math.log(cfg.tor_sigma_min / math.pi) - TOR_LO) / (TOR_HI - TOR_LO) * TOR_N)
    hi_t = math.floor((math.log(cfg.tor_sigma_max / math.pi) - TOR_LO) / (TOR_HI - TOR_LO) * TOR_N) - 1
    kr = np.linspace(max(lo_r, 0), min(hi_r, SO3_N - 2), n_bins).astype(int)
    kt = np.linspace(max(lo_t, 0), min(hi_t, TOR_N - 1), n_bins).astype(int)
    t_rot, t_tor = [0.0, 1.0], [0.0, 1.0]
    for d in deltas:
        for sgn in (-1, 1):
            for a, b in zip(kr, kt[::-1]):
                pr = a + 0.5 + sgn * d
                pt = b + 0.5 + sgn * d
                t_rot.append(_t_at(cfg.rot_sigma_min, cfg.rot_sigma_max, SO3_LO + pr / SO3_N * (SO3_HI - SO3_LO), math.log10))
                t_tor.append(_t_at(cfg.tor_sigma_min / math.pi, cfg.tor_sigma_max / math.pi,
                                   TOR_LO + pt / TOR_N * (TOR_HI - TOR_LO), math.log))
    return t_rot, t_tor


def score_norm_bins_case(make, place, cfg, t_rot, t_tor, tie=1e-3):
    """One forward of a tiny complex with one (t_tr, t_rot, t_tor) per graph.  Graphs whose reference position lies within
    `tie` bins of a rounding boundary may take either neighbour and are reported; every other graph meets the element-wise
    bound against the float64 oracle, and where the so3 table holds NaN the kernel's rot score is NaN too."""
    from util import elem_excess, set_times
    B = len(t_rot)
    t_rot = np.clip(np.asarray(t_rot, dtype=np.float32), 0, 1)
    t_tor = np.clip(np.asarray(t_tor, dtype=np.float32), 0, 1)
    t_tr = np.linspace(0, 1, B, dtype=np.float32)[np.random.default_rng(0).permutation(B)]
    sd = init_state_dict(cfg, seed=5)
    g = make_complex(seed=61, n_res=14, n_lig=8, lm_dim=cfg.lm_embedding_dim)
    from diffdock_amd.synth import make_pose_list as mpl
    batch = HeteroBatch.from_data_list(mpl(g, B, tr_sigma_max=cfg.tr_sigma_max, seed=62, initial_noise_std_proportion=0.3))
    set_times(batch, t_tr, t_rot, t_tor)
    R = int(g["ligand"].edge_mask.sum())
    assert R > 0
    pos_r, pos_t = _ref_bin_position(cfg, t_rot, t_tor)
    near_r = np.abs(pos_r - np.floor(pos_r) - 0.5) < tie
    near_t = np.abs(pos_t - np.floor(pos_t) - 0.5) < tie
    if near_r.any() or near_t.any():
        print(f"score-norm bins: graphs within {tie} bin of a tie (either neighbour accepted): rot {np.flatnonzero(near_r).tolist()}"
              f" tor {np.flatnonzero(near_t).tolist()}")
    tr, rot, tor, _ = oracle_model(cfg, sd, dtype=F64)(batch)
    out = [o.cpu() for o in make(cfg, sd)(place(batch))[:3]]
    assert_scores_close(out[:1], (tr,), names=("tr",), what="score-norm bins")
    nan_ref = torch.isnan(rot).any(1)
    assert torch.equal(torch.isnan(out[1]).any(1), nan_ref), ("NaN rows of the so3 table", nan_ref.nonzero().flatten().tolist())
    ok_r = ~nan_ref & ~torch.from_numpy(near_r)
    assert elem_excess(out[1][ok_r], rot[ok_r]) <= 1.0, ("rot", elem_excess(out[1][ok_r], rot[ok_r]))
    ok_t = ~torch.from_numpy(np.repeat(near_t, R))
    assert elem_excess(out[2][ok_t], tor[ok_t]) <= 1.0, ("tor", elem_excess(out[2][ok_t], tor[ok_t]))
    return nan_ref


def crop_under_three_schedules_case(make, place, cfg=TINY):
    """A 3-step ddmi_sample with crop_beyond and three different schedules: the receptor mask the last step leaves in
    crop_keep is the oracle's crop at that step's 3 sigma_tr + crop_beyond (utils/sampling.py:104-109), around the ligand
    positions the oracle's own trajectory reached; with sigma_rot or sigma_tor another set of residues would be kept."""
    from oracle.conformer import t_to_sigma
    from oracle.sampling import sampling as oracle_sampling
    from diffdock_amd.synth import make_pose_list as mpl
    steps, B = 3, 2
    cfg = cfg.replace(crop_beyond=5.0)
    s = get_t_schedule(steps)
    scheds = (s, s ** 3, s ** 0.25)     # last step: t = 1/3, 0.037, 0.76 -> 3 sigma = 1.1, 0.1, 3.1 A
    sd = init_state_dict(cfg, seed=9)
    g = make_complex(seed=71, n_res=60, n_lig=10)
    dl = mpl(g, B, tr_sigma_max=cfg.tr_sigma_max, seed=72, initial_noise_std_proportion=0.3)
    R = int(g["ligand"].edge_mask.sum())
    gen = torch.Generator().manual_seed(3)
    noise = (torch.randn(steps, B, 3, generator=gen), torch.randn(steps, B, 3, generator=gen), torch.randn(steps, B * R, generator=gen))
    record = []
    oracle_sampling([d.clone() for d in dl], oracle_model(cfg, sd), steps, cfg, noise, scheds, batch_size=B,
                    no_final_step_noise=True, record=record)
    last = [r for r in record if r["t_idx"] == steps - 1][0]
    lig = last["pos_in"].double().reshape(B, -1, 3)
    rec = torch.stack([d["receptor"].pos for d in dl]).double()
    dmin = torch.cdist(rec, lig).min(-1).values.reshape(-1)     # [B * n_res]: each residue's distance to its pose's ligand
    sig = [float(x) for x in t_to_sigma(cfg, *(float(sc[steps - 1]) for sc in scheds))]
    cut = [3 * x + cfg.crop_beyond for x in sig]
    want = dmin < cut[0]
    assert not torch.equal(want, dmin < cut[1]) or not torch.equal(want, dmin < cut[2]), "sigma_rot / sigma_tor crop the same"
    m = make(cfg, sd)
    m.sample_batch(place(HeteroBatch.from_data_list(dl)), steps, scheds, noise=noise, no_final_step_noise=True,
                   crop_beyond=cfg.crop_beyond)
    keep = torch.from_numpy(np.asarray(m.debug_buffer("crop_keep"))).reshape(-1).bool()
    assert keep.shape == want.shape and 0 < int(want.sum()) < want.numel()
    firm = (dmin - cut[0]).abs() > 1e-2    # the two trajectories agree to ~1e-3 A; a residue on the cutoff may go either way
    assert torch.equal(keep[firm], want[firm]), (keep.nonzero().flatten().tolist(), want.nonzero().flatten().tolist())
    assert int(firm.sum()) >= want.numel() - 2


def all_atom_mixed_times_case(make, place):
    """AAModel at the DDL-synth widths with one time per graph and noise type (the 'atom' nodes carry node_t too)."""
    from diffdock_amd.synth import make_pose_list as mpl
    from util import elem_excess, set_times
    from diffdock_amd.config import DDL_SYNTH
    cfg = DDL_SYNTH.replace(all_atoms=True, num_conv_layers=4, lm_embedding_type=None)
    sd = init_state_dict(cfg, seed=77)
    g = make_complex(seed=12, n_res=60, n_lig=20, lm_dim=0, all_atoms=True)
    batch = HeteroBatch.from_data_list(mpl(g, 3, tr_sigma_max=cfg.tr_sigma_max, seed=13, initial_noise_std_proportion=0.05))
    set_times(batch, *_times(MIXED_T, 3))
    tr, rot, tor, _, inter = oracle_model(cfg, sd, dtype=F64)(batch, return_intermediates=True)
    m = make(cfg, sd)
    out = m(place(batch))[:3]
    assert inter["edge_counts"][2] > 0 and int(m.debug_buffer("offs_la_l")[-1]) == inter["edge_counts"][2]
    assert_scores_close(out, (tr, rot, tor), what="all-atom, per-graph times")
    for l in range(cfg.num_conv_layers - 1):   # all node rows: ligand, residues, atoms
        ref = inter[f"node_attr{l + 1}"]
        mine = torch.from_numpy(m.debug_buffer(f"x{l + 1}"))[:, :ref.shape[1]]
        assert rel_err(mine, ref) < 1e-4 and elem_excess(mine, ref) <= 1.0, (l, rel_err(mine, ref), elem_excess(mine, ref))


def clip_end_config():
    """sigma ranges that run past both ends of both tables (so3: log10 eps below log10 5e-4 and above log10 4; torus: sigma / pi
    below 3e-3 and above 2), with graphs in the NaN bins of the shipped so3 table (153-170, 261) and at t = 0 / 1."""
    cfg = TINY.replace(rot_sigma_min=1e-4, rot_sigma_max=6.0, tor_sigma_min=0.005, tor_sigma_max=8.0)
    t_rot, t_tor = score_norm_times(cfg, n_bins=12)
    for k in (153, 160, 170, 261):
        t_rot.append(_t_at(cfg.rot_sigma_min, cfg.rot_sigma_max, SO3_LO + k / SO3_N * (SO3_HI - SO3_LO), math.log10))
        t_tor.append(0.5)
    t_rot += [0.01, 0.99]
    t_tor += [0.99, 0.01]
    return cfg, t_rot, t_tor


def three_schedules_loops_case(make, place, device):
    """The reference trajectory of tiny_l1_mixt (tr, rot and tor schedules differ) through ddmi_sample's own step
    coefficients and through the host step_coefficients loop."""
    from diffdock_amd.sampling import sampling
    from util import fixture_case, fixture_schedules, split_draws
    fx, cfg, data_list = fixture_case("tiny_l1_mixt")
    s = fx["sampling"]
    B, R = len(data_list), int(data_list[0]["ligand"].edge_mask.sum())
    noise = split_draws(s["draws"], s["steps"], B, R)
    tr_s, rot_s, tor_s = fixture_schedules(s)
    assert not np.array_equal(tr_s, rot_s) and not np.array_equal(tr_s, tor_s) and not np.array_equal(rot_s, tor_s)
    for native in (True, False):
        m = make(cfg, fx["state_dict"])
        out, _ = sampling([d.clone() for d in data_list], m, s["steps"], tr_s, rot_s, tor_s, device, None, cfg, batch_size=8,
                          noise=noise, no_final_step_noise=True, native_loop=native, **s["temp"])
        final = torch.stack([d["ligand"].pos.cpu() for d in out])
        assert (final - s["final_pos"]).abs().max() < 2e-3, native
