"""Cases of the initial poses on the device (ddmi_randomize_position, HeteroBatch.replicate, sampling.sample_poses).  Run on the
CPU emulation build by tests/test_randpos_emu.py and on the MI355X by tests/test_gpu_randpos.py through the same C ABI.
`make(cfg, sd)` returns a loaded MIScoreModel, `place` moves a batch or tensor to the model's device.  References: the
reference-executed fixture tests/golden/randpos.pt, and synth.randomize_position (float64) fed the draws the kernel must have used.

Bounds: 5e-5 A on coordinates (what k_modify_conformer is held to against units.pt; a float32 restatement of the same
arithmetic is 9.5e-7 A from the fixture at coordinates up to 21 A), 1e-4 relative on confidence scores (the project's score bound);
everything that compares the device with itself is torch.equal."""
import argparse
import ctypes

import numpy as np
import torch

import diffdock_amd.lib as L
from diffdock_amd.config import TINY
from diffdock_amd.hetero import HeteroBatch
from diffdock_amd.sampling import crop_beyond, sample_poses, sampling
from diffdock_amd.synth import make_complex, randomize_position
from diffdock_amd.weights import init_state_dict
from oracle.conformer import get_t_schedule
from util import fixture_case, graph_from_dict, load_fixture, rel_err
from pack_cases import ragged_complexes

TOL = 5e-5
STEP = 0xFFFFFFFF   # step -1 as the unsigned counter word


def clones(g, n):
    return [g.clone() for _ in range(n)]


def model_for(make, cfg=TINY):
    return make(cfg, init_state_dict(cfg, seed=3))


# ------------------------------------------------------------------ the draws the kernel must have used
def philox_word0(m, seed, sample_ids, comps):
    """Output word 0 of the library's Philox block for counters (sample id, step -1, component), key = seed: [len(ids), len(comps)]."""
    ctr = np.array([[s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF, STEP, c] for s in sample_ids for c in comps], dtype=np.uint32)
    key = np.tile(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32), (len(ctr), 1))
    out = np.zeros((len(ctr), 4), dtype=np.uint32)
    L.check(m.lib, m.lib.ddmi_debug_philox(ctr.ctypes.data, key.ctypes.data, len(ctr), out.ctypes.data))
    return out[:, 0].reshape(len(sample_ids), len(comps)).astype(np.int64)


def normals(m, place, seed, sample_ids):
    """Components 0..6 at step -1 through ddmi_debug_normal: float64 [len(ids), 7]."""
    rows = []
    for s in sample_ids:
        out = place(torch.zeros(1, 7))
        L.check(m.lib, m.lib.ddmi_debug_normal(seed, s, 1, -1, 7, ctypes.c_void_p(out.data_ptr()), m._stream()))
        if out.device.type == "cuda":
            torch.cuda.synchronize()
        rows.append(out.cpu().double().numpy()[0])
    return np.stack(rows)


def restated_draws(m, place, seed, sample_ids, n_tor, rec_pos, tr_std, choose_residue=False):
    """The documented draw layout (include/ddmi.h) turned into angles, rotation matrices and translations on the host, float64."""
    z = normals(m, place, seed, sample_ids)
    rot = []
    for w, x, y, zz in z[:, :4] / np.linalg.norm(z[:, :4], axis=1, keepdims=True):
        rot.append(np.array([[1 - 2 * (y * y + zz * zz), 2 * (x * y - zz * w), 2 * (x * zz + y * w)],
                             [2 * (x * y + zz * w), 1 - 2 * (x * x + zz * zz), 2 * (y * zz - x * w)],
                             [2 * (x * zz - y * w), 2 * (y * zz + x * w), 1 - 2 * (x * x + y * y)]]))
    idx = None
    if choose_residue:
        idx = philox_word0(m, seed, sample_ids, [7])[:, 0] % rec_pos.shape[0]
        tr = rec_pos.double().numpy()[idx] + 0.01 * z[:, 4:7]
    else:
        tr = tr_std * z[:, 4:7]
    ang = np.zeros((len(sample_ids), 0))
    if n_tor:
        u = ((philox_word0(m, seed, sample_ids, [8 + j for j in range(n_tor)]) >> 8) + 0.5) / 2.0 ** 24
        ang = (2 * u - 1) * np.pi
    return dict(torsion=list(ang), rotation=rot, tr=[t.reshape(1, 3) for t in tr]), idx


def tr_std_of(g, prop, tr_sigma_max):
    if prop >= 0:
        return float(torch.sqrt(torch.mean(torch.sum(g["receptor"].pos ** 2, dim=1)))) * prop / 1.73
    return -prop * tr_sigma_max


def restated(g, draws, no_torsion=False, no_random=False):
    """synth.randomize_position in float64 arithmetic on clones of g with the given draws -> [n, Nl, 3] float64.  (The function
    rounds its result to float32: |error| <= 2^-24 * 32 A = 2e-6 A, inside TOL.)"""
    n = len(draws["rotation"])
    out = randomize_position(clones(g, n), no_torsion, no_random, 0.0, draws=draws)
    return torch.stack([d["ligand"].pos for d in out]).double()


def generator_case(make, place, g, seed, ids, prop, choose_residue=False, no_torsion=False, no_random=False, m=None):
    """Device poses with library draws against the float64 restatement fed the same draws.  Returns (device poses, draws, error)."""
    m = m or model_for(make)
    B, R = len(ids), int(g["ligand"].edge_mask.sum())
    batch = place(HeteroBatch.from_data_list(clones(g, B)))
    got = m.randomize_position(batch, no_torsion, no_random, TINY.tr_sigma_max, initial_noise_std_proportion=prop,
                               choose_residue=choose_residue, seed=seed, sample_ids=ids).cpu().reshape(B, -1, 3)
    draws, idx = restated_draws(m, place, seed, ids, 0 if no_torsion else R, g["receptor"].pos,
                                tr_std_of(g, prop, TINY.tr_sigma_max), choose_residue)
    want = restated(g, draws, no_torsion, no_random)
    err = (got.double() - want).abs().max().item()
    print(f"randomize_position generator path: B={B} Nl={got.shape[1]} R={R} prop={prop} choose_residue={choose_residue} "
          f"max |dev - f64| = {err:.3e} A")
    assert torch.isfinite(got).all()
    assert err < TOL, err
    return got, draws, idx


# ------------------------------------------------------------------ 1. reference-executed fixture
def fixture_case_injected(make, place):
    fx = load_fixture("randpos")
    m = model_for(make)
    worst = 0.0
    for tag, c in fx["cases"].items():
        batch = place(HeteroBatch.from_data_list([graph_from_dict(fx["graph"]) for _ in range(3)]))
        got = m.randomize_position(batch, False, False, fx["tr_sigma_max"], initial_noise_std_proportion=c["prop"],
                                   draws=c["draws"]).cpu().reshape(3, -1, 3)
        err = (got - c["pos"]).abs().max().item()
        print(f"randomize_position fixture '{tag}': max |dev - reference| = {err:.3e} A (max |coordinate| {c['pos'].abs().max():.1f})")
        assert err < TOL, (tag, err)
        worst = max(worst, err)
    return worst


# ------------------------------------------------------------------ 2. generator path
def generator_path_case(make, place):
    g = make_complex(seed=31, n_res=50, n_lig=16)
    R = int(g["ligand"].edge_mask.sum())
    assert R >= 2
    m = model_for(make)
    for prop in (1.46, -0.5):
        _, draws, _ = generator_case(make, place, g, seed=11, ids=[0, 1, 2, 3, 4], prop=prop, m=m)
        for a in draws["torsion"]:
            assert a.shape == (R,) and np.all(np.abs(a) < np.pi)
        for Rm in draws["rotation"]:
            assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-5 and abs(np.linalg.det(Rm) - 1) < 1e-5
    std = [tr_std_of(g, p, TINY.tr_sigma_max) for p in (1.46, -0.5)]
    assert abs(std[0] - std[1]) > 1.0     # the two formulas really give different translations here
    # choose_residue: a residue of the graph, translation = its position + 0.01 z
    got, draws, idx = generator_case(make, place, g, seed=11, ids=[0, 1, 2, 3, 4], prop=-0.5, choose_residue=True, m=m)
    assert np.all((idx >= 0) & (idx < 50)) and len(set(idx.tolist())) > 1
    centre = g["receptor"].pos.mean(0).double()
    for i in range(5):   # the pose's mean is centre + translation: it sits on the chosen residue (to the 0.01 A draw)
        assert (got[i].double().mean(0) - centre - g["receptor"].pos[idx[i]].double()).abs().max() < 0.1


# ------------------------------------------------------------------ 3. batch / shard invariance
def shard_invariance_case(make, place):
    g = make_complex(seed=31, n_res=50, n_lig=16)
    m = model_for(make)
    run = lambda ids, seed=7: m.randomize_position(place(HeteroBatch.from_data_list(clones(g, len(ids)))), False, False,
                                                   TINY.tr_sigma_max, seed=seed, sample_ids=ids).cpu().reshape(len(ids), -1, 3)
    whole = run([0, 1, 2, 3, 4])
    default_ids = m.randomize_position(place(HeteroBatch.from_data_list(clones(g, 5))), False, False, TINY.tr_sigma_max, seed=7)
    assert torch.equal(whole, default_ids.cpu().reshape(5, -1, 3))      # NULL sample ids = 0..B-1
    parts = torch.cat([run([0, 1]), run([2, 3]), run([4])])
    assert torch.equal(whole, parts)
    other = run([0, 1, 2, 3, 4], seed=8)
    for i in range(5):
        assert (whole[i] - other[i]).abs().max() > 1e-2, i
        for j in range(i):
            assert (whole[i] - whole[j]).abs().max() > 1e-2, (i, j)


# ------------------------------------------------------------------ 4. edge shapes
def edge_shapes_case(make, place):
    m = model_for(make)
    g = make_complex(seed=31, n_res=50, n_lig=16)
    # no rotatable bonds
    g0 = ragged_complexes()[0]
    assert int(g0["ligand"].edge_mask.sum()) == 0
    generator_case(make, place, g0, seed=3, ids=[5, 6], prop=-0.5, m=m)
    # no_torsion on a ligand with torsions: rigid
    got, _, _ = generator_case(make, place, g, seed=3, ids=[0, 1, 2], prop=-0.5, no_torsion=True, m=m)
    d0 = torch.cdist(g["ligand"].pos, g["ligand"].pos)
    for p in got:
        assert (torch.cdist(p, p) - d0).abs().max() < 1e-5
    flex, _, _ = generator_case(make, place, g, seed=3, ids=[0], prop=-0.5, m=m)
    assert (torch.cdist(flex[0], flex[0]) - d0).abs().max() > 1e-2    # with torsions the conformer does change
    # no_random: every pose's mean is the centre
    got, _, _ = generator_case(make, place, g, seed=3, ids=[0, 1, 2], prop=-0.5, no_random=True, m=m)
    centre = g["receptor"].pos.mean(0)
    for p in got:
        assert (p.mean(0) - centre).abs().max() < 1e-5
    # an explicit centre moves the pose with it
    batch = place(HeteroBatch.from_data_list(clones(g, 3)))
    shifted = m.randomize_position(batch, False, True, TINY.tr_sigma_max, center=centre + torch.tensor([1.0, -2.0, 3.0]),
                                   seed=3).cpu().reshape(3, -1, 3)
    assert (shifted - got - torch.tensor([1.0, -2.0, 3.0])).abs().max() < 1e-5
    # one graph
    generator_case(make, place, g, seed=3, ids=[9], prop=1.46, m=m)
    # a sample id above 2^32: the high counter word is used
    hi, _, _ = generator_case(make, place, g, seed=3, ids=[(1 << 32) + 9], prop=1.46, m=m)
    lo, _, _ = generator_case(make, place, g, seed=3, ids=[9], prop=1.46, m=m)
    assert (hi - lo).abs().max() > 1e-2
    # 70 atoms: the 64-stride atom loops take a second trip
    g70 = make_complex(seed=33, n_res=40, n_lig=70)
    assert int(g70["ligand"].edge_mask.sum()) > 0
    generator_case(make, place, g70, seed=3, ids=[0, 1], prop=-0.5, m=m)


# ------------------------------------------------------------------ 5. ragged layout
def ragged_case(make, place):
    gs = ragged_complexes()[:3]          # R_b = 0, 2, 5; 9, 13, 17 atoms
    m = model_for(make)
    ids = [4, 0, 7]
    centres = torch.stack([g["receptor"].pos.mean(0) + k for k, g in enumerate(gs)])
    batch = place(HeteroBatch.from_data_list([g.clone() for g in gs]))
    got = m.randomize_position(batch, False, False, TINY.tr_sigma_max, center=centres, seed=5, sample_ids=ids).cpu()
    assert m._layout == (3,)
    a = 0
    for b, g in enumerate(gs):
        n = g["ligand"].pos.shape[0]
        alone = m.randomize_position(place(HeteroBatch.from_data_list([g.clone()])), False, False, TINY.tr_sigma_max,
                                     center=centres[b], seed=5, sample_ids=[ids[b]]).cpu()
        assert torch.isfinite(alone).all() and torch.equal(got[a:a + n], alone), b
        a += n
    assert a == got.shape[0]
    # injected torsion angles are addressed per graph under the layout
    R = [int(g["ligand"].edge_mask.sum()) for g in gs]
    ang = [np.linspace(-1.0, 2.0, r) for r in R]
    inj = m.randomize_position(batch, False, True, TINY.tr_sigma_max, center=centres, seed=5, sample_ids=ids,
                               draws=dict(torsion=ang)).cpu()
    a = 0
    for b, g in enumerate(gs):
        n = g["ligand"].pos.shape[0]
        alone = m.randomize_position(place(HeteroBatch.from_data_list([g.clone()])), False, True, TINY.tr_sigma_max,
                                     center=centres[b], seed=5, sample_ids=[ids[b]], draws=dict(torsion=[ang[b]])).cpu()
        assert torch.equal(inj[a:a + n], alone), b
        a += n


# ------------------------------------------------------------------ 6. replicate
def assert_same(a, b, what):
    if torch.is_tensor(a) or torch.is_tensor(b):
        assert torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), what
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), what
        for k in a:
            assert_same(a[k], b[k], what + (k,))
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            assert_same(x, y, what + (i,))
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b), what
    else:
        assert a == b, what


def assert_batches_equal(got, want):
    assert type(got) is type(want)
    assert list(got._stores) == list(want._stores)
    for key in want._stores:
        assert list(got._stores[key].keys()) == list(want._stores[key].keys()), key
        for k in want._stores[key].keys():
            assert_same(got._stores[key][k], want._stores[key][k], (key, k))
    assert list(got._globals) == list(want._globals)
    for k in want._globals:
        assert_same(got._globals[k], want._globals[k], ("global", k))


def replicate_equals_collate_case():
    for g in (make_complex(seed=31, n_res=20, n_lig=9), make_complex(seed=32, n_res=12, n_lig=7, all_atoms=True, atoms_per_res=(2, 4))):
        for n in (1, 3):
            assert_batches_equal(HeteroBatch.replicate(g, n), HeteroBatch.from_data_list(clones(g, n)))
            assert_batches_equal(HeteroBatch.replicate(g, n, device="cpu"), HeteroBatch.from_data_list(clones(g, n)).to("cpu"))
    back = HeteroBatch.replicate(g, 2).to_data_list()
    assert torch.equal(back[1]["atom", "receptor"].edge_index, g["atom", "receptor"].edge_index)


def replicate_through_models_case(make, place):
    from util import set_times
    g = make_complex(seed=31, n_res=16, n_lig=9)
    dev = place(torch.zeros(1)).device
    ccfg = TINY.replace(confidence_mode=True)
    for cfg in (TINY, ccfg):
        m = make(cfg, init_state_dict(cfg, seed=3))
        a = set_times(HeteroBatch.replicate(g, 3, device=dev), 0.4, 0.4, 0.4)
        b = set_times(place(HeteroBatch.from_data_list(clones(g, 3))), 0.4, 0.4, 0.4)
        out_a, out_b = m(a), m(b)
        assert m._copies and m._keep["mask_rotate"] is not None
        for x, y in zip(out_a[:1] if cfg.confidence_mode else out_a[:3], out_b):
            assert torch.isfinite(x).all() and torch.equal(x, y)


# ------------------------------------------------------------------ 7. sample_poses = sampling()
def sample_poses_case(make, place, crop=None, trajectory=False, N=5, steps=4, seed=9):
    g = make_complex(seed=31, n_res=16, n_lig=9)
    m = model_for(make)
    margs = TINY.replace(crop_beyond=crop)
    dev = place(torch.zeros(1)).device
    s = get_t_schedule(steps)
    common = dict(model_args=margs, seed=seed, batch_size=2, no_final_step_noise=True, return_full_trajectory=trajectory)
    if trajectory:   # and a confidence model without a confidence graph: it scores the sampling batch at the last step's times
        common["confidence_model"] = model_for(make, TINY.replace(confidence_mode=True))
    got = sample_poses(g, N, m, steps, s, s, s, initial_noise_std_proportion=0.3, **common)
    # the same initial poses, written into N clones, through sampling()
    dl = clones(g, N)
    for lo in range(0, N, 2):
        b = min(2, N - lo)
        p0 = m.randomize_position(HeteroBatch.replicate(g, b, device=dev), margs.no_torsion, False, margs.tr_sigma_max,
                                  initial_noise_std_proportion=0.3, seed=seed, sample_ids=list(range(lo, lo + b))).cpu().reshape(b, -1, 3)
        for i in range(b):
            dl[lo + i]["ligand"].pos = p0[i]
    want = sampling(dl, m, steps, s, s, s, device=dev, **common)
    pos = torch.stack([d["ligand"].pos.cpu() for d in want[0]])
    assert (got[1] is None and want[1] is None) or trajectory
    assert got[0].shape == (N, 9, 3) and got[0].dtype == torch.float32 and got[0].device.type == dev.type
    assert torch.isfinite(got[0]).all() and torch.equal(got[0].cpu(), pos)
    if trajectory:
        assert got[1].shape[0] == N and torch.isfinite(got[1]).all() and torch.equal(got[1].cpu(), want[1].cpu())
        assert got[2].shape == (steps + 1, N, 9, 3) and torch.equal(got[2].cpu(), want[2].cpu())
        assert torch.equal(got[2][-1], got[0])
    assert (got[0].cpu() - torch.stack([d["ligand"].pos for d in clones(g, N)])).abs().max() > 1e-2
    return got


# ------------------------------------------------------------------ 8. confidence
def confidence_case(make, place, seed=1, cutoff=16.0):
    fs, cfg, data_list = fixture_case("tiny_l1")
    fc, ccfg, _ = fixture_case("tiny_conf_l2")
    g = data_list[0]
    score, conf_model = make(cfg, fs["state_dict"]), make(ccfg, fc["state_dict"])
    dev = place(torch.zeros(1)).device
    N, steps = 5, 2
    s = get_t_schedule(steps)
    common = dict(model_args=cfg, seed=seed, batch_size=2, no_final_step_noise=True, confidence_model=conf_model)
    kw = dict(initial_noise_std_proportion=0.2)

    def through_sampling(cargs, conf_graphs):
        """sampling() from the initial poses of model.randomize_position: the same final poses bit for bit (sample_poses_case)."""
        dl = clones(g, N)
        for lo in range(0, N, 2):
            b = min(2, N - lo)
            p0 = score.randomize_position(HeteroBatch.replicate(g, b, device=dev), cfg.no_torsion, False, cfg.tr_sigma_max,
                                          seed=seed, sample_ids=list(range(lo, lo + b)), **kw).cpu().reshape(b, -1, 3)
            for i in range(b):
                dl[lo + i]["ligand"].pos = p0[i]
        out, conf = sampling(dl, score, steps, s, s, s, device=dev, confidence_data_list=conf_graphs, confidence_model_args=cargs,
                             **common)
        return torch.stack([d["ligand"].pos.cpu() for d in out]), conf.cpu()
    # without a crop: equal to sampling()'s confidence on the same poses (sample_poses_case covers the run without a confidence graph)
    pos, conf = sample_poses(g, N, score, steps, s, s, s, confidence_graph=g, **common, **kw)
    assert conf.shape[0] == N and torch.isfinite(conf).all()
    ref_pos, ref_conf = through_sampling(None, clones(g, N))
    assert torch.equal(pos.cpu(), ref_pos) and torch.equal(conf.cpu(), ref_conf)
    # with a confidence crop: every pose keeps a residue, at least one loses some (checked with the host crop_beyond)
    kept = []
    for i in range(N):
        c = g.clone()
        c["ligand"].pos = pos[i].cpu()
        kept.append(int(crop_beyond(c, cutoff)["receptor"].pos.shape[0]))
    n_res = int(g["receptor"].pos.shape[0])
    assert min(kept) >= 1 and min(kept) < n_res, kept
    cargs = argparse.Namespace(crop_beyond=cutoff, all_atoms=False)
    pos3, conf3 = sample_poses(g, N, score, steps, s, s, s, confidence_graph=g, confidence_model_args=cargs, **common, **kw)
    ref_pos, ref_conf = through_sampling(cargs, clones(g, N))
    assert torch.equal(pos3.cpu(), ref_pos)
    err = rel_err(conf3.cpu(), ref_conf)
    print(f"sample_poses confidence under a {cutoff} A crop (kept residues {kept} of {n_res}): rel_err = {err:.3e}")
    assert err < 1e-4, err
    assert not torch.equal(conf3.cpu(), conf.cpu())      # the crop is really applied


# ------------------------------------------------------------------ 9. errors
def errors_case(make, place):
    import pytest
    m = model_for(make)
    g = make_complex(seed=31, n_res=20, n_lig=9)
    pos = place(torch.cat([g["ligand"].pos] * 3).clone())
    centre = np.zeros((3, 3), dtype=np.float32)

    def call(struct_size=None, center=centre):
        rc = L.RandomizeCfg()
        rc.struct_size = ctypes.sizeof(L.RandomizeCfg) if struct_size is None else struct_size
        rc.center = None if center is None else center.ctypes.data
        return m.lib.ddmi_randomize_position(m._h, ctypes.c_void_p(pos.data_ptr()), ctypes.byref(rc), m._stream())
    assert call() == -2                                          # no complex set
    batch = place(HeteroBatch.from_data_list(clones(g, 3)))
    m._ensure_complex(batch)
    assert call() == 0
    assert call(struct_size=ctypes.sizeof(L.RandomizeCfg) - 8) == -1
    assert call(center=None) == -1
    # a batch whose graphs differ, set by hand without the layout the wrapper adds
    gs = ragged_complexes()[:3]
    rb = place(HeteroBatch.from_data_list(gs))
    m._ensure_complex(rb)
    assert m._layout == (3,)
    c = m._keep
    cx = L.Complex()
    cx.num_graphs, cx.n_lig, cx.n_rec = 3, rb["ligand"].pos.shape[0], rb["receptor"].pos.shape[0]
    cx.n_bond_edges, cx.n_rec_edges = rb["ligand", "ligand"].edge_index.shape[1], rb["receptor", "receptor"].edge_index.shape[1]
    cx.n_tor = int(rb["ligand"].edge_mask.sum())
    for name in ("lig_ptr", "rec_ptr", "lig_x", "bond_index", "bond_attr", "edge_mask", "rec_x", "rec_pos", "rec_edge_index"):
        setattr(cx, name, c[name].data_ptr())
    assert m.lib.ddmi_set_complex(m._h, ctypes.byref(cx), m._stream()) == 0
    pos = rb["ligand"].pos.float().clone()
    assert call() == -2
    m.invalidate_complex()
    # rotatable bonds without a mask
    nomask = HeteroBatch.from_data_list(clones(g, 3))
    del nomask["ligand"].__dict__["mask_rotate"]
    with pytest.raises(L.DdmiError, match="mask_rotate"):
        m.randomize_position(place(nomask), False, False, 5.0)
    assert torch.isfinite(m.randomize_position(place(nomask), True, False, 5.0)).all()     # no_torsion needs none
    with pytest.raises(NotImplementedError, match="sampling"):
        sample_poses(g, 2, m, 1, [1.0], [1.0], [1.0], visualization_list=[])
