"""Cases of the pose metrics on the device (ddmi_pose_metrics, MIScoreModel.pose_metrics, diffdock_amd.metrics).  Run on the CPU
emulation build by tests/test_metrics_emu.py and on the MI355X by tests/test_gpu_metrics.py through the same C ABI.
`make(cfg, sd)` returns a loaded MIScoreModel, `place` moves a tensor to the model's device.

References: tests/golden/pose_metrics.pt, whose isomorphisms and symmetry-corrected RMSDs come from EXECUTING the reference's
vendored spyrmsd (tests/golden/make_golden_metrics.py), and `restated` below: the formulas of include/ddmi.h and the one-liners of
evaluate.py:481, :486, :503-505 in float64 on the same float32 inputs.

Bound: TOL = 1e-5 relative on every distance, derived and not measured: the sum of a (pose, reference, permutation) is at most
ceil(m / 64) + 6 float32 additions of squares of once-rounded differences of identical float32 inputs, a relative error below 1e-6
for m <= 128 (the fixture: a float32 restatement is within 1.6e-7 of float64), so 1e-5 leaves a factor of ten; the 2049-atom case
of the in-place path has 39 additions per sum, 39 * 2^-24 = 2.3e-6.  The centroid distance is a norm of mean DIFFERENCES in the kernel
(no cancellation of 30 A coordinates) and holds the same bound on these inputs, where it is 0.1 A and more.  Indices are judged
through values: the float64 value of the reported (k, s) must be within TOL of the float64 minimum (the fixture's smallest relative
gap between the best and the second-best triple is 1.2e-3).  Everything that compares the device with itself is torch.equal."""
import ctypes

import numpy as np
import pytest
import torch

import diffdock_amd.lib as L
from diffdock_amd.config import TINY
from diffdock_amd.metrics import Isomorphisms, evaluate_poses, isomorphisms
from diffdock_amd.weights import init_state_dict
from util import load_fixture

TOL = 1e-5
DIST = ("rmsd", "rmsd_plain", "centroid_distance", "min_self_distance", "min_point_distance")
_models = {}


def model_for(make):
    """One handle per runner: ddmi_pose_metrics needs no complex, weights or tables, any model serves."""
    if make not in _models:
        _models[make] = make(TINY, init_state_dict(TINY, seed=3))
    return _models[make]


def fixture():
    if "fx" not in _models:
        _models["fx"] = load_fixture("pose_metrics")
    return _models["fx"]


# ------------------------------------------------------------------ float64 restatement
def triple_sums(pos, ref, perm=None, atom_index=None):
    """sum_j |ref[k, perm[s, j]] - pos[p, atom_index[j]]|^2 in float64 -> [P, K, S]."""
    pos, ref = np.asarray(pos, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    x = pos if atom_index is None else pos[:, np.asarray(atom_index)]
    perm = np.arange(ref.shape[1])[None] if perm is None else np.asarray(perm)
    out = np.empty((x.shape[0], ref.shape[0], perm.shape[0]))
    for k in range(ref.shape[0]):
        out[:, k] = ((ref[k][perm][None] - x[:, None]) ** 2).sum(-1).sum(-1)
    return out


def restated(pos, ref, perm=None, atom_index=None, points=None):
    pos, ref = np.asarray(pos, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    x = pos if atom_index is None else pos[:, np.asarray(atom_index)]
    m = x.shape[1]
    sums = triple_sums(pos, ref, perm, atom_index)
    per_ref = np.sqrt(sums.min(-1) / m)
    out = dict(sums=sums, rmsd_per_ref=per_ref, rmsd=per_ref.min(-1))
    out["rmsd_plain"] = np.sqrt(((x[None] - ref[:, None]) ** 2).sum(axis=3).mean(axis=2)).min(0)                       # evaluate.py:481, :484
    out["centroid_distance"] = np.min(np.linalg.norm(x.mean(axis=1)[None, :] - ref.mean(axis=1)[:, None], axis=2), axis=0)   # :486
    d = np.linalg.norm(x[:, :, None, :] - x[:, None, :, :], axis=-1)                                                 # :503-505
    d = np.where(np.eye(m), np.inf, d)
    out["min_self_distance"] = np.min(d, axis=(1, 2))
    if points is None or len(points) == 0:
        out["min_point_distance"] = np.full(x.shape[0], np.inf)
    else:
        q = np.asarray(points, dtype=np.float64)
        out["min_point_distance"] = np.linalg.norm(x[:, :, None, :] - q[None, None], axis=-1).min(axis=(1, 2))
    return out


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both_inf = np.isinf(got) & np.isinf(want) & (got == want)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(got - want) / np.abs(want)
    e = np.where(both_inf, 0.0, e)
    return float(np.max(np.where(np.isnan(e), np.inf, e))) if e.size else 0.0


def check(tag, out, want, per_ref=True):
    """Every distance within TOL of the float64 restatement; the reported (k, s) through its float64 value."""
    worst = {}
    for name in DIST + (("rmsd_per_ref",) if per_ref else ()):
        got = out[name].cpu().numpy()
        assert got.shape == want[name].shape and got.dtype == np.float32, (tag, name, got.shape, want[name].shape)
        worst[name] = rel(got, want[name])
    best = out["best"].cpu().numpy()
    P, K, S = want["sums"].shape
    assert best.shape == (P, 2) and best.dtype == np.int32
    assert ((best[:, 0] >= 0) & (best[:, 0] < K) & (best[:, 1] >= 0) & (best[:, 1] < S)).all(), (tag, best)
    at_best = want["sums"][np.arange(P), best[:, 0], best[:, 1]]
    worst["best"] = rel(at_best, want["sums"].reshape(P, -1).min(-1))
    print(f"pose metrics '{tag}' (P={P} K={K} S={S}): max relative error " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, e in worst.items():
        assert e < TOL, (tag, name, e)
    # the outputs agree with each other bit for bit
    assert torch.equal(out["rmsd"], out["rmsd_per_ref"].min(-1).values) if per_ref else True
    return worst


def run(make, place, pos, ref, perm=None, atom_index=None, points=None, per_ref=True):
    m = model_for(make)
    t = lambda a, dt: None if a is None else place(torch.as_tensor(np.asarray(a)).to(dt))
    return m.pose_metrics(t(pos, torch.float32), t(ref, torch.float32), perm=t(perm, torch.int32), atom_index=t(atom_index, torch.int32),
                          points=t(points, torch.float32), per_ref=per_ref)


def some_points(q, seed=5):
    return (np.random.default_rng(seed).normal(0.0, 6.0, size=(q, 3)) + np.array([20.0, -15.0, 30.0])).astype(np.float32)


# ------------------------------------------------------------------ 1. fixture
def fixture_case(make, place, name):
    """All outputs on a fixture molecule: rmsd / rmsd_per_ref against the spyrmsd-EXECUTED values, the rest against the restatement."""
    mol = fixture()[name]
    pos, ref, perm = mol["pos"].numpy(), mol["ref"].numpy(), mol["perm"].numpy()
    pts = some_points(300)
    out = run(make, place, pos, ref, perm, points=pts)
    want = restated(pos, ref, perm, points=pts)
    e_ref = rel(out["rmsd"].cpu().numpy(), mol["rmsd"].numpy())
    e_per = rel(out["rmsd_per_ref"].cpu().numpy(), mol["rmsd_per_ref"].numpy().T)
    print(f"fixture '{name}': rmsd vs spyrmsd.symmrmsd (executed) {e_ref:.2e}, per reference {e_per:.2e}")
    assert e_ref < TOL and e_per < TOL, (e_ref, e_per)
    check(name, out, want)
    # a kernel that ignored perm would report the plain value: it differs for these inputs
    differs = int((out["rmsd_plain"] != out["rmsd"]).sum())
    assert differs == mol["plain_differs"] and differs >= 37, differs
    # isomorphisms(): the same SET of rows as the reference-enumerated ones
    iso = isomorphisms(mol["z"].numpy(), bonds=mol["bonds"].tolist())
    assert iso.complete and iso.perm.dtype == np.int32 and iso.perm.shape == perm.shape
    assert sorted(map(tuple, iso.perm.tolist())) == sorted(map(tuple, perm.tolist()))
    adj = isomorphisms(mol["z"].numpy(), adjacency=mol["adjacency"].numpy())
    assert sorted(map(tuple, adj.perm.tolist())) == sorted(map(tuple, perm.tolist()))


# ------------------------------------------------------------------ 2. edge shapes
def edge_inputs(shape):
    fx = fixture()["sym576"]
    pos, ref, perm = fx["pos"].numpy(), fx["ref"].numpy(), fx["perm"].numpy()
    rng = np.random.default_rng(17)
    off = np.array([20.0, -15.0, 30.0])
    cloud = lambda *s: (rng.normal(0.0, 2.0, size=s + (3,)) + off).astype(np.float32)
    if shape == "m1":              # one atom: no pair, min_self_distance = +inf
        return dict(pos=cloud(3, 1), ref=cloud(2, 1), perm=np.zeros((1, 1), np.int32), points=some_points(4))
    if shape == "n2":              # two identical atoms
        return dict(pos=cloud(3, 2), ref=cloud(1, 2), perm=np.array([[0, 1], [1, 0]], np.int32), points=some_points(4))
    if shape == "n65":             # one atom past a wave
        rows = np.stack([np.arange(65)] + [rng.permutation(65) for _ in range(2)]).astype(np.int32)
        return dict(pos=cloud(2, 65), ref=cloud(2, 65), perm=rows, points=some_points(4))
    if shape == "P1":
        return dict(pos=pos[:1], ref=ref, perm=perm, points=some_points(4))
    if shape == "K1_noperm":
        return dict(pos=pos, ref=ref[:1], perm=None, points=some_points(4))
    if shape == "S575":            # a ragged last chunk of permutations
        return dict(pos=pos[:8], ref=ref, perm=perm[:575], points=some_points(4))
    if shape == "nopoints":
        return dict(pos=pos[:4], ref=ref, perm=perm[:70], points=None)
    if shape == "Q1":
        return dict(pos=pos[:4], ref=ref, perm=perm[:70], points=some_points(1))
    if shape == "Q300":            # more points than threads of a workgroup
        return dict(pos=pos[:4], ref=ref, perm=perm[:70], points=some_points(300))
    if shape == "m2049":           # past the LDS budget of 2048 kept atoms: the in-place path, with a gather
        n, m = 2100, 2049
        keep = np.sort(rng.permutation(n)[:m]).astype(np.int32)
        rows = np.stack([np.arange(m), np.arange(m)[::-1], rng.permutation(m)]).astype(np.int32)
        return dict(pos=cloud(2, n), ref=cloud(2, m), perm=rows, atom_index=keep, points=some_points(5))
    raise KeyError(shape)


EDGE_SHAPES = ("m1", "n2", "n65", "P1", "K1_noperm", "S575", "nopoints", "Q1", "Q300", "m2049")


def edge_shape_case(make, place, shape):
    kw = edge_inputs(shape)
    out = run(make, place, **kw)
    want = restated(**kw)
    check(shape, out, want)
    if shape == "m1":
        assert torch.isinf(out["min_self_distance"]).all() and (out["min_self_distance"] > 0).all()
        assert torch.equal(out["rmsd"], out["rmsd_plain"])
    if shape == "nopoints":
        assert torch.isinf(out["min_point_distance"]).all() and (out["min_point_distance"] > 0).all()
    if shape == "K1_noperm":       # identity only: the symmetric value IS the plain one, and best = (0, 0)
        assert torch.equal(out["rmsd"], out["rmsd_plain"]) and not out["best"].any()


def atom_index_ties_case(make, place):
    """atom_index dropping every third atom; the rows of perm (m-space) are the isomorphisms that keep the kept set, restricted to
    it, and the whole list is given twice, so every row coincides with another on the kept atoms: exact ties, and `best` must be the
    lowest index of its row."""
    fx = fixture()["sym576"]
    pos, ref, perm = fx["pos"].numpy(), fx["ref"].numpy(), fx["perm"].numpy()
    keep = np.array([j for j in range(pos.shape[1]) if j % 3 != 2], dtype=np.int32)
    new = -np.ones(pos.shape[1], dtype=np.int64)
    new[keep] = np.arange(len(keep))
    rows = np.array([new[row[keep]] for row in perm if (new[row[keep]] >= 0).all()], dtype=np.int32)
    assert len(rows) >= 2
    rows = np.concatenate([rows, rows])
    out = run(make, place, pos, ref[:, keep], rows, atom_index=keep, points=some_points(4))
    want = restated(pos, ref[:, keep], rows, atom_index=keep, points=some_points(4))
    check("atom_index ties", out, want)
    best = out["best"].cpu().numpy()
    first = np.array([min(s for s in range(len(rows)) if np.array_equal(rows[s], rows[b])) for b in best[:, 1]])
    print(f"atom_index ties: m = {len(keep)}, {len(rows)} rows, {len(set(map(tuple, rows.tolist())))} distinct")
    assert len(set(map(tuple, rows.tolist()))) <= len(rows) // 2 and np.array_equal(best[:, 1], first), (best[:, 1], first)
    # the same reference twice: equal sums under k = 0 and k = 1, the lower k wins
    twice = run(make, place, pos, np.concatenate([ref[:1, keep], ref[:1, keep]]), rows, atom_index=keep)
    assert not twice["best"][:, 0].any()
    assert torch.equal(twice["rmsd_per_ref"][:, 0], twice["rmsd_per_ref"][:, 1])


# ------------------------------------------------------------------ 3. independence
def independence_case(make, place):
    fx = fixture()
    mol = fx["sym576"]
    pos, ref, perm = mol["pos"].numpy(), mol["ref"].numpy(), mol["perm"].numpy()[:130]       # three chunks, the last one of two rows
    pts = some_points(7)
    keys = DIST + ("rmsd_per_ref", "best")
    whole = run(make, place, pos, ref, perm, points=pts)
    for p in range(pos.shape[0]):          # 40 poses in one call = each pose alone
        alone = run(make, place, pos[p:p + 1], ref, perm, points=pts)
        for k in keys:
            assert torch.equal(whole[k][p:p + 1], alone[k]), (p, k)
    one_ref = run(make, place, pos[:6], ref[1:], perm[30:100])           # other K, S: the value of a triple does not move
    sub = run(make, place, pos[:6], ref, perm[30:100])
    assert torch.equal(one_ref["rmsd_per_ref"][:, 0], sub["rmsd_per_ref"][:, 1])
    traj = pos[:15].reshape(3, 5, -1, 3)                                  # [T = 3, P, n, 3] = three calls
    tout = run(make, place, traj, ref, perm, points=pts)
    for k in keys:
        assert tout[k].shape[:2] == (3, 5)
    for t in range(3):
        step = run(make, place, traj[t], ref, perm, points=pts)
        for k in keys:
            assert torch.equal(tout[k][t], step[k]), (t, k)
    # pose-by-pose matrix (clustering): ref = pos
    mol = fx["1a0q"]
    pos, perm = mol["pos"].numpy(), mol["perm"].numpy()
    d = run(make, place, pos, pos, perm)["rmsd_per_ref"].cpu().double()
    assert d.shape == (40, 40) and not d.diagonal().any()
    off = ~torch.eye(40, dtype=torch.bool)
    asym = float(((d - d.T).abs() / d.clamp(min=1e-30))[off].max())
    print(f"pose-by-pose matrix: max relative asymmetry {asym:.2e}")
    assert asym < TOL and float(d[off].min()) > 0.5


# ------------------------------------------------------------------ 4. evaluate_poses
def evaluate_case(make, place):
    mol = fixture()["sym576"]
    pos, ref, perm = place(mol["pos"]), place(mol["ref"]), mol["perm"].numpy()
    m = model_for(make)
    rng = np.random.default_rng(23)
    conf = rng.normal(size=40).astype(np.float32)
    conf[7] = np.nan
    out = evaluate_poses(pos, ref, model=m, perm=perm, confidence=place(torch.from_numpy(conf)))
    order = np.argsort(np.nan_to_num(conf, nan=-1e-6))[::-1]                                  # evaluate.py:491-493
    assert out["complete"] is True and np.array_equal(out["order"].cpu().numpy(), order)
    rmsd = out["rmsd"].cpu().numpy()
    assert out["top1_rmsd"].item() == rmsd[order][0] and out["top5_rmsd"].item() == np.min(rmsd[order][:5])   # evaluate.py:627
    assert rel(rmsd, mol["rmsd"].numpy()) < TOL
    assert np.array_equal(out["rmsd_below_2"].cpu().numpy(), rmsd < 2) and np.array_equal(out["rmsd_below_5"].cpu().numpy(), rmsd < 5)
    assert 0 < int(out["rmsd_below_2"].sum()) < 40
    for v in (out["order"], out["top1_rmsd"], out["top5_rmsd"], out["rmsd_below_2"]):
        assert v.device == pos.device
    few = perm[:70]                                                                            # (the rest: fewer rows, the same code)
    one = evaluate_poses(pos, ref, model=m, perm=few, confidence=place(torch.from_numpy(conf)))
    two = np.stack([conf, -conf], axis=1)                                                      # a two-column confidence: column 0
    out2 = evaluate_poses(pos, ref, model=m, perm=few, confidence=place(torch.from_numpy(two)))
    assert torch.equal(out2["order"], out["order"]) and torch.equal(out2["top5_rmsd"], one["top5_rmsd"])
    # a trajectory: the ordering of the poses applies to every step
    traj = evaluate_poses(torch.stack([pos, pos.flip(0)]), ref, model=m, perm=few, confidence=place(torch.from_numpy(conf)))
    assert traj["top1_rmsd"].shape == (2,) and traj["top1_rmsd"][0] == one["top1_rmsd"]
    assert traj["top1_rmsd"][1].item() == one["rmsd"].cpu().numpy()[::-1][order][0]
    # an enumeration cut short is reported, and its RMSD is an upper bound
    cut = isomorphisms(mol["z"].numpy(), bonds=mol["bonds"].tolist(), max_isomorphisms=10)
    assert isinstance(cut, Isomorphisms) and cut.complete is False and cut.perm.shape == (10, 21)
    assert any(np.array_equal(r, np.arange(21)) for r in cut.perm)
    part = evaluate_poses(pos, ref, model=m, perm=cut)
    assert part["complete"] is False and "order" not in part
    assert (part["rmsd"] >= out["rmsd"]).all() and (part["rmsd"] > out["rmsd"]).any()
    assert (part["rmsd"] <= part["rmsd_plain"]).all() and torch.equal(part["rmsd_plain"], out["rmsd_plain"])


# ------------------------------------------------------------------ 5. errors
def errors_case(make, place):
    m = model_for(make)
    mol = fixture()["1a0q"]
    pos, ref = place(mol["pos"].clone()), place(mol["ref"].clone())
    out = place(torch.zeros(40))

    def call(**kw):
        c = L.PoseMetricsCfg()
        c.struct_size = ctypes.sizeof(L.PoseMetricsCfg)
        c.n_poses, c.n_atoms, c.n_kept, c.n_refs = 40, 23, 23, 2
        c.pos, c.ref, c.rmsd = pos.data_ptr(), ref.data_ptr(), out.data_ptr()
        for k, v in kw.items():
            setattr(c, k, v)
        return m.lib.ddmi_pose_metrics(m._h, ctypes.byref(c), m._stream())
    assert call() == 0
    for kw in (dict(struct_size=ctypes.sizeof(L.PoseMetricsCfg) - 8), dict(pos=None), dict(ref=None), dict(n_poses=0), dict(n_kept=24),
               dict(n_kept=20), dict(n_refs=0), dict(n_atoms=-1), dict(perm=pos.data_ptr(), n_perms=0),
               dict(points=pos.data_ptr(), n_points=0)):
        rc = call(**kw)
        assert rc == -1, (kw, rc)                                   # DDMI_ERR_ARG
        with pytest.raises(L.DdmiError, match="ddmi error -1: ddmi_pose_metrics_cfg"):
            L.check(m.lib, rc)
    with pytest.raises(L.DdmiError, match="ddmi error -1"):         # through the wrapper: P = 0 is refused
        m.pose_metrics(pos[:0], ref)
    with pytest.raises(ValueError, match="ref"):
        m.pose_metrics(pos, ref[:, :5])
    with pytest.raises(ValueError, match="max_isomorphisms"):
        isomorphisms(mol["z"].numpy(), bonds=mol["bonds"].tolist(), max_isomorphisms=0)


# ------------------------------------------------------------------ 7. recorded trajectory (run on the GPU)
def recorded_trajectory_case(make, place, steps=3):
    """One 3-step sample_batch(record=...) on the tiny CG case of the record tests: its recorded poses through pose_metrics as
    [T, P, n, 3] against the float64 restatement on the copied-back poses."""
    from diffdock_amd.hetero import HeteroBatch
    from oracle.conformer import get_t_schedule
    from record_cases import tiny_l1_inputs
    fx, cfg, dl, noise, temp = tiny_l1_inputs(2, steps)
    m = make(cfg, fx["state_dict"])
    batch = place(HeteroBatch.from_data_list([g.clone() for g in dl]))
    pos, rec = m.sample_batch(batch, steps, (get_t_schedule(steps),) * 3, noise=noise, no_final_step_noise=True, record={"pos"}, **temp)
    n = dl[0]["ligand"].pos.shape[0]
    traj = rec.pos.reshape(steps, 2, n, 3)
    ref = torch.stack([fx["graph"]["lig_pos"], dl[1]["ligand"].pos]).float()
    pts = dl[0]["receptor"].pos.float()
    out = m.pose_metrics(traj, place(ref), points=place(pts), per_ref=True)
    host = traj.cpu().numpy()
    assert np.isfinite(host).all() and torch.equal(traj[-1].reshape(-1, 3), pos)
    for t in range(steps):
        want = restated(host[t], ref.numpy(), points=pts.numpy())
        check(f"recorded step {t}", {k: v[t] for k, v in out.items()}, want)
    assert float((out["rmsd"][0] - out["rmsd"][-1]).abs().max()) > 1e-4          # the poses do move between the steps
