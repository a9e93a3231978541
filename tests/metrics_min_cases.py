"""Cases of the minimised symmetric RMSD and the fitting transform (ddmi_pose_fit, MIScoreModel.pose_fit, evaluate_poses(minimize=True),
metrics.superpose).  Run on the CPU emulation build by tests/test_metrics_min_emu.py and on the MI355X by tests/test_gpu_metrics_min.py
through the same C ABI; `make` and `place` as in tests/metrics_cases.py, whose handle and fixture cache are shared.

References: tests/golden/pose_metrics_min.pt, whose values come from EXECUTING the reference's vendored spyrmsd with minimize=True
(tests/golden/make_golden_metrics_min.py), and `restated_e` below: e = Ga + Gb - 2 lambda_max with numpy's eigvalsh of the key matrix
in float64 on the same float32 inputs -- the fixture script holds the same function and pins it to the executed values.

Bound: TOL = 1e-5 relative on every non-zero distance, derived and not measured: the kernel's arithmetic is float64 (absolute error of
e about 1e-12 A^2) up to one rounding of e to float32, one float32 division by m and one sqrtf, below 2e-7 relative.  Where the
reference's atol rule (|e| < 1e-9) gives 0 the device value must be exactly 0.0.  Indices are judged through values, as in
metrics_cases.check.  The transform: R and t are rounded to float32, which moves an atom by a few 1e-6 A as a near-rigid shift; the
plain RMSD after applying them in float64 is within 1e-5 * rmsd_min + 1e-5 A of rmsd_min.  Everything that compares the device with
itself is torch.equal."""
import ctypes

import numpy as np
import pytest
import torch

import diffdock_amd.lib as L
from diffdock_amd.metrics import evaluate_poses, superpose
from metrics_cases import TOL, fixture, model_for
from util import load_fixture

ATOL = 1e-9
FIT_KEYS = ("rmsd_min", "best_min", "rotation", "translation", "rmsd_min_per_ref")
_cache = {}


def fixture_min():
    if "fx" not in _cache:
        _cache["fx"] = load_fixture("pose_metrics_min")
    return _cache["fx"]


# ------------------------------------------------------------------ float64 restatement
def key_matrices(M):
    """[..., 3, 3] -> [..., 4, 4]: the symmetric key matrix of spyrmsd/qcp.py:55-122."""
    xx, xy, xz, yx, yy, yz, zx, zy, zz = (M[..., i, j] for i in range(3) for j in range(3))
    rows = [[xx + yy + zz, yz - zy, zx - xz, xy - yx], [yz - zy, xx - yy - zz, xy + yx, zx + xz],
            [zx - xz, xy + yx, -xx + yy - zz, yz + zy], [xy - yx, zx + xz, yz + zy, -xx - yy + zz]]
    return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)


def restated_e(pos, ref, perm=None, atom_index=None):
    """e = Ga + Gb - 2 lambda_max in float64 -> [P, K, S], for a_j = pos[p, atom_index[j]] and b_j = ref[k, perm[s, j]]."""
    pos, ref = np.asarray(pos, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    x = pos if atom_index is None else pos[:, np.asarray(atom_index)]
    perm = np.arange(ref.shape[1])[None] if perm is None else np.asarray(perm)
    A = x - x.mean(axis=1, keepdims=True)
    B = ref - ref.mean(axis=1, keepdims=True)
    Ga, Gb = (A ** 2).sum(axis=(1, 2)), (B ** 2).sum(axis=(1, 2))
    out = np.empty((x.shape[0], ref.shape[0], perm.shape[0]))
    for k in range(ref.shape[0]):
        M = np.einsum("pji,sjl->psil", A, B[k][perm])
        out[:, k] = Ga[:, None] + Gb[k] - 2.0 * np.linalg.eigvalsh(key_matrices(M))[..., -1]
    return out


def rmsd_of_e(e, m):
    return np.where(np.abs(e) < ATOL, 0.0, np.sqrt(np.maximum(e, 0.0) / m))


def rel0(got, want):
    """Max relative error where want != 0; where want == 0 the value must be exactly 0.0 (-> inf otherwise)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    zero = want == 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(zero, np.where(got == 0.0, 0.0, np.inf), np.abs(got - want) / np.abs(want))
    return float(np.max(np.where(np.isnan(e), np.inf, e))) if e.size else 0.0


def run(make, place, pos, ref, perm=None, atom_index=None, per_ref=True):
    m = model_for(make)
    t = lambda a, dt: None if a is None else place(torch.as_tensor(np.asarray(a)).to(dt))
    return m.pose_fit(t(pos, torch.float32), t(ref, torch.float32), perm=t(perm, torch.int32), atom_index=t(atom_index, torch.int32),
                      per_ref=per_ref)


def not_collinear(x):
    """m >= 3 atoms that span a plane at least: the second singular value of the centred coordinates is not small."""
    x = np.asarray(x, dtype=np.float64)
    return x.shape[0] >= 3 and np.linalg.svd(x - x.mean(0), compute_uv=False)[1] > 1e-3


def check(tag, out, pos, ref, perm=None, atom_index=None, executed=None, executed_per_ref=None):
    """rmsd_min / rmsd_min_per_ref within TOL of the restatement (and of the executed values when given), exact zeros, best_min
    through values, and the transform.  Returns the restated rmsd_min [P]."""
    pos, ref = np.asarray(pos), np.asarray(ref)
    x = pos if atom_index is None else pos[:, np.asarray(atom_index)]
    m = x.shape[1]
    e = restated_e(pos, ref, perm, atom_index)
    P, K, S = e.shape
    want_per = rmsd_of_e(e, m).min(-1)
    want = want_per.min(-1)
    got, got_per, best = out["rmsd_min"].cpu().numpy(), out["rmsd_min_per_ref"].cpu().numpy(), out["best_min"].cpu().numpy()
    assert got.dtype == np.float32 and got_per.dtype == np.float32 and best.dtype == np.int32 and best.shape == (P, 2)
    worst = dict(rmsd_min=rel0(got, want), rmsd_min_per_ref=rel0(got_per, want_per))
    if executed is not None:
        worst["rmsd_min vs executed"] = rel0(got, executed)
    if executed_per_ref is not None:
        worst["rmsd_min_per_ref vs executed"] = rel0(got_per, executed_per_ref)
    assert ((best[:, 0] >= 0) & (best[:, 0] < K) & (best[:, 1] >= 0) & (best[:, 1] < S)).all(), (tag, best)
    worst["best_min"] = rel0(rmsd_of_e(e[np.arange(P), best[:, 0], best[:, 1]], m), want)
    # the transform, applied in float64
    R, t = out["rotation"].cpu().numpy().astype(np.float64), out["translation"].cpu().numpy().astype(np.float64)
    assert R.shape == (P, 3, 3) and t.shape == (P, 3) and out["rotation"].dtype == torch.float32
    worst_det = float(np.abs(np.linalg.det(R) - 1.0).max())
    worst_orth = float(np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max())
    rows = np.arange(m)[None] if perm is None else np.asarray(perm)
    worst_fit, judged = 0.0, 0
    for p in range(P):
        if want[p] < 1e-3 or not not_collinear(x[p]) or not not_collinear(ref[best[p, 0]]):
            continue
        moved = x[p].astype(np.float64) @ R[p].T + t[p]
        after = np.sqrt(((moved - ref[best[p, 0]].astype(np.float64)[rows[best[p, 1]]]) ** 2).sum(-1).mean())
        worst_fit = max(worst_fit, abs(after - want[p]) / (1e-5 * want[p] + 1e-5))
        judged += 1
    print(f"pose fit '{tag}' (P={P} K={K} S={S} m={m}): max relative error " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f"; |det R - 1| {worst_det:.1e}, |R R^T - 1| {worst_orth:.1e}, transform of {judged} poses at {worst_fit:.2e} of its bound")
    for name, v in worst.items():
        assert v < TOL, (tag, name, v)
    assert worst_det < 1e-5 and worst_orth < 1e-5 and worst_fit < 1.0, (tag, worst_det, worst_orth, worst_fit)
    assert torch.equal(out["rmsd_min"], out["rmsd_min_per_ref"].min(-1).values)
    return want


# ------------------------------------------------------------------ 1. fixture molecules
def fixture_case(make, place, name):
    mol, mn = fixture()[name], fixture_min()[name]
    pos, ref, perm = mol["pos"].numpy(), mol["ref"].numpy(), mol["perm"].numpy()
    out = run(make, place, pos, ref, perm)
    check(name, out, pos, ref, perm, executed=mn["rmsd_min"].numpy(), executed_per_ref=mn["rmsd_min_per_ref"].numpy().T)
    # a test that read the unminimised output would fail: the values differ
    assert (mn["rmsd_min"].numpy() < mol["rmsd"].numpy() - 1e-3).all()


# ------------------------------------------------------------------ 2. rigid copies and small sets
def rigid_case(make, place, name):
    mol, rg = fixture()[name], fixture_min()[name]["rigid"]
    pos, ref, perm = rg["pos"].numpy(), mol["ref"].numpy(), mol["perm"].numpy()
    out = run(make, place, pos, ref, perm)
    executed = rg["rmsd_min"].numpy()
    check(name + " rigid", out, pos, ref, perm, executed=executed, executed_per_ref=rg["rmsd_min_per_ref"].numpy().T)
    sigma = rg["sigma"].numpy()
    got = out["rmsd_min"].cpu().numpy()
    assert (executed[sigma == 0] == 0).all() and (got[sigma == 0] == 0).all() and (got[sigma > 0] > 0).all(), got


SMALL_SETS = ("m1", "m2", "m3", "ring6", "chain4", "mirror5")


def small_set_case(make, place, name):
    st = fixture_min()["small"][name]
    pos, ref = st["pos"].numpy()[None], st["ref"].numpy()[None]
    out = run(make, place, pos, ref)
    check("small " + name, out, pos, ref, executed=np.array([st["rmsd_min"]]))
    got = out["rmsd_min"].item()
    if name == "m1":
        assert got == 0.0 and torch.equal(out["rotation"].cpu(), torch.eye(3)[None])
        assert torch.equal(out["translation"].cpu(), torch.from_numpy(ref[0] - pos[0]))
    if name == "mirror5":      # a Kabsch that allowed a reflection would return 0
        assert st["rmsd_min"] > 0.1 and got > 0.1


# ------------------------------------------------------------------ 4. edge shapes
#             name           m     S     K  P
EDGE_SHAPES = {"m1_noperm": (1, None, 1, 1), "m2_S1": (2, 1, 3, 5), "m3_noperm": (3, None, 1, 5), "m63_S63": (63, 63, 3, 1),
               "m64_S64": (64, 64, 1, 5), "m65_S65": (65, 65, 3, 5), "m130_S130": (130, 130, 1, 1), "atom_index": (27, 5, 3, 5),
               "m2049": (2049, 2, 1, 2)}


def edge_inputs(shape):
    m, S, K, P = EDGE_SHAPES[shape]
    rng = np.random.default_rng(29)
    off = np.array([20.0, -15.0, 30.0])
    cloud = lambda *s: (rng.normal(0.0, 2.0, size=s + (3,)) + off).astype(np.float32)
    n = {"atom_index": 40, "m2049": 2100}.get(shape, m)
    keep = None if n == m else np.sort(rng.permutation(n)[:m]).astype(np.int32)
    perm = None if S is None else np.stack([rng.permutation(m) for _ in range(S)]).astype(np.int32)
    return dict(pos=cloud(P, n), ref=cloud(K, m), perm=perm, atom_index=keep)


def edge_shape_case(make, place, shape):
    kw = edge_inputs(shape)
    out = run(make, place, **kw)
    check(shape, out, **kw)
    if kw["perm"] is None:
        assert not out["best_min"][:, 1].any()


# ------------------------------------------------------------------ 5. independence and ties
def independence_case(make, place):
    mol = fixture()["sym576"]
    pos, ref, perm = mol["pos"].numpy()[:6], mol["ref"].numpy(), mol["perm"].numpy()[:130]   # three chunks, the last one of two rows
    whole = run(make, place, pos, ref, perm)
    for p in range(pos.shape[0]):          # a batch = each pose alone
        alone = run(make, place, pos[p:p + 1], ref, perm)
        for k in FIT_KEYS:
            assert torch.equal(whole[k][p:p + 1], alone[k]), (p, k)
    traj = run(make, place, pos.reshape(2, 3, -1, 3), ref, perm)          # [T = 2, P, n, 3] = two calls
    for k in FIT_KEYS:
        assert traj[k].shape[:2] == (2, 3) and torch.equal(traj[k].reshape(whole[k].shape), whole[k]), k
    # references and permutation rows added around the winning ones: the value of a triple does not move
    sub = run(make, place, pos, ref[1:], perm[30:100])
    more = run(make, place, pos, ref, perm[30:100])
    assert torch.equal(sub["rmsd_min_per_ref"][:, 0], more["rmsd_min_per_ref"][:, 1])
    best = whole["best_min"].cpu().numpy()
    for p in range(pos.shape[0]):
        k, s = best[p]
        lo, hi = max(0, s - 3), min(len(perm), s + 4)
        few = run(make, place, pos[p:p + 1], ref[k:k + 1], perm[lo:hi])
        assert few["best_min"].cpu().tolist() == [[0, s - lo]], (p, few["best_min"], k, s)
        for name in ("rmsd_min", "rotation", "translation"):
            assert torch.equal(few[name], whole[name][p:p + 1]), (p, name)
    # exact ties: a duplicated permutation row and a duplicated known pose fall to the lowest k * S + s
    rows = np.concatenate([perm[:70], perm[:70]])
    twice = run(make, place, pos, np.concatenate([ref, ref]), rows)
    once = run(make, place, pos, ref, perm[:70])
    assert torch.equal(twice["best_min"], once["best_min"]) and torch.equal(twice["rmsd_min"], once["rmsd_min"])
    assert torch.equal(twice["rmsd_min_per_ref"][:, :2], twice["rmsd_min_per_ref"][:, 2:])
    assert torch.equal(twice["rotation"], once["rotation"]) and torch.equal(twice["translation"], once["translation"])


# ------------------------------------------------------------------ 6. evaluate_poses(minimize=True), superpose
TODAY = {"rmsd", "best", "rmsd_plain", "centroid_distance", "min_self_distance", "min_point_distance", "complete", "rmsd_below_2",
         "rmsd_below_5", "order", "top1_rmsd", "top5_rmsd"}


def evaluate_case(make, place):
    mol, mn = fixture()["sym576"], fixture_min()["sym576"]
    N = 12                                                                                    # (the ordering needs more than five poses)
    pos, ref, perm = place(mol["pos"][:N]), place(mol["ref"]), mol["perm"].numpy()[:20]
    m = model_for(make)
    conf = np.random.default_rng(23).normal(size=N).astype(np.float32)
    conf[7] = np.nan
    cf = place(torch.from_numpy(conf))
    plain = evaluate_poses(pos, ref, model=m, perm=perm, confidence=cf)
    off = evaluate_poses(pos, ref, model=m, perm=perm, confidence=cf, minimize=False)
    assert set(plain) == TODAY and set(off) == TODAY
    out = evaluate_poses(pos, ref, model=m, perm=perm, confidence=cf, minimize=True, per_ref=True)
    assert set(out) == TODAY | {"rmsd_per_ref"} | set(FIT_KEYS) | {"top1_rmsd_min", "top5_rmsd_min"}
    for k in TODAY:
        same = (lambda a, b: torch.equal(a, b)) if torch.is_tensor(plain[k]) else (lambda a, b: a == b)
        assert same(plain[k], off[k]) and same(plain[k], out[k]), k
    direct = m.pose_fit(pos, ref, perm=place(torch.from_numpy(perm)), per_ref=True)
    for k in FIT_KEYS:
        assert torch.equal(out[k], direct[k]) and out[k].device == pos.device, k
    order = np.argsort(np.nan_to_num(conf, nan=-1e-6))[::-1]                                  # evaluate.py:491-493
    rmin = out["rmsd_min"].cpu().numpy()
    assert out["top1_rmsd_min"].item() == rmin[order][0] and out["top5_rmsd_min"].item() == np.min(rmin[order][:5])
    assert (out["rmsd_min"] <= out["rmsd"]).all() and (out["rmsd_min"] < out["rmsd"]).any()
    assert (rmin >= mn["rmsd_min"].numpy()[:N] * (1 - TOL)).all()                             # 20 of the 576 rows: an upper bound
    # superpose: pos @ R^T + t on the device, and the poses it returns sit at rmsd_min from their best known pose
    moved = superpose(pos, out)
    assert moved.device == pos.device and moved.shape == pos.shape
    assert torch.equal(moved, pos @ out["rotation"].transpose(-1, -2) + out["translation"].unsqueeze(-2))
    best = out["best_min"].cpu().numpy()
    target = mol["ref"].numpy().astype(np.float64)[best[:, 0][:, None], perm[best[:, 1]]]
    after = np.sqrt(((moved.cpu().numpy().astype(np.float64) - target) ** 2).sum(-1).mean(-1))
    assert np.abs(after - rmin).max() < 1e-4, np.abs(after - rmin).max()    # float32 arithmetic on 40 A coordinates: a few 1e-6 A per atom
    # a trajectory: the ordering of the poses applies to every step
    traj = evaluate_poses(torch.stack([pos, pos.flip(0)]), ref, model=m, perm=perm, confidence=cf, minimize=True)
    assert traj["top1_rmsd_min"].shape == (2,) and traj["top1_rmsd_min"][0] == out["top1_rmsd_min"]
    assert traj["top1_rmsd_min"][1].item() == rmin[::-1][order][0]
    assert traj["rotation"].shape == (2, N, 3, 3) and superpose(torch.stack([pos, pos.flip(0)]), traj).shape == (2, N, 21, 3)


# ------------------------------------------------------------------ 7. errors
def errors_case(make, place):
    m = model_for(make)
    mol = fixture()["1a0q"]
    pos, ref = place(mol["pos"].clone()), place(mol["ref"].clone())
    out = place(torch.zeros(40))

    def call(**kw):
        c = L.PoseFitCfg()
        c.struct_size = ctypes.sizeof(L.PoseFitCfg)
        c.n_poses, c.n_atoms, c.n_kept, c.n_refs = 40, 23, 23, 2
        c.pos, c.ref, c.rmsd_min = pos.data_ptr(), ref.data_ptr(), out.data_ptr()
        for k, v in kw.items():
            setattr(c, k, v)
        return m.lib.ddmi_pose_fit(m._h, ctypes.byref(c), m._stream())
    assert call() == 0
    for kw in (dict(struct_size=ctypes.sizeof(L.PoseFitCfg) - 8), dict(pos=None), dict(ref=None), dict(n_poses=0), dict(n_kept=24),
               dict(n_kept=20), dict(n_refs=0), dict(n_atoms=-1), dict(perm=pos.data_ptr(), n_perms=0)):
        rc = call(**kw)
        assert rc == -1, (kw, rc)                                   # DDMI_ERR_ARG
        with pytest.raises(L.DdmiError, match="ddmi error -1: ddmi_pose_fit_cfg"):
            L.check(m.lib, rc)
    with pytest.raises(L.DdmiError, match="ddmi error -1"):         # through the wrapper: P = 0 is refused
        m.pose_fit(pos[:0], ref)
    with pytest.raises(ValueError, match="ref"):
        m.pose_fit(pos, ref[:, :5])
    with pytest.raises(ValueError, match="perm"):
        m.pose_fit(pos, ref, perm=torch.zeros(3, 5, dtype=torch.int32))
    with pytest.raises(TypeError):                                  # pose_fit has no points
        m.pose_fit(pos, ref, points=pos[0])


# ------------------------------------------------------------------ 8. recorded trajectory (run on the GPU)
def recorded_trajectory_case(make, place, steps=3):
    """One 3-step sample_batch(record=...) on the tiny CG case of the record tests: its recorded poses through pose_fit as
    [T, P, n, 3] equal the per-step calls bit for bit, and the restatement on the copied-back poses."""
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
    out = m.pose_fit(traj, place(ref), per_ref=True)
    host = traj.cpu().numpy()
    assert np.isfinite(host).all() and torch.equal(traj[-1].reshape(-1, 3), pos)
    for t in range(steps):
        step = m.pose_fit(traj[t], place(ref), per_ref=True)
        for k in FIT_KEYS:
            assert torch.equal(out[k][t], step[k]), (t, k)
        check(f"recorded step {t}", step, host[t], ref.numpy())
