"""Cases of conformer matching on the device (ddmi_match_conformer, MIScoreModel.match_conformer, diffdock_amd.matching,
io.complex_graph(conformers=...)).  Run on the CPU emulation build by tests/test_matching_emu.py and on the MI355X by
tests/test_gpu_matching.py through the same C ABI; `make` and `place` as in tests/metrics_cases.py, whose handle is shared.

Ligands are synth.make_complex(seed, n_res=20, n_lig=n) ligands; the target is the ligand twisted by seeded angles in float64
(synth._torsion_update_numpy) plus seeded Gaussian noise of 0.3 A unless a case says otherwise.  All conformers stay within 16 A of
the origin.

Reference of the objective: the numpy torsion loop in float64 followed by restated_e / rmsd_of_e of metrics_min_cases.py.
Bound: OBJ_ATOL + OBJ_RTOL * value = 1e-4 A + 1e-5 * value, derived and not measured: a float32 rotation step moves a coordinate of
magnitude < 16 A by a few ulp (1e-6 A), there are at most 12 sequential steps (the objective cases pass at most the first 12
rotatable bonds of a ligand), and the RMSD is 1-Lipschitz in the RMS displacement; the float64 part is bounded as in
metrics_min_cases.py.  The transform bound (1e-5 * rmsd + 1e-5 A) is the one of the pose-fit tests.  Everything that compares the
device with itself is torch.equal."""
import ctypes
import gzip
import os

import numpy as np
import pytest
import torch

import diffdock_amd.lib as L
from diffdock_amd.matching import match_conformers, match_conformers_host, torsion_table
from diffdock_amd.synth import _torsion_update_numpy, make_complex
from metrics_cases import TOL, model_for
from metrics_min_cases import restated_e, rmsd_of_e
from util import load_fixture

OBJ_ATOL, OBJ_RTOL = 1e-4, 1e-5
OUT_KEYS = ("angles", "rmsd", "pos", "best_history")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ jobs
def ligand(seed, n, max_bonds=None):
    g = make_complex(seed, n_res=20, n_lig=n)
    u, v, mask = torsion_table(g)
    if max_bonds is not None:
        u, v, mask = u[:max_bonds], v[:max_bonds], mask[:max_bonds]
    return dict(start=g["ligand"].pos.numpy().astype(np.float32), u=u, v=v, mask=mask)


def twisted(job, seed, noise=0.3):
    """The job with its target: the start twisted by seeded angles in float64, plus seeded noise."""
    rng = np.random.default_rng(1000 + seed)
    ang = rng.uniform(-np.pi, np.pi, size=len(job["u"]))
    tgt = _torsion_update_numpy(job["start"].astype(np.float64), list(zip(job["u"], job["v"])), job["mask"], ang)
    tgt = tgt + noise * rng.normal(size=tgt.shape)
    out = dict(job, target=tgt.astype(np.float32), true_angles=ang)
    assert np.linalg.norm(out["start"], axis=1).max() < 16 and np.linalg.norm(out["target"], axis=1).max() < 16
    return out


def synth_job(seed, n, noise=0.3, max_bonds=None):
    return twisted(ligand(seed, n, max_bonds), seed, noise)


def restated(job, theta):
    """E(theta) in float64 on the float32 inputs."""
    x = _torsion_update_numpy(job["start"].astype(np.float64), list(zip(job["u"], job["v"])), job["mask"], np.asarray(theta, dtype=np.float64))
    return float(rmsd_of_e(restated_e(x[None], job["target"][None]), len(x))[0, 0, 0])


def run(make, place, jobs, init=None, **kw):
    """One device call on a list of jobs; init = per job [n_init, R] rows."""
    m = model_for(make)
    lig = np.cumsum([0] + [len(j["start"]) for j in jobs])
    tor = np.cumsum([0] + [len(j["u"]) for j in jobs])
    cat = lambda key, dt: place(torch.from_numpy(np.concatenate([np.asarray(j[key]).reshape(-1) for j in jobs]).astype(dt)))
    args = dict(rot_u=cat("u", np.int32), rot_v=cat("v", np.int32), mask_rotate=cat("mask", np.uint8)) if tor[-1] else {}
    if init is not None:
        n_init = len(init[0])
        kw.update(n_init=n_init, init_angles=place(torch.from_numpy(np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1) for a in init]))))
    pos = lambda key: place(torch.from_numpy(np.concatenate([j[key] for j in jobs]).astype(np.float32)))
    out = m.match_conformer(pos("start"), pos("target"), lig, tor, **args, **kw)
    out["lig_ptr"], out["tor_ptr"] = lig, tor
    return out


def split(out, j):
    """Job j's slices of a batch result."""
    lig, tor = out["lig_ptr"], out["tor_ptr"]
    return dict(angles=out["angles"][tor[j]:tor[j + 1]], rmsd=out["rmsd"][j], pos=out["pos"][lig[j]:lig[j + 1]], best_history=out["best_history"][j],
                n_generations=out["n_generations"][j])


def check_result(make, place, tag, out, jobs, zero_row=True):
    """Result consistency of an optimiser run, in float64 on the host; zero_row: the run had no caller rows."""
    hist = out["best_history"].cpu().numpy()
    assert torch.equal(out["rmsd"], out["best_history"][:, -1]), tag
    assert (hist[:, 1:] <= hist[:, :-1]).all(), (tag, hist)
    assert (out["angles"].abs().cpu().numpy().astype(np.float64) <= np.pi).all(), tag
    worst_fit = worst_obj = 0.0
    for j, job in enumerate(jobs):
        r = split(out, j)
        rmsd = float(r["rmsd"])
        pos = r["pos"].cpu().numpy().astype(np.float64)
        plain = np.sqrt(((pos - job["target"].astype(np.float64)) ** 2).sum(-1).mean())
        worst_fit = max(worst_fit, abs(plain - rmsd) / (1e-5 * rmsd + 1e-5))
        e = restated(job, r["angles"].cpu().numpy())
        worst_obj = max(worst_obj, abs(e - rmsd) / (OBJ_ATOL + OBJ_RTOL * e))
    print(f"matching '{tag}': pos at {worst_fit:.2e} of the transform bound, E(angles) at {worst_obj:.2e} of the objective bound")
    assert worst_fit < 1.0 and worst_obj < 1.0, (tag, worst_fit, worst_obj)
    if zero_row:   # the zero row: the start is never worse than the unmatched conformer, as the device evaluates it
        zero = run(make, place, jobs, init=[np.zeros((1, len(j["u"]))) for j in jobs], popsize=1, maxiter=0)
        assert (out["best_history"][:, 0] <= zero["init_energy"][:, 0]).all(), tag


def optimise(make, place, jobs, tag, **kw):
    out = run(make, place, jobs, **kw)
    check_result(make, place, tag, out, jobs, zero_row="init" not in kw)
    return out


# ------------------------------------------------------------------ 1. the objective
#              n: (seed, bonds passed)
OBJECTIVE_SHAPES = {1: (0, None), 2: (0, None), 5: (1, None), 12: (0, None), 30: (0, None), 63: (6, None), 64: (4, None), 65: (4, None), 130: (10, 12)}


def objective_case(make, place, n):
    seed, max_bonds = OBJECTIVE_SHAPES[n]
    job = synth_job(seed, n, max_bonds=max_bonds)
    R = len(job["u"])
    assert R <= 12 and (R == 0) == (n <= 2) and (n != 5 or R == 1)
    rows = np.random.default_rng(7 + n).uniform(-np.pi, np.pi, size=(8, R)).astype(np.float32)
    rows[3] = 0.0
    out = run(make, place, [job], init=[rows], popsize=1, maxiter=0)
    got = out["init_energy"].cpu().numpy()[0].astype(np.float64)
    want = np.array([restated(job, r) for r in rows])
    err = np.abs(got - want) / (OBJ_ATOL + OBJ_RTOL * want)
    print(f"objective n={n} R={R}: worst error {np.abs(got - want).max():.2e} A, {err.max():.2e} of the bound")
    assert err.max() < 1.0, (n, got, want)
    # an all-zero row = pose_fit(start, target)
    m = model_for(make)
    fit = m.pose_fit(place(torch.from_numpy(job["start"]))[None], place(torch.from_numpy(job["target"])))["rmsd_min"].item()
    assert abs(got[3] - fit) <= TOL * fit, (got[3], fit)
    # maxiter = 0 returns the argmin of the initial population
    assert out["rmsd"].item() == out["init_energy"].min().item() and out["n_generations"].item() == 0
    assert torch.equal(out["angles"].cpu(), torch.from_numpy(rows[int(out["init_energy"][0].argmin())]))
    # target = start with zero angles: exactly 0.0
    same = dict(job, target=job["start"])
    out0 = run(make, place, [same], init=[np.zeros((1, R))], popsize=1, maxiter=0)
    assert out0["init_energy"].item() == 0.0


# ------------------------------------------------------------------ 3. determinism and independence
BATCH = ((1, 5), (0, 30), (0, 1), (4, 65), (0, 12))    # (seed, n): R = 1, 11, 0, 8, 4; an R = 0 job in the middle
SMALL = dict(popsize=8, maxiter=6, tol=0.0)             # P = 8, 88, -, 64, 32: every one a multiple of the 8 waves per workgroup
ODD = dict(popsize=7, maxiter=6, tol=0.0)               # P = 7, 77, -, 56, 28: 7, 77 and 28 are no multiples of the 8 waves


def determinism_case(make, place, budget=SMALL):
    jobs =[synth_job(s, n) for s, n in BATCH]
    whole = optimise(make, place, jobs, f"ragged batch of five, popsize {budget['popsize']}", seed=3, **budget)
    again = run(make, place, jobs, seed=3, **budget)
    for k in OUT_KEYS + ("n_generations",):
        assert torch.equal(whole[k], again[k]), k
    assert whole["n_generations"].cpu().tolist() == [6, 6, 0, 6, 6]
    for j in (1, 2, 3):          # a job of the batch = the job alone with its job id
        alone = run(make, place, [jobs[j]], seed=3, job_ids=[j], **budget)
        a, b = split(whole, j), split(alone, 0)
        for k in OUT_KEYS:
            assert torch.equal(a[k], b[k]), (j, k)
    order = [3, 0, 4, 2, 1]
    perm = run(make, place, [jobs[j] for j in order], seed=3, job_ids=order, **budget)
    for at, j in enumerate(order):
        a, b = split(whole, j), split(perm, at)
        for k in OUT_KEYS:
            assert torch.equal(a[k], b[k]), (j, k)
    other = run(make, place, jobs, seed=4, **budget)
    assert not torch.equal(other["angles"], whole["angles"])
    # five members for one bond and popsize 1: P = max(5, popsize R)
    one = optimise(make, place, [jobs[0]], "P = 5", popsize=1, maxiter=6, tol=0.0)
    assert one["n_generations"].item() == 6


# ------------------------------------------------------------------ 4. edges
def edges_case(make, place):
    job = synth_job(0, 12)
    R = len(job["u"])
    # tol large enough to stop after generation 1
    out = optimise(make, place, [job], "early stop", popsize=4, maxiter=5, tol=1e6)
    assert out["n_generations"].item() == 1
    h = out["best_history"][0]
    assert torch.equal(h[1:], h[1].expand(5))
    # more caller rows than popsize * R
    rows = np.random.default_rng(5).uniform(-np.pi, np.pi, size=(3 * R + 2, R)).astype(np.float32)
    out = optimise(make, place, [job], "n_init > popsize R", init=[rows], popsize=3, maxiter=2, tol=0.0)
    assert out["init_energy"].shape == (1, 3 * R + 2) and out["best_history"][0, 0].item() == out["init_energy"].min().item()
    # a population that does not fit LDS lives in the handle's scratch (a second launch): alone, and next to a job that fits
    big = synth_job(1, 65)
    assert len(big["u"]) == 27 and 4 * (2 * 12 * 27 * 27 + 12 * 27) > 64 * 1024
    alone = optimise(make, place, [big], "population in scratch", popsize=12, maxiter=2, tol=0.0, job_ids=[1])
    both = run(make, place, [job, big], popsize=12, maxiter=2, tol=0.0)
    for k in OUT_KEYS:
        assert torch.equal(split(both, 1)[k], split(alone, 0)[k]), k
    # the generating angles as a caller row on a noise-free target
    clean = synth_job(0, 12, noise=0.0)
    rows = np.random.default_rng(6).uniform(-np.pi, np.pi, size=(2, R)).astype(np.float32)
    rows[1] = clean["true_angles"].astype(np.float32)
    out = optimise(make, place, [clean], "generating angles", init=[rows], popsize=3, maxiter=3, tol=0.0)
    assert out["rmsd"].item() < 1e-4 and out["n_generations"].item() == 3


# ------------------------------------------------------------------ 5. errors
def errors_case(make, place):
    m = model_for(make)
    job = synth_job(0, 12)
    n, R = len(job["start"]), len(job["u"])
    start, target = place(torch.from_numpy(job["start"])), place(torch.from_numpy(job["target"]))
    u, v = place(torch.from_numpy(job["u"])), place(torch.from_numpy(job["v"]))
    mask = place(torch.from_numpy(job["mask"].astype(np.uint8)))
    rmsd = place(torch.zeros(2))
    lig, tor = np.array([0, n], dtype=np.int32), np.array([0, R], dtype=np.int32)
    arr = lambda *x: np.array(x, dtype=np.int32)

    def call(**kw):
        c = L.MatchCfg()
        c.struct_size = ctypes.sizeof(L.MatchCfg)
        c.n_jobs, c.popsize, c.maxiter, c.tol = 1, 2, 1, 0.01
        c.lig_ptr, c.tor_ptr = lig.ctypes.data, tor.ctypes.data
        c.start, c.target, c.rot_u, c.rot_v, c.mask_rotate, c.rmsd = (t.data_ptr() for t in (start, target, u, v, mask, rmsd))
        keep = []
        for k, val in kw.items():
            if isinstance(val, np.ndarray):
                keep.append(val)
                val = val.ctypes.data
            setattr(c, k, val)
        return m.lib.ddmi_match_conformer(m._h, ctypes.byref(c), m._stream())
    assert call() == 0
    for kw in (dict(struct_size=ctypes.sizeof(L.MatchCfg) - 8), dict(start=None), dict(target=None), dict(lig_ptr=None), dict(tor_ptr=None),
               dict(n_jobs=0), dict(lig_ptr=arr(1, n)), dict(tor_ptr=arr(1, R)), dict(n_jobs=2, lig_ptr=arr(0, n, n - 1), tor_ptr=arr(0, R, R)),
               dict(n_jobs=2, lig_ptr=arr(0, 6, n), tor_ptr=arr(0, R, R - 1)), dict(n_jobs=2, lig_ptr=arr(0, n, n), tor_ptr=arr(0, R, R)),
               dict(rot_u=None), dict(rot_v=None), dict(mask_rotate=None), dict(popsize=0), dict(maxiter=-1), dict(tol=-0.5), dict(tol=float("nan")),
               dict(n_init=-1), dict(n_init=1)):
        rc = call(**kw)
        assert rc == -1, (kw, rc)                                   # DDMI_ERR_ARG
        with pytest.raises(L.DdmiError, match="ddmi error -1: ddmi_match_cfg"):
            L.check(m.lib, rc)
    args = dict(rot_u=u, rot_v=v, mask_rotate=mask)
    for kw in (dict(popsize=0), dict(maxiter=-1), dict(tol=-1.0)):  # through the wrapper
        with pytest.raises(L.DdmiError, match="ddmi error -1: ddmi_match_cfg"):
            m.match_conformer(start, target, lig, tor, **args, **kw)
    with pytest.raises(L.DdmiError, match="ddmi error -1"):
        m.match_conformer(start, target, lig, tor, popsize=2, maxiter=1)          # rotatable bonds without their tables
    with pytest.raises(L.DdmiError, match="limits are 256 and 64"):
        m.match_conformer(torch.zeros(257, 3), torch.zeros(257, 3), [0, 257], popsize=2, maxiter=1)
    with pytest.raises(ValueError, match="target"):
        m.match_conformer(start, target[:5], lig, tor, **args)
    with pytest.raises(ValueError, match="start"):
        m.match_conformer(start[:5], target[:5], lig, tor, **args)
    with pytest.raises(ValueError, match="rot_u"):
        m.match_conformer(start, target, lig, tor, rot_u=u[:1], rot_v=v, mask_rotate=mask)
    with pytest.raises(ValueError, match="mask_rotate"):
        m.match_conformer(start, target, lig, tor, rot_u=u, rot_v=v, mask_rotate=mask[:1])
    with pytest.raises(ValueError, match="init_angles"):
        m.match_conformer(start, target, lig, tor, **args, init_angles=torch.zeros(R + 1), n_init=1)
    with pytest.raises(ValueError, match="job_ids"):
        m.match_conformer(start, target, lig, tor, **args, job_ids=[0, 1])


# ------------------------------------------------------------------ 6. quality against the reference's algorithm
QUALITY_MARGIN = 1.02


def fixture_jobs():
    fx = load_fixture("conformer_matching")
    jobs = [dict(start=j["start"].numpy(), target=j["target"].numpy(), u=j["rot_u"].numpy(), v=j["rot_v"].numpy(), mask=j["mask"].numpy().astype(bool),
                 host=float(j["host_rmsd"]), name=j["name"]) for j in fx["jobs"]]
    return fx, jobs


def quality_same_budget_case(make, place):
    """(a) R <= 8 at the host's budget 40 / 40, tol 0.01, seeds 0, 1, 2: every run within QUALITY_MARGIN of the host value."""
    fx, jobs = fixture_jobs()
    jobs = [j for j in jobs if len(j["u"]) <= 8]
    assert [(len(j["start"]), len(j["u"])) for j in jobs] == [(30, 7), (30, 5), (30, 7), (20, 7), (20, 8)]
    worst = 0.0
    for seed in (0, 1, 2):
        out = optimise(make, place, jobs, f"quality (a) seed {seed}", popsize=40, maxiter=40, tol=0.01, seed=seed)
        ratio = out["rmsd"].cpu().numpy().astype(np.float64) / np.array([j["host"] for j in jobs])
        print(f"quality (a) seed {seed} (scipy {fx['scipy']}): device / host = " + ", ".join(f"{j['name']} {r:.4f}" for j, r in zip(jobs, ratio))
              + f"; generations {out['n_generations'].cpu().tolist()}")
        worst = max(worst, ratio.max())
    assert worst <= QUALITY_MARGIN, worst


def quality_long_budget_case(make, place):
    """(b) R = 11 at 40 / 200 with tol 0 against the host's 40 / 40 value."""
    fx, jobs = fixture_jobs()
    jobs = [j for j in jobs if len(j["u"]) == 11]
    assert len(jobs) == 1 and len(jobs[0]["start"]) == 30
    out = optimise(make, place, jobs, "quality (b)", popsize=40, maxiter=200, tol=0.0, seed=0)
    ratio = out["rmsd"].item() / jobs[0]["host"]
    print(f"quality (b) (scipy {fx['scipy']}): device 40/200 {out['rmsd'].item():.4f} / host 40/40 {jobs[0]['host']:.4f} = {ratio:.4f}")
    assert ratio <= QUALITY_MARGIN, ratio


# ------------------------------------------------------------------ 7. match_conformers and complex_graph
def tries_case(make, place):
    m = model_for(make)
    lig = ligand(2, 30)
    tries = [twisted(lig, 40 + t) for t in range(3)]
    target = tries[0]["target"]
    starts = np.stack([_torsion_update_numpy(lig["start"].astype(np.float64), list(zip(lig["u"], lig["v"])), lig["mask"], t["true_angles"]).astype(np.float32)
                       for t in tries])
    table = (lig["u"], lig["v"], lig["mask"])
    res = match_conformers([(table, place(torch.from_numpy(starts)), target)], m, popsize=4, maxiter=4, tol=0.0, seed=1)[0]
    single = [run(make, place, [dict(lig, start=starts[t], target=target)], popsize=4, maxiter=4, tol=0.0, seed=1, job_ids=[t]) for t in range(3)]
    rmsds = torch.stack([s["rmsd"][0] for s in single])
    assert torch.equal(res["rmsds"], rmsds) and int(res["best"]) == int(rmsds.argmin())
    b = int(rmsds.argmin())
    assert torch.equal(res["pos"], single[b]["pos"]) and torch.equal(res["angles"], single[b]["angles"]) and res["rmsd"].item() == rmsds.min().item()
    assert res["pos"].device == single[0]["pos"].device


def _files(tmp):
    data = os.path.join(ROOT, "tests", "golden", "1a0q")
    for name in ("1a0q_protein_processed.pdb", "1a0q_ligand.sdf"):
        with gzip.open(os.path.join(data, name + ".gz"), "rb") as src, open(os.path.join(tmp, name), "wb") as dst:
            dst.write(src.read())
    return os.path.join(tmp, "1a0q_protein_processed.pdb"), os.path.join(tmp, "1a0q_ligand.sdf")


def complex_graph_case(make, place, tmp, device_route=True):
    from diffdock_amd.io import complex_graph, read_sdf
    pdb, sdf = _files(str(tmp))
    plain = complex_graph(pdb, sdf, lm_dim=0, model=model_for(make) if device_route else None)
    assert "rmsd_matching" not in plain and "orig_pos" not in plain["ligand"]
    u, v, mask = torsion_table(plain)
    lc = read_sdf(sdf)[0]
    ang = np.random.default_rng(11).uniform(-np.pi, np.pi, size=len(u))
    conf = _torsion_update_numpy(np.asarray(lc, dtype=np.float64), list(zip(u, v)), mask, ang)
    conf = conf - conf.mean(0)                                    # a generated conformer has a frame of its own
    kw = dict(model=model_for(make), matching_popsize=4, matching_maxiter=6) if device_route else dict(matching_popsize=2, matching_maxiter=2)
    g = complex_graph(pdb, sdf, lm_dim=0, conformers=[conf], **kw)
    assert np.array_equal(np.asarray(g["ligand"].orig_pos), np.asarray(lc)) and isinstance(g.rmsd_matching, float)
    assert g["ligand"].pos.dtype == torch.float32 and g["ligand"].pos.shape == plain["ligand"].pos.shape
    want = rmsd_of_e(restated_e(g["ligand"].pos.numpy()[None], plain["ligand"].pos.numpy()[None]), len(lc))[0, 0, 0]
    assert abs(want - g.rmsd_matching) <= OBJ_ATOL + OBJ_RTOL * want, (want, g.rmsd_matching)
    plain_rmsd = np.sqrt(((g["ligand"].pos.numpy().astype(np.float64) - plain["ligand"].pos.numpy()) ** 2).sum(-1).mean())
    assert abs(plain_rmsd - g.rmsd_matching) <= 1e-4, (plain_rmsd, g.rmsd_matching)   # the conformer sits in the frame of the file's pose
    unmatched = rmsd_of_e(restated_e(conf[None].astype(np.float32), plain["ligand"].pos.numpy()[None]), len(lc))[0, 0, 0]
    assert g.rmsd_matching < unmatched
    assert torch.equal(g["ligand"].edge_mask, plain["ligand"].edge_mask) and np.array_equal(g["ligand"].mask_rotate[0], plain["ligand"].mask_rotate[0])
    assert torch.equal(g["ligand"].x, plain["ligand"].x)
    for store in ("receptor",):
        for key in ("x", "pos", "side_chain_vecs"):
            assert torch.equal(g[store][key], plain[store][key]), key
    assert torch.equal(g["receptor", "rec_contact", "receptor"].edge_index, plain["receptor", "rec_contact", "receptor"].edge_index)
    assert torch.equal(g.original_center, plain.original_center)
