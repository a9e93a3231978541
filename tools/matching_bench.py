#!/usr/bin/env python
"""Time of conformer matching: the device call (matching.match_conformers -> ddmi_match_conformer, every (ligand, try) one job of ONE
call) against the host route (matching.match_conformers_host: scipy.optimize.differential_evolution as the reference's
optimize_rotatable_bonds calls it, one try at a time) on the same jobs.

    python tools/matching_bench.py [--workload one|batch] [--popsize 40] [--maxiter 40] [--reps 9] [--warmup 2] [--host-jobs N]

  one     one job: the ligand of tests/golden/1a0q, started from a seeded twist of the file's pose in a frame of its own
  batch   256 jobs: 64 synth.make_complex ligands (30 atoms) x 4 tries, each try a seeded twist; the target is another seeded
          twist plus Gaussian noise of 0.3 A

  device  median of --reps calls after --warmup; the clock stops after a device synchronisation
  host    the first --host-jobs ligands (default: 1 for `one`, 2 for `batch`; every try of them), timed once -- at 1-6 s per try the
          whole batch is minutes; "host_ms_per_job" is that time per (ligand, try), "speedup_per_job" compares it with device_ms / jobs

One JSON line.  Information only: nothing in the suite depends on these numbers."""
import argparse
import gzip
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffdock_amd.config import TINY  # noqa: E402
from diffdock_amd.matching import match_conformers, match_conformers_host, torsion_table, torsions  # noqa: E402
from diffdock_amd.model import MIScoreModel  # noqa: E402
from diffdock_amd.synth import make_complex  # noqa: E402


def twist(pos, table, rng):
    return torsions(pos, *table, rng.uniform(-np.pi, np.pi, size=len(table[0])))


def jobs_one():
    from diffdock_amd.io import complex_graph
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("1a0q_protein_processed.pdb", "1a0q_ligand.sdf"):
            with gzip.open(os.path.join(ROOT, "tests", "golden", "1a0q", name + ".gz"), "rb") as src, open(os.path.join(tmp, name), "wb") as dst:
                dst.write(src.read())
        g = complex_graph(os.path.join(tmp, "1a0q_protein_processed.pdb"), os.path.join(tmp, "1a0q_ligand.sdf"), lm_dim=0)
    table, target = torsion_table(g), g["ligand"].pos.numpy()
    start = twist(target, table, np.random.default_rng(0))
    return [(table, (start - start.mean(0)).astype(np.float32)[None], target)]


def jobs_batch(ligands=64, tries=4, n=30):
    out = []
    for seed in range(ligands):
        g = make_complex(seed, n_res=20, n_lig=n)
        table, pos = torsion_table(g), g["ligand"].pos.numpy()
        rng = np.random.default_rng(1000 + seed)
        target = (twist(pos, table, rng) + 0.3 * rng.normal(size=pos.shape)).astype(np.float32)
        out.append((table, np.stack([twist(pos, table, rng) for _ in range(tries)]).astype(np.float32), target))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="batch", choices=("one", "batch"))
    ap.add_argument("--popsize", type=int, default=40)
    ap.add_argument("--maxiter", type=int, default=40)
    ap.add_argument("--tol", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-jobs", type=int, default=None)
    args = ap.parse_args()
    jobs = jobs_one() if args.workload == "one" else jobs_batch()
    n_jobs = sum(len(j[1]) for j in jobs)
    m = MIScoreModel(TINY, device="cuda:0")          # matching needs a handle only: no weights, tables or complex
    res = None
    ts = []
    for r in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = match_conformers(jobs, m, popsize=args.popsize, maxiter=args.maxiter, tol=args.tol)
        torch.cuda.synchronize()
        if r >= args.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    d_ms = statistics.median(ts)
    # evaluations of the device call: P for the initial population and P per generation run
    lig = np.cumsum([0] + [len(j[2]) for j in jobs for _ in j[1]])
    tor = np.cumsum([0] + [len(j[0][0]) for j in jobs for _ in j[1]])
    cat = lambda parts, dt: torch.from_numpy(np.concatenate(parts).astype(dt))
    raw = m.match_conformer(cat([s for j in jobs for s in j[1]], np.float32), cat([j[2] for j in jobs for _ in j[1]], np.float32), lig, tor,
                            rot_u=cat([j[0][0] for j in jobs for _ in j[1]], np.int32), rot_v=cat([j[0][1] for j in jobs for _ in j[1]], np.int32),
                            mask_rotate=cat([j[0][2].reshape(-1) for j in jobs for _ in j[1]], np.uint8), popsize=args.popsize,
                            maxiter=args.maxiter, tol=args.tol)
    P = np.maximum(5, args.popsize * np.diff(tor))
    d_evals = int(np.sum(P * (1 + raw["n_generations"].cpu().numpy())))
    host_n = args.host_jobs if args.host_jobs is not None else (1 if args.workload == "one" else 2)
    sub = jobs[:host_n]
    t0 = time.perf_counter()
    host = match_conformers_host(sub, popsize=args.popsize, maxiter=args.maxiter)
    h_ms = (time.perf_counter() - t0) * 1e3
    h_jobs = sum(len(j[1]) for j in sub)
    rmsds = [(round(float(res[i]["rmsd"]), 4), round(host[i]["rmsd"], 4)) for i in range(len(sub))]
    print(json.dumps({"workload": args.workload, "jobs": n_jobs, "popsize": args.popsize, "maxiter": args.maxiter, "device_ms": round(d_ms, 3),
                      "device_evaluations": d_evals, "device_ms_per_job": round(d_ms / n_jobs, 4), "host_jobs": h_jobs, "host_ms": round(h_ms, 1),
                      "host_evaluations": int(sum(h["evaluations"] for h in host)), "host_ms_per_job": round(h_ms / h_jobs, 1),
                      "speedup_per_job": round(h_ms / h_jobs / (d_ms / n_jobs), 1), "rmsd_device_host": rmsds}))


if __name__ == "__main__":
    main()
