#!/usr/bin/env python
"""poses/s of bench.py's all-atom workload (configs2 --all_atoms: 20 steps x 40 poses, 300 residues / 30 atoms) with and without the
per-step receptor crop of the device loop (crop_beyond = 20: cutoff 3 sigma_tr(t) + 20 A), and what the crop costs when it drops
nothing (a cutoff beyond the receptor: same edges, crop kernels on).  bench.py itself measures the no-crop path and stays as it is;
this driver builds the same inputs through bench.py's own helpers -- only the initial poses are drawn inside the pocket (a small
initial_noise_std_proportion), so that residues really are cropped once sigma has fallen -- and times the same call:

    python tools/aa_crop_bench.py [--steps K] [--warmup W] [--samples S] [--crop 20] [--noise 0.05]

One JSON line: {"no_crop", "crop", "crop_keeps_all" (poses/s), "kept" (per step of the cropped loop: residues, atoms and atom-atom
edges kept, as fractions of the uncropped batch, from the recorded poses), "crop_kernels" (ddmi_kernel_timings rows of the crop's own
kernels and the list builds, ms per forward, from one extra timed run of the cropped and of the uncropped loop)}."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from diffdock_amd.hetero import HeteroBatch  # noqa: E402
from diffdock_amd.model import MIScoreModel  # noqa: E402
from diffdock_amd.synth import make_complex, make_pose_list  # noqa: E402
from diffdock_amd.tables import default_tables  # noqa: E402
from diffdock_amd.weights import init_state_dict  # noqa: E402

CROP_ROWS = ("k_crop_mask", "k_rel_filter", "vn_build", "forward_total")


def kept_per_step(cfg, g, pos_before, sched, crop):
    """Residues, atoms and atom-atom edges the crop keeps at every step, summed over the poses, as fractions (utils/utils.py:391-410 on
    the host, from the pose every step started at)."""
    rec = g["receptor"].pos
    res_of = g["atom", "receptor"].edge_index[1]
    aa = g["atom", "atom"].edge_index
    out = []
    for k, t in enumerate(sched):
        cutoff = 3 * cfg.tr_sigma_min ** (1 - t) * cfg.tr_sigma_max ** t + crop
        keep = (torch.cdist(pos_before[k], rec[None]) < cutoff).any(1)          # [S, n_res]
        akeep = keep[:, res_of]
        out.append(dict(step=k, cutoff=round(float(cutoff), 2), residues=round(float(keep.float().mean()), 4),
                        atoms=round(float(akeep.float().mean()), 4),
                        atom_edges=round(float((akeep[:, aa[0]] & akeep[:, aa[1]]).float().mean()), 4)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--samples", type=int, default=None)
    ap.add_argument("--crop", type=float, default=20.0)
    ap.add_argument("--noise", type=float, default=0.05, help="initial_noise_std_proportion of the initial poses")
    args = ap.parse_args()
    cfg = bench.bench_cfg().replace(all_atoms=True)
    wl = bench.WORKLOADS["configs2"]
    n_res, n_lig, cseed = wl["complexes"][0]
    S = args.samples or wl["samples"]
    m = MIScoreModel(cfg, device="cuda:0")
    m.load_state_dict(init_state_dict(cfg, seed=1234))
    m.set_tables(*default_tables())
    g = make_complex(seed=cseed, n_res=n_res, n_lig=n_lig, all_atoms=True)
    dl = make_pose_list(g, S, tr_sigma_max=cfg.tr_sigma_max, seed=1000, initial_noise_std_proportion=args.noise)
    batch = HeteroBatch.from_data_list(dl).to("cuda:0")
    K = bench.INFERENCE_STEPS
    sched = bench.t_schedule(K)
    run = lambda seed, crop, rec=None: m.sample_batch(batch, K, (sched, sched, sched), seed=seed, sample_ids=list(range(S)),
                                                      no_final_step_noise=True, crop_beyond=crop, record=rec, **bench.TEMP)

    def poses_per_s(crop):
        for w in range(args.warmup):
            run(w, crop)
        torch.cuda.synchronize()
        t0 = time.time()
        for k in range(args.steps):
            run(100 + k, crop)
        torch.cuda.synchronize()
        return round(S * args.steps / (time.time() - t0), 3)

    def timed_rows(crop):
        m.set_kernel_timing(True, 1)
        run(100, crop)
        torch.cuda.synchronize()
        rows = m.kernel_timings()
        m.set_kernel_timing(False)
        return {k: round(rows[k][0] / K, 4) for k in CROP_ROWS if k in rows}

    arms = {"no_crop": poses_per_s(None), "crop": poses_per_s(args.crop), "crop_keeps_all": poses_per_s(1e4)}
    pos, rec = run(100, args.crop, {"pos"})
    n = n_lig
    before = torch.cat([batch["ligand"].pos.reshape(1, S, n, 3), rec.pos.reshape(K, S, n, 3)[:-1]]).cpu()
    print(json.dumps(dict(arms, unit="poses/s", samples=S, steps=K, crop_beyond=args.crop, noise=args.noise,
                          n_res=n_res, n_atoms=int(g["atom"].pos.shape[0]), n_atom_edges=int(g["atom", "atom"].edge_index.shape[1]),
                          finite=bool(torch.isfinite(pos).all()), kept=kept_per_step(cfg, g, before, sched, args.crop),
                          crop_kernels={"crop": timed_rows(args.crop), "crop_keeps_all": timed_rows(1e4), "no_crop": timed_rows(None)})))


if __name__ == "__main__":
    main()
