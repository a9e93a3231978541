#!/usr/bin/env python
"""poses/s of bench.py's default workload (configs2: 20 steps x 40 poses, 300 residues / 30 atoms) with the per-step record of
the device loop switched on or off -- the record-on arm of an A/B (none is on file yet).  bench.py itself measures the record-off path
and stays as it is; this driver builds the same inputs through bench.py's own helpers and times the same call:

    python tools/record_bench.py [--record all|pos|nan|off] [--steps K] [--warmup W]

One JSON line: {"record", "value" (poses/s), "ms_per_step", "bitwise_equal_to_record_off"}."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", default="all", choices=["all", "pos", "nan", "off"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    record = {"all": True, "pos": {"pos"}, "nan": {"nan"}, "off": None}[args.record]
    cfg = bench.bench_cfg()
    wl = bench.WORKLOADS["configs2"]
    n_res, n_lig, cseed = wl["complexes"][0]
    S = wl["samples"]
    m = MIScoreModel(cfg, device="cuda:0")
    m.load_state_dict(init_state_dict(cfg, seed=1234))
    m.set_tables(*default_tables())
    g = make_complex(seed=cseed, n_res=n_res, n_lig=n_lig)
    dl = make_pose_list(g, S, tr_sigma_max=cfg.tr_sigma_max, seed=1000, initial_noise_std_proportion=0.3)
    batch = HeteroBatch.from_data_list(dl).to("cuda:0")
    sched = bench.t_schedule(bench.INFERENCE_STEPS)
    run = lambda seed, rec: m.sample_batch(batch, bench.INFERENCE_STEPS, (sched, sched, sched), seed=seed, sample_ids=list(range(S)),
                                           no_final_step_noise=True, record=rec, **bench.TEMP)
    for w in range(args.warmup):
        run(w, record)
    torch.cuda.synchronize()
    t0 = time.time()
    for k in range(args.steps):
        out = run(100 + k, record)
    torch.cuda.synchronize()
    dt = (time.time() - t0) / args.steps
    same = None
    if record is not None:   # the record must not change a pose
        pos, rec = out
        same = bool(torch.equal(pos, run(100 + args.steps - 1, None)))
        if rec.pos is not None:
            same = same and bool(torch.equal(rec.pos[-1], pos))
    print(json.dumps({"record": args.record, "value": round(S / dt, 3), "unit": "poses/s", "ms_per_step": round(dt * 1e3, 3),
                      "bitwise_equal_to_record_off": same}))


if __name__ == "__main__":
    main()
