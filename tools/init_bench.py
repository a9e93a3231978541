#!/usr/bin/env python
"""Wall time from one complex graph to N sampled poses, the host preparation included -- what bench.py leaves out because its
inputs are resident.  Two arms on bench.py's default complex (300 residues / 30 atoms) and model:

  (a) clones     N graph clones + synth.randomize_position (host numpy per pose) + HeteroBatch.from_data_list + upload +
                 MIScoreModel.sample_batch                                   (inference.py:239-242 followed by sampling())
  (b) replicate  sampling.sample_poses: HeteroBatch.replicate on the device, initial poses drawn by ddmi_randomize_position,
                 the same step loop

    python tools/init_bench.py [--poses N] [--steps K] [--reps R] [--warmup W]

Both arms synchronise the device before the clock starts and before it stops.  The two arms draw DIFFERENT initial poses (a host
generator against the library's counter-based one), so their final poses differ; the step loop does the same work per pose.
One JSON line: {"poses", "steps", "clones_ms", "replicate_ms", "speedup"} (medians over the repetitions)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from diffdock_amd.hetero import HeteroBatch  # noqa: E402
from diffdock_amd.model import MIScoreModel  # noqa: E402
from diffdock_amd.sampling import sample_poses  # noqa: E402
from diffdock_amd.synth import make_complex, randomize_position  # noqa: E402
from diffdock_amd.tables import default_tables  # noqa: E402
from diffdock_amd.weights import init_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=40)
    ap.add_argument("--steps", type=int, default=bench.INFERENCE_STEPS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    cfg = bench.bench_cfg()
    n_res, n_lig, cseed = bench.WORKLOADS["configs2"]["complexes"][0]
    N = args.poses
    m = MIScoreModel(cfg, device="cuda:0")
    m.load_state_dict(init_state_dict(cfg, seed=1234))
    m.set_tables(*default_tables())
    g = make_complex(seed=cseed, n_res=n_res, n_lig=n_lig)
    sched = bench.t_schedule(args.steps)
    loop = dict(no_final_step_noise=True, **bench.TEMP)

    def clones(seed):
        dl = randomize_position([g.clone() for _ in range(N)], cfg.no_torsion, False, cfg.tr_sigma_max,
                                initial_noise_std_proportion=0.3, seed=seed)
        batch = HeteroBatch.from_data_list(dl).to("cuda:0")
        return m.sample_batch(batch, args.steps, (sched, sched, sched), seed=seed, sample_ids=list(range(N)), **loop)

    def replicate(seed):
        return sample_poses(g, N, m, args.steps, sched, sched, sched, model_args=cfg, batch_size=N, seed=seed,
                            initial_noise_std_proportion=0.3, **loop)[0]

    def timed(fn):
        for w in range(args.warmup):
            fn(w)
        ts = []
        for k in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(100 + k)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            assert bool(torch.isfinite(out).all())
        return statistics.median(ts)
    a, b = timed(clones), timed(replicate)
    print(json.dumps({"poses": N, "steps": args.steps, "clones_ms": round(a, 2), "replicate_ms": round(b, 2),
                      "speedup": round(a / b, 3),
                      "note": "host preparation included in both arms; the arms draw different initial poses"}))


if __name__ == "__main__":
    main()
