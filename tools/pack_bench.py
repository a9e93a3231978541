"""A/B of packing several complexes into one device batch (sampling.sample_complexes) against one batch per complex.

Workload: the nine complexes of bench.py's `mix` shapes (Nr in {150, 300, 500} x Nl in {20, 30, 45}) at 10 poses each
(DiffDock-L's samples_per_complex), 20 steps, DiffDock-L temperatures, one model handle.
  Arm A: one sample_batch per complex (inference.py's pattern: sampling() of one complex at a time).
  Arm B: sample_complexes packing whole 10-pose chunks into batches of at most --max-graphs graphs (4 complexes = 40 graphs).
Two rates per arm: the device loop alone (the collated batches are built and ddmi_set_complex has run before the clock starts)
and end to end (collate + ddmi_set_complex / ddmi_set_batch_layout + loop + write-back: sampling() per complex for A,
sample_complexes for B).  Every timing ends with a device synchronise; the arms alternate within one process after a warm-up.

    python tools/pack_bench.py [--reps 5] [--warmup 1] [--max-graphs 40] [--out profiles/pack_ab.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("DDMI_HARNESS", "1")

from diffdock_amd.config import DDL_SYNTH  # noqa: E402
from diffdock_amd.hetero import HeteroBatch  # noqa: E402
from diffdock_amd.model import MIScoreModel  # noqa: E402
from diffdock_amd.sampling import sample_complexes, sampling  # noqa: E402
from diffdock_amd.synth import make_complex, make_pose_list  # noqa: E402
from diffdock_amd.tables import default_tables  # noqa: E402
from diffdock_amd.weights import init_state_dict  # noqa: E402

STEPS = 20
POSES = 10
TEMP = dict(temp_sampling=[1.170050527854316, 2.06391612594481, 7.044261621607846],       # default_inference_args.yaml
            temp_psi=[0.727287304570729, 0.9022615585677628, 0.5946212391366862],
            temp_sigma_data=[0.9299802531572672, 0.7464326999906034, 0.6943254174849822])
MIX = [(nr, nl, 10 + 3 * i + j) for i, nr in enumerate((150, 300, 500)) for j, nl in enumerate((20, 30, 45))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-graphs", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = DDL_SYNTH.replace(dynamic_max_cross=False, cross_max_distance=80.0)   # bench.py's configuration
    m = MIScoreModel(cfg, device=str(dev))
    m.load_state_dict(init_state_dict(cfg, seed=1234))
    m.set_tables(*default_tables())
    sched = np.linspace(1, 0, STEPS + 1)[:-1]
    scheds = (sched, sched, sched)
    lists = [make_pose_list(make_complex(seed=s, n_res=nr, n_lig=nl), POSES, tr_sigma_max=cfg.tr_sigma_max, seed=1000,
                            initial_noise_std_proportion=0.3) for nr, nl, s in MIX]
    n_poses = POSES * len(lists)
    offsets = [POSES * k for k in range(len(lists))]
    kw = dict(seed=7, no_final_step_noise=True, **TEMP)

    # device-loop-only inputs: A = one collated batch per complex, B = whole complexes packed up to --max-graphs graphs
    per = max(1, args.max_graphs // POSES)
    batches_a = [(HeteroBatch.from_data_list(dl).to(dev), list(range(o, o + POSES)), None) for dl, o in zip(lists, offsets)]
    batches_b = []
    for lo in range(0, len(lists), per):
        grp = lists[lo:lo + per]
        batches_b.append((HeteroBatch.from_data_list([g for dl in grp for g in dl]).to(dev),
                          list(range(offsets[lo], offsets[lo] + POSES * len(grp))), [POSES] * len(grp)))

    def loop_only(batches):
        total = 0.0
        for batch, ids, groups in batches:
            m._ensure_complex(batch)          # ddmi_set_complex (+ layout) outside the clock
            m._ensure_layout(groups)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.sample_batch(batch, STEPS, scheds, sample_ids=ids, groups=groups, **kw)
            torch.cuda.synchronize()
            total += time.perf_counter() - t0
        return total

    def end_to_end_a():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for dl, o in zip(lists, offsets):
            sampling([g.clone() for g in dl], m, STEPS, *scheds, device=dev, batch_size=POSES, sample_id_offset=o, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def end_to_end_b():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sample_complexes([[g.clone() for g in dl] for dl in lists], m, STEPS, *scheds, device=dev, batch_size=POSES,
                         max_batch_graphs=args.max_graphs, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    arms = {"A_loop": lambda: loop_only(batches_a), "B_loop": lambda: loop_only(batches_b),
            "A_e2e": end_to_end_a, "B_e2e": end_to_end_b}
    for _ in range(args.warmup):
        for f in arms.values():
            f()
    times = {k: [] for k in arms}
    for _ in range(args.reps):                # alternate the arms inside every repetition
        for k, f in arms.items():
            times[k].append(f())
    lines = [f"pack_bench: {len(lists)} complexes x {POSES} poses, {STEPS} steps, DiffDock-L temperatures, "
             f"B packs <= {args.max_graphs} graphs ({[len(b[1]) for b in batches_b]}); {args.reps} alternating reps after "
             f"{args.warmup} warm-up; {torch.cuda.get_device_name(0)}"]
    res = {}
    for k, ts in times.items():
        ts = np.asarray(ts)
        rate = n_poses / ts
        res[k] = dict(poses_per_s=float(np.median(rate)), min=float(rate.min()), max=float(rate.max()), seconds=ts.tolist())
        lines.append(f"  {k:7s} {np.median(rate):8.2f} poses/s  (min {rate.min():.2f}, max {rate.max():.2f}; median {np.median(ts) * 1e3:.1f} ms)")
    for what in ("loop", "e2e"):
        a, b = res[f"A_{what}"]["poses_per_s"], res[f"B_{what}"]["poses_per_s"]
        lines.append(f"  B / A ({what}): {b / a:.3f}")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
