#!/usr/bin/env python
"""The first launches of each kind in a forward (layer 0: four k_conv_fused / k_edge_hidden_mm, eight k_gemm_nt_batch, one k_reduce_bn)
over the last 10 forwards of a rocprofv3 --kernel-trace rocpd database (forwards delimited by k_perturb): workgroups, stream, mean
duration, plus the per-forward kernel sums.  usage: layer0_launches.py results.db > table.txt"""
import re, sqlite3, sys
from collections import defaultdict
db = sqlite3.connect(sys.argv[1])
rows = db.execute("""select d.start, d.end, s.kernel_name, d.grid_size_x, d.grid_size_y, d.grid_size_z, d.workgroup_size_x, d.workgroup_size_y, d.stream_id
                     from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id order by d.start""").fetchall()
short = lambda n: (re.search(r"k_[a-z0-9_]+", n) or [n[:30]])[0]
marks = [r[0] for r in rows if "k_perturb" in r[2]]
nf = 10
acc = defaultdict(list)
for f in range(nf):
    t0, t1 = marks[-nf - 2 + f], marks[-nf - 1 + f]
    fw = [r for r in rows if t0 < r[0] < t1]
    seen = defaultdict(int)
    for a, b, n, gx, gy, gz, wx, wy, st in fw:
        k = short(n)
        if k not in ("k_conv_fused", "k_edge_hidden_mm", "k_reduce_bn", "k_gemm_nt_batch", "k_vn_lists", "k_vn_rows_grouped"): continue
        i = seen[k]; seen[k] += 1
        lim = {"k_conv_fused": 4, "k_edge_hidden_mm": 4, "k_reduce_bn": 1, "k_gemm_nt_batch": 8}.get(k, 1)
        if i >= lim: continue
        wgs = (gx // wx) * (gy // max(wy, 1)) * gz
        acc[(k, i)].append((wgs, st, (b - a) / 1e3))
    totals = defaultdict(float)
    for a, b, n, *_ in fw: totals[short(n)] += (b - a) / 1e3
    acc[("fwd_wall_us", 0)].append((0, 0, (t1 - t0) / 1e3))
    for k in ("k_conv_fused", "k_edge_hidden_mm", "k_reduce_bn"): acc[(k + " (sum/forward)", 0)].append((0, 0, totals[k]))
print(f"{'launch (order in forward)':34s} {'workgroups':>10s} {'stream':>6s} {'mean us':>9s}   (last {nf} forwards)")
for (k, i), v in sorted(acc.items(), key=lambda x: (x[0][0], x[0][1])):
    print(f"{k + ' #' + str(i):34s} {v[0][0]:10d} {v[0][1]:6d} {sum(x[2] for x in v) / len(v):9.1f}")
