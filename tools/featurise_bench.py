#!/usr/bin/env python
"""Time of building the two receptor neighbour graphs of an all-atom complex (residues: 15 A / 24 neighbours, atoms: 5 A / 8): the
host routes against one ddmi_neighbor_graph call on the device.

    python tools/featurise_bench.py [--reps R] [--warmup W] [--skip-large-host]

Inputs: the stored 1a0q complex (416 residues, 3181 atoms) and a synthetic 1500-residue receptor of diffdock_amd.synth (about
12 000 atoms).

  reference_ms  the reference's route (datasets/process_mols.py:171-192, 207-228) as diffdock_amd.io.receptor_graph restates it: a
                dense float32 torch.cdist matrix per graph, then a Python loop with one np.where and, where the cap binds, one
                np.argsort over a full row per node
  host_ms       diffdock_amd.io.neighbor_graph without a model: the float64 restatement of the device rule, in row blocks
  device_ms     MIScoreModel.neighbor_graph: both graphs in ONE ragged call (coordinates already on the device), the edge total read
                back to shape the result; the clock stops after a device synchronisation
  enqueue_ms    the C call alone on preallocated outputs (no read-back): count, scan and fill enqueued, then a synchronisation

`columns_differing_from_float64` compares the device with the float64 restatement: 0 on 1a0q; the synthetic chain has equal 3.8 A steps,
i.e. neighbour distances that tie in float64 to the last bits, and differs only in the order of such pairs (rows under the decision
margin of tests/neighbor_cases.py).

One JSON line per input (medians).  Information only: nothing in the suite depends on these numbers."""
import argparse
import ctypes
import gzip
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diffdock_amd.lib as L  # noqa: E402
from diffdock_amd import io as dio  # noqa: E402
from diffdock_amd.config import TINY  # noqa: E402
from diffdock_amd.model import MIScoreModel  # noqa: E402
from diffdock_amd.synth import make_complex  # noqa: E402

REC, ATOM = (15.0, 24), (5.0, 8)


def inputs():
    with tempfile.TemporaryDirectory() as tmp:
        pdb = os.path.join(tmp, "p.pdb")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "1a0q", "1a0q_protein_processed.pdb.gz"), "rb") as src, open(pdb, "wb") as dst:
            shutil.copyfileobj(src, dst)
        table, _ = dio.read_pdb_atoms(pdb)
    flat = table.reshape(-1, 3)
    yield "1a0q", table[:, 1].astype(np.float32), flat[~np.isnan(flat).any(1)].astype(np.float32)
    g = make_complex(seed=1, n_res=1500, n_lig=10, lm_dim=0, all_atoms=True, atoms_per_res=(6, 11))
    yield "synth1500", g["receptor"].pos.numpy(), g["atom"].pos.numpy()


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-large-host", action="store_true", help="no host routes for the synthetic receptor (tens of seconds)")
    args = ap.parse_args()
    m = MIScoreModel(TINY, device="cuda:0")          # a handle only: no weights, tables or complex
    for name, rc, ac in inputs():
        n_res, n_atom = len(rc), len(ac)
        ptr = np.asarray([0, n_res, n_res + n_atom], dtype=np.int32)
        pos = torch.from_numpy(np.concatenate([rc, ac])).to("cuda:0")
        cut, cap = np.asarray([REC[0], ATOM[0]], dtype=np.float32), np.asarray([REC[1], ATOM[1]], dtype=np.int32)

        def device():
            out = m.neighbor_graph(pos, (REC[0], ATOM[0]), (REC[1], ATOM[1]), ptr=ptr)
            torch.cuda.synchronize()
            return out[0]
        capacity = n_res * REC[1] + n_atom * ATOM[1]
        edge = torch.empty(2, capacity, dtype=torch.int64, device="cuda:0")
        deg = torch.empty(n_res + n_atom, dtype=torch.int32, device="cuda:0")
        n_edges = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        c = L.NeighborGraphCfg()
        c.struct_size, c.n_nodes, c.n_sets, c.capacity = ctypes.sizeof(L.NeighborGraphCfg), n_res + n_atom, 2, capacity
        c.pos, c.ptr, c.set_cutoff, c.set_max_neighbors = pos.data_ptr(), ptr.ctypes.data, cut.ctypes.data, cap.ctypes.data
        c.deg, c.edge_index, c.n_edges = deg.data_ptr(), edge.data_ptr(), n_edges.data_ptr()

        def enqueue():
            L.check(m.lib, m.lib.ddmi_neighbor_graph(m._h, ctypes.byref(c), m._stream()))
            torch.cuda.synchronize()
        d_ms, d_out = timed(device, args.reps, args.warmup)
        e_ms, _ = timed(enqueue, args.reps, args.warmup)
        assert int(n_edges.item()) == d_out.shape[1] and torch.equal(edge[:, :d_out.shape[1]], d_out)
        row = {"input": name, "residues": n_res, "atoms": n_atom, "edges": int(d_out.shape[1]), "device_ms": round(d_ms, 3),
               "enqueue_ms": round(e_ms, 3)}
        if name == "1a0q" or not args.skip_large_host:
            reps = args.reps if name == "1a0q" else 1
            r_ms, _ = timed(lambda: (dio.receptor_graph(rc, *REC), dio.receptor_graph(ac, *ATOM)), reps, 0)
            h_ms, h_out = timed(lambda: (dio.neighbor_graph(rc, *REC), dio.neighbor_graph(ac, *ATOM)), reps, 0)
            host_edges = np.concatenate([h_out[0], h_out[1] + n_res], axis=1)
            row.update(reference_ms=round(r_ms, 1), host_ms=round(h_ms, 1), speedup_vs_reference=round(r_ms / d_ms, 1),
                       columns_differing_from_float64=int((host_edges != d_out.cpu().numpy()).any(0).sum())
                       if host_edges.shape == tuple(d_out.shape) else -1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
