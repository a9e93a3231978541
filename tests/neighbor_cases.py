"""Cases of the neighbour lists on the device (ddmi_neighbor_graph, MIScoreModel.neighbor_graph, diffdock_amd.io.neighbor_graph).
Run on the CPU emulation build by tests/test_neighbor_emu.py and on the MI355X by tests/test_gpu_neighbor.py through the same C ABI.
`make(cfg, sd)` returns a loaded MIScoreModel, `place` moves a tensor to the model's device.

References: the host restatement `diffdock_amd.io.neighbor_graph(model=None)` -- the same rule in float64 on the same float32
coordinates -- and tests/golden/1a0q_aa_graph.pt, whose atom graphs come from EXECUTING the reference's
new_extract_receptor_structure (tests/golden/make_1a0q_aa.py).

Bound: rows are compared EXACTLY, as ordered lists.  A row may differ from the float64 oracle only if one of its float64 decision gaps
is below MARGIN = 1e-5 A: |d_ij - cutoff| for any j; for a row with more candidates than the cap, the gap between the cap-th and the
next neighbour and the gaps between consecutive kept neighbours.  Derived, not measured: d^2 carries six float32 roundings on top of
exact inputs, a relative error of about 4e-7 on d^2, 2e-7 on d, i.e. about 5e-6 A at 30 A for coordinates below 128 A (1a0q's largest
is 70.4 A).  At most MAX_EXCUSED = 3 rows of an input may use the excuse (on the CPU: 1, 2, 0 and 0 rows of the four 1a0q inputs are
under the margin at all); the small shapes of `SHAPES` have no row under it and none is excused."""
import ctypes
import gzip
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import diffdock_amd.io as dio
import diffdock_amd.lib as L
from diffdock_amd.config import TINY
from diffdock_amd.weights import init_state_dict
from util import GOLDEN, load_fixture

MARGIN = 1e-5
MAX_EXCUSED = 3
_cache = {}


def model_for(make):
    """One handle per runner: ddmi_neighbor_graph needs no complex, weights or tables, any model serves."""
    if ("model", make) not in _cache:
        _cache["model", make] = make(TINY, init_state_dict(TINY, seed=3))
    return _cache["model", make]


def fixture():
    if "fx" not in _cache:
        fx = load_fixture("1a0q_aa_graph")
        _cache["fx"] = {k: (v.long() if torch.is_tensor(v) and v.dtype == torch.int16 else v) for k, v in fx.items()}
    return _cache["fx"]


def calpha():
    """The uncentred C-alpha coordinates of the stored 1a0q file, float32 [416, 3]."""
    if "ca" not in _cache:
        with tempfile.TemporaryDirectory() as tmp:
            pdb = os.path.join(tmp, "p.pdb")
            with gzip.open(os.path.join(GOLDEN, "1a0q", "1a0q_protein_processed.pdb.gz"), "rb") as src, open(pdb, "wb") as dst:
                shutil.copyfileobj(src, dst)
            _cache["ca"] = dio.read_pdb_calpha(pdb)[0].astype(np.float32)
    return _cache["ca"]


INPUTS = {"atoms_5_8": (5.0, 8), "atoms_5_uncapped": (5.0, None), "calpha_15_24": (15.0, 24), "calpha_30_10": (30.0, 10)}


def input_points(name):
    return fixture()["atom_pos_uncentred"].numpy() if name.startswith("atoms") else calpha()


# ------------------------------------------------------------------ rows, oracle, decision gaps
def rows_of(edge_index, n):
    """edge_index [2, E] ordered by centre -> the neighbour list of every node, in stored order."""
    ei = np.asarray(edge_index.cpu() if torch.is_tensor(edge_index) else edge_index)
    assert ei.shape[0] == 2 and (np.diff(ei[1]) >= 0).all(), "edge_index is not ordered by centre"
    cuts = np.searchsorted(ei[1], np.arange(n + 1))
    return [ei[0, cuts[i]:cuts[i + 1]].tolist() for i in range(n)]


def under_margin(x, cutoff, cap, ptr=None):
    """bool [n]: rows with a float64 decision gap below MARGIN (module docstring)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    ptr = [0, len(x)] if ptr is None else ptr
    cap = cap or 1000
    out = np.zeros(len(x), dtype=bool)
    for g in range(len(ptr) - 1):
        lo, hi = ptr[g], ptr[g + 1]
        for b in range(lo, hi, 512):
            rows = np.arange(b, min(b + 512, hi))
            d = np.sqrt(((x[rows, None, :] - x[None, lo:hi, :]) ** 2).sum(-1))
            d[np.arange(len(rows)), rows - lo] = np.inf
            out[rows] = (np.abs(d - cutoff) < MARGIN).any(axis=1)
            for r, i in enumerate(rows):
                inside = np.sort(d[r][d[r] < cutoff])
                if len(inside) > cap and (np.diff(inside[:cap + 1]) < MARGIN).any():
                    out[i] = True
    return out


def oracle(name):
    """(rows of the float64 host restatement, rows under the margin) of a 1a0q input, computed once."""
    if ("oracle", name) not in _cache:
        x, (cutoff, cap) = input_points(name), INPUTS[name]
        _cache["oracle", name] = (rows_of(dio.neighbor_graph(x, cutoff, cap), len(x)), under_margin(x, cutoff, cap))
    return _cache["oracle", name]


def device_rows(make, place, name):
    """The device's rows of a 1a0q input, computed once per runner (cases A and B share them)."""
    if ("device", make, name) not in _cache:
        x, (cutoff, cap) = input_points(name), INPUTS[name]
        ei, deg = model_for(make).neighbor_graph(place(torch.from_numpy(x)), cutoff, cap)
        rows = rows_of(ei, len(x))
        assert deg.cpu().tolist() == [len(r) for r in rows]
        _cache["device", make, name] = rows
    return _cache["device", make, name]


def compare_exact(tag, got, want, excusable, max_excused):
    differing = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    print(f"neighbour lists '{tag}': {len(got)} rows, {int(np.sum(excusable))} under the margin, {len(differing)} differ from float64: {differing[:8]}")
    assert len(got) == len(want)
    assert all(excusable[i] for i in differing), (tag, [(i, got[i], want[i]) for i in differing if not excusable[i]][:4])
    assert len(differing) <= max_excused, (tag, differing)


# ------------------------------------------------------------------ A. exactness against the float64 oracle
def exact_case(make, place, name):
    want, excusable = oracle(name)
    compare_exact(name, device_rows(make, place, name), want, excusable, MAX_EXCUSED)


# ------------------------------------------------------------------ B. against the reference-executed fixture
def fixture_case(make, place, name):
    """Rows as sets: wherever the device differs from the executed reference, the float64 oracle differs from it too (the
    reference's torch.cdist noise, 3e-2 A on this input), or the row is one excused in A."""
    fx = fixture()
    assert "new_extract_receptor_structure(all_atoms=True)" in fx["provenance"]
    n = len(fx["atom_pos_uncentred"])
    ref = [set(r) for r in rows_of(fx["atom_edge_index" if name == "atoms_5_8" else "atom_edge_index_uncapped"], n)]
    want, excusable = oracle(name)
    got = device_rows(make, place, name)
    dev_diff = [i for i in range(n) if set(got[i]) != ref[i]]
    ora_diff = {i for i in range(n) if set(want[i]) != ref[i]}
    print(f"fixture '{name}': the device differs from the executed reference in {len(dev_diff)} rows, float64 in {len(ora_diff)}")
    assert all(i in ora_diff or excusable[i] for i in dev_diff), [i for i in dev_diff if i not in ora_diff and not excusable[i]][:8]


# ------------------------------------------------------------------ C. the smallest shapes that can go wrong
def _normals(n, seed=0):
    return (np.random.default_rng(seed + n).normal(size=(n, 3)) * 6.0).astype(np.float32)


def _lattice():
    return np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def _cluster_and_one():
    x = _normals(40, seed=7)
    x[17] = [300.0, -200.0, 100.0]      # one node far from everything, in the middle of the index range
    return x


SHAPES = {
    "n1": (lambda: np.zeros((1, 3), np.float32), 5.0, 8),
    "n2_apart": (lambda: np.asarray([[0, 0, 0], [20, 0, 0]], np.float32), 5.0, 8),                    # nearest-other fallback
    "n63": (lambda: _normals(63), 5.0, 8), "n64": (lambda: _normals(64), 5.0, 8),                     # wave boundaries
    "n65": (lambda: _normals(65), 5.0, 8), "n129": (lambda: _normals(129), 5.0, 8),
    "cap1": (lambda: _normals(65, seed=1), 5.0, 1),
    "cap_never_binds": (lambda: _normals(65, seed=2), 5.0, 64),                                      # cap >= n - 1
    "uncapped": (lambda: _normals(129, seed=3), 8.0, None),
    "lattice_ties": (_lattice, 1.5, 4),                                                               # exact ties go to the lower index
    "identical_pair": (lambda: np.asarray([[1, 2, 3], [1, 2, 3], [1, 2, 4.5], [9, 9, 9]], np.float32), 2.0, 8),
    "isolated_in_cluster": (_cluster_and_one, 5.0, 8),
    "overflow_4500": (lambda: (np.random.default_rng(11).normal(size=(4500, 3)) * 20.0).astype(np.float32), 1000.0, 8),
}


def shape_case(make, place, name):
    build, cutoff, cap = SHAPES[name]
    x = build()
    n = len(x)
    ei, deg = model_for(make).neighbor_graph(place(torch.from_numpy(x)), cutoff, cap)
    got = rows_of(ei, n)
    assert deg.cpu().tolist() == [len(r) for r in got] and ei.dtype == torch.int64 and deg.dtype == torch.int32
    assert all(i not in r for i, r in enumerate(got)), "a node is its own neighbour"
    if name == "overflow_4500":     # (the oracle's only large case: every row keeps the 8 nearest of 4499)
        excusable = _overflow_margin(x, cap)
    else:
        excusable = under_margin(x, cutoff, cap)
    if name != "lattice_ties":      # (the lattice's ties are exact in float32 and float64 alike: integer coordinates)
        assert not excusable.any(), (name, np.nonzero(excusable)[0][:8])   # the shape was chosen so: nothing to excuse
    compare_exact(name, got, rows_of(dio.neighbor_graph(x, cutoff, cap), n), np.zeros(n, dtype=bool), 0)
    if name == "n1":
        assert ei.shape == (2, 0)
    if name == "n2_apart":
        assert got == [[1], [0]]
    if name == "identical_pair":
        assert got[0] == [1, 2] and got[1] == [0, 2] and got[3] == [2]
    if name == "lattice_ties":      # the corner 0 has three neighbours at distance 1 and three at sqrt(2): 1, 4, 16 then 5 (the lowest)
        assert got[0] == [1, 4, 16, 5]
    if name == "isolated_in_cluster":
        assert len(got[17]) == 1


def _overflow_margin(x, cap):
    x = x.astype(np.float64)
    out = np.zeros(len(x), dtype=bool)
    for b in range(0, len(x), 500):
        d = np.sqrt(((x[b:b + 500, None] - x[None]) ** 2).sum(-1))
        d[np.arange(d.shape[0]), np.arange(b, b + d.shape[0])] = np.inf
        nearest = np.sort(np.partition(d, cap + 1, axis=1)[:, :cap + 1], axis=1)
        out[b:b + 500] = (np.diff(nearest, axis=1) < MARGIN).any(axis=1)
    return out


# ------------------------------------------------------------------ D. independence
def independence_case(make, place):
    """A set's rows are bit-identical alone, in a ragged call and after permuting the sets of the call."""
    m = model_for(make)
    sets = [_normals(40, seed=21), calpha(), _normals(65, seed=22)]
    cutoff, cap = 15.0, 10
    alone = [m.neighbor_graph(place(torch.from_numpy(s)), cutoff, cap) for s in sets]
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        xs = [sets[k] for k in order]
        ptr = np.concatenate([[0], np.cumsum([len(s) for s in xs])])
        ei, deg = m.neighbor_graph(place(torch.from_numpy(np.concatenate(xs))), cutoff, cap, ptr=ptr)
        assert (ei[1, 1:] >= ei[1, :-1]).all()
        e0 = 0
        for slot, k in enumerate(order):
            ei_k, deg_k = alone[k]
            lo, hi = int(ptr[slot]), int(ptr[slot + 1])
            assert torch.equal(deg[lo:hi], deg_k), (order, k)
            assert torch.equal(ei[:, e0:e0 + ei_k.shape[1]] - lo, ei_k), (order, k)
            e0 += ei_k.shape[1]
        assert e0 == ei.shape[1]
    # one cutoff and cap per set: each set as if it were called alone with its own
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    ei, deg = m.neighbor_graph(place(torch.from_numpy(np.concatenate(sets))), (5.0, 15.0, 8.0), (8, 24, None), ptr=ptr)
    e0 = 0
    for k, (c, q) in enumerate(((5.0, 8), (15.0, 24), (8.0, None))):
        ei_k, deg_k = m.neighbor_graph(place(torch.from_numpy(sets[k])), c, q)
        assert torch.equal(deg[int(ptr[k]):int(ptr[k + 1])], deg_k)
        assert torch.equal(ei[:, e0:e0 + ei_k.shape[1]] - int(ptr[k]), ei_k)
        e0 += ei_k.shape[1]
    assert e0 == ei.shape[1]


# ------------------------------------------------------------------ E. ABI and errors
def abi_case(make, place):
    """The C entry point itself: outputs on preallocated buffers, read only after an explicit synchronisation of the stream the
    call was enqueued on (a capped call returns without one: E <= N * cap sizes the buffer in advance); the error rules."""
    m = model_for(make)
    x = _normals(129, seed=31)
    n, cap = len(x), 8
    pos = place(torch.from_numpy(x))
    dev = pos.device
    capacity = n * cap
    deg = torch.full((n,), -1, dtype=torch.int32, device=dev)
    offsets = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    edge = torch.full((2, capacity), -7, dtype=torch.int64, device=dev)
    n_edges = torch.full((1,), -1, dtype=torch.int32, device=dev)
    ptr = np.asarray([0, n], dtype=np.int32)

    def cfg(**kw):
        c = L.NeighborGraphCfg()
        c.struct_size = ctypes.sizeof(L.NeighborGraphCfg)
        c.n_nodes, c.n_sets, c.max_neighbors, c.cutoff, c.capacity = n, 1, cap, 5.0, capacity
        c.pos, c.ptr = pos.data_ptr(), ptr.ctypes.data
        c.deg, c.offsets, c.edge_index, c.n_edges = deg.data_ptr(), offsets.data_ptr(), edge.data_ptr(), n_edges.data_ptr()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def call(c):
        return m.lib.ddmi_neighbor_graph(m._h, ctypes.byref(c), m._stream())
    assert call(cfg()) == 0
    if dev.type == "cuda":
        torch.cuda.current_stream(dev).synchronize()
    E = int(n_edges.item())
    want = dio.neighbor_graph(x, 5.0, cap)
    assert E == want.shape[1] and int(deg.sum()) == E and int(offsets[-1]) == E and int(offsets[0]) == 0
    assert torch.equal(offsets[1:].long(), torch.cumsum(deg.long(), 0))
    assert np.array_equal(edge[:, :E].cpu().numpy(), want)
    assert bool((edge[:, E:] == -7).all()), "columns past n_edges were written"
    # counting only; then a capacity below the total of an UNCAPPED call drops the columns past it and still reports the total
    n_edges.fill_(-1)
    assert call(cfg(edge_index=None, capacity=0, max_neighbors=0)) == 0
    if dev.type == "cuda":
        torch.cuda.current_stream(dev).synchronize()
    total = int(n_edges.item())
    uncapped = dio.neighbor_graph(x, 5.0, None)
    assert total == uncapped.shape[1] and total > 10
    small = torch.full((2, 10), -7, dtype=torch.int64, device=dev)
    n_edges.fill_(-1)
    assert call(cfg(edge_index=small.data_ptr(), capacity=10, max_neighbors=0)) == 0
    if dev.type == "cuda":
        torch.cuda.current_stream(dev).synchronize()
    assert int(n_edges.item()) == total and np.array_equal(small.cpu().numpy(), uncapped[:, :10])
    # errors: nothing is enqueued
    bad_ptr = np.asarray([0, 70, 60, n], dtype=np.int32)
    nan = float("nan")
    for c in (cfg(struct_size=ctypes.sizeof(L.NeighborGraphCfg) - 8), cfg(pos=None), cfg(ptr=None), cfg(n_nodes=0), cfg(n_sets=0),
              cfg(n_sets=3, ptr=bad_ptr.ctypes.data), cfg(ptr=np.asarray([0, n - 1], dtype=np.int32).ctypes.data),
              cfg(cutoff=0.0), cfg(cutoff=-1.0), cfg(cutoff=nan), cfg(max_neighbors=-1), cfg(capacity=capacity - 1), cfg(capacity=-1)):
        assert call(c) == -1, m.lib.ddmi_last_error()
        assert b"ddmi_neighbor_graph" in m.lib.ddmi_last_error() or b"null" in m.lib.ddmi_last_error()
    with pytest.raises(L.DdmiError, match="ddmi error -1"):
        m.neighbor_graph(pos, 0.0, cap)
    with pytest.raises(ValueError):
        m.neighbor_graph(pos, (5.0, 6.0), cap)
    assert call(cfg()) == 0      # the handle is unharmed


# ------------------------------------------------------------------ F. end to end
def end_to_end_case(make, place, tmp_path):
    """complex_graph(all_atoms=True, model=m) on the 1a0q files against the host path of the same call: every tensor equal; the two
    neighbour graphs as in B (rows as sets; a differing row is one where the float64 oracle differs from the host path as well --
    the residue graph's host path is the reference's torch.cdist arithmetic -- or one under the margin)."""
    for name in ("1a0q_protein_processed.pdb", "1a0q_ligand.sdf"):
        with gzip.open(os.path.join(GOLDEN, "1a0q", name + ".gz"), "rb") as src, open(tmp_path / name, "wb") as dst:
            shutil.copyfileobj(src, dst)
    files = (str(tmp_path / "1a0q_protein_processed.pdb"), str(tmp_path / "1a0q_ligand.sdf"))
    host = dio.complex_graph(*files, lm_dim=0, all_atoms=True)
    dev = dio.complex_graph(*files, lm_dim=0, all_atoms=True, model=model_for(make))
    for nt, attrs in (("receptor", ("x", "pos")), ("atom", ("x", "pos")), ("ligand", ("x", "pos", "edge_mask"))):
        for a in attrs:
            assert torch.equal(getattr(host[nt], a), getattr(dev[nt], a)), (nt, a)
    assert torch.equal(host["atom", "receptor"].edge_index, dev["atom", "receptor"].edge_index)
    assert torch.equal(host["ligand", "ligand"].edge_index, dev["ligand", "ligand"].edge_index)
    assert torch.equal(host.original_center, dev.original_center)
    for rel, inp in ((("receptor", "receptor"), "calpha_15_24"), (("atom", "atom"), "atoms_5_8")):
        want, excusable = oracle(inp)
        n = len(want)
        h = [set(r) for r in rows_of(host[rel].edge_index, n)]
        d = [set(r) for r in rows_of(dev[rel].edge_index, n)]
        diff = [i for i in range(n) if d[i] != h[i]]
        print(f"end to end {rel}: device and host path differ in {len(diff)} rows")
        assert all(set(want[i]) != h[i] or excusable[i] for i in diff), (rel, diff[:8])
