"""Judging sampled poses: what every caller of `sampling()` runs next (evaluate.py:474-505, utils/training.py:282-287,
confidence/dataset.py:241) -- on the device, next to the poses.

    iso = isomorphisms(atomic_numbers, bonds)                   once per ligand, on the host (networkx)
    out = evaluate_poses(pos, ref, model=model, perm=iso, confidence=conf)

`pos` is the `[N, n, 3]` tensor `sample_poses` returns, or the `[steps + 1, N, n, 3]` trajectory; everything returned is a device
tensor.  The reference runs spyrmsd's Python loop over all graph isomorphisms per pose under a 10 s alarm and, on a timeout,
silently reports the UNCORRECTED RMSD (utils/molecules_utils.py:3-18, evaluate.py:479-481).  Here the loop over isomorphisms is a
device reduction (ddmi_pose_metrics), and an enumeration cut short is reported (`complete=False`), never replaced.

Out of scope: the dataset-level statistics of evaluate.py:554-640 (percentiles and success rates over complexes) and GNINA.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch


class Isomorphisms(NamedTuple):
    perm: np.ndarray   # int32 [S, m]: row s maps atom j of a pose onto atom perm[s, j] of the reference
    complete: bool     # False: the enumeration stopped at max_isomorphisms; an RMSD over these rows is an upper bound


def isomorphisms(atomic_numbers, bonds=None, adjacency=None, max_isomorphisms=None) -> Isomorphisms:
    """All graph isomorphisms of a molecule onto itself, nodes matched on atomic number: networkx graph matching as spyrmsd's
    networkx backend runs it (spyrmsd/graphs/nx.py:51-101).  `bonds` = [(a, b, ...)] as `io.read_sdf` returns them, or `adjacency`
    = an [m, m] matrix.  A pair (idx1, idx2) of spyrmsd (rmsd.py:184-187: sum |c1[idx1[i]] - c2[idx2[i]]|^2, c1 the reference)
    becomes the row perm[idx2[i]] = idx1[i].  When there are more than `max_isomorphisms`, the first that many are returned (the
    identity among them) with complete=False."""
    import networkx as nx
    z = np.asarray(atomic_numbers).reshape(-1)
    m = len(z)
    if (bonds is None) == (adjacency is None):
        raise ValueError("isomorphisms: give bonds or adjacency")
    if max_isomorphisms is not None and max_isomorphisms < 1:
        raise ValueError("isomorphisms: max_isomorphisms must be at least 1")
    G = nx.Graph()
    G.add_nodes_from(range(m))
    if adjacency is not None:
        A = np.asarray(adjacency)
        if A.shape != (m, m):
            raise ValueError(f"adjacency: [{m}, {m}] expected, got {A.shape}")
        G.add_edges_from((int(a), int(b)) for a, b in zip(*np.nonzero(A)))
    else:
        G.add_edges_from((int(b[0]), int(b[1])) for b in bonds)
    nx.set_node_attributes(G, {i: int(z[i]) for i in range(m)}, "aprops")
    GM = nx.algorithms.isomorphism.GraphMatcher(G, G, lambda a, b: a["aprops"] == b["aprops"])
    identity = np.arange(m, dtype=np.int32)
    rows, complete, has_identity = [], True, False
    for iso in GM.isomorphisms_iter():
        if max_isomorphisms is not None and len(rows) >= max_isomorphisms:
            complete = False
            break
        row = np.empty(m, dtype=np.int32)
        row[list(iso.values())] = list(iso.keys())
        has_identity = has_identity or np.array_equal(row, identity)
        rows.append(row)
    if not has_identity:   # an enumeration cut short may not have reached it
        rows[-1] = identity
    return Isomorphisms(np.stack(rows), complete)


def confidence_order(confidence):
    """evaluate.py:488-493: column 0 of a multi-output confidence, NaN -> -1e-6, np.argsort(..)[::-1] (an ascending sort, reversed)."""
    c = torch.as_tensor(confidence)
    if c.dim() > 1:
        c = c[:, 0]
    c = torch.nan_to_num(c.float(), nan=-1e-6, posinf=float("inf"), neginf=float("-inf"))
    return torch.argsort(c, stable=True).flip(0)


def evaluate_poses(pos, ref, *, model, perm=None, atom_index=None, points=None, confidence=None, per_ref=False, minimize=False):
    """`model.pose_metrics` (any MIScoreModel: it lends its device and stream) plus what follows from the values, all on the device:
    rmsd_below_2 / rmsd_below_5 flags per pose, `complete` (False when `perm` is an Isomorphisms cut short: the RMSDs are then upper
    bounds), and with `confidence` [N] or [N, outputs]: `order` (evaluate.py:488-493), `top1_rmsd` = the RMSD of the most confident
    pose, `top5_rmsd` = the smallest among the five most confident (evaluate.py:627).  For a trajectory [T, N, n, 3] the ordering of
    the N poses applies to every step: top1_rmsd / top5_rmsd are [T].
    `minimize=True` adds the outputs of `model.pose_fit` (ddmi_pose_fit: rmsd_min = spyrmsd's symmrmsd with minimize=True, best_min,
    rotation, translation, and rmsd_min_per_ref with per_ref) and, with `confidence`, top1_rmsd_min / top5_rmsd_min built as
    top1_rmsd / top5_rmsd are.  Without it nothing of that is computed."""
    complete = True
    if isinstance(perm, Isomorphisms):
        perm, complete = perm.perm, perm.complete
    out = model.pose_metrics(pos, ref, perm=perm, atom_index=atom_index, points=points, per_ref=per_ref)
    out["complete"] = complete
    out["rmsd_below_2"], out["rmsd_below_5"] = out["rmsd"] < 2.0, out["rmsd"] < 5.0
    if minimize:
        out.update(model.pose_fit(pos, ref, perm=perm, atom_index=atom_index, per_ref=per_ref))
    if confidence is not None:
        order = confidence_order(torch.as_tensor(confidence).to(out["rmsd"].device))
        if order.shape[0] != out["rmsd"].shape[-1]:
            raise ValueError(f"confidence: one row per pose expected ({out['rmsd'].shape[-1]}), got {order.shape[0]}")
        ranked = out["rmsd"].index_select(-1, order)
        out["order"] = order
        out["top1_rmsd"] = ranked[..., 0]
        out["top5_rmsd"] = ranked[..., :5].min(dim=-1).values
        if minimize:
            ranked = out["rmsd_min"].index_select(-1, order)
            out["top1_rmsd_min"] = ranked[..., 0]
            out["top5_rmsd_min"] = ranked[..., :5].min(dim=-1).values
    return out


def superpose(pos, fit):
    """The poses moved onto their best known pose: `pos @ rotation^T + translation` with the transform `pose_fit` (or
    `evaluate_poses(minimize=True)`) returned, on the device of `fit`, e.g. for writing aligned poses out.  The transform was fitted
    on the kept atoms and is applied to all of `pos` [.., n, 3]."""
    R, t = fit["rotation"], fit["translation"]
    pos = torch.as_tensor(pos).to(R.device, R.dtype)
    return pos @ R.transpose(-1, -2) + t.unsqueeze(-2)
