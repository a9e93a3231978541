"""tests/golden/pose_metrics.pt: the fixture of the pose-metric tests (tests/metrics_cases.py).  Data only.

    python tests/golden/make_golden_metrics.py        (on a machine that has the reference; the tests need only the fixture)

What is REFERENCE-EXECUTED: the reference's vendored spyrmsd, unmodified -- `spyrmsd.graph.graph_from_adjacency_matrix` and
`spyrmsd.graph.match_graphs` (networkx backend) enumerate the graph isomorphisms, `spyrmsd.rmsd.symmrmsd` (center = minimize =
False, as utils/molecules_utils.py:9-17 calls it) gives the symmetry-corrected RMSD of every pose to every reference in float64.
RDKit is not needed: adjacency matrices and atomic numbers are passed directly, as get_symmetry_rmsd does after its conversion.

Two molecules, each with K = 2 references near (20, -15, 30) A and P = 40 poses = reference 0 under a random isomorphism plus
N(0, 1 A) noise (numpy default_rng(0)), stored in float32 (the symmrmsd inputs are those float32 values):
  1a0q     the ligand of tests/golden/1a0q (io.read_sdf): 23 heavy atoms
  sym576   21 atoms: a centre (Z = 14) carrying two six-rings of carbon, each bound through one ring atom, and two CF3 groups;
           2 (ring flip)^2 * 2 (ring swap) * 6^2 (fluorines) * 2 (CF3 swap) = 576 isomorphisms

Per molecule: z [m], adjacency [m, m], ref [2, m, 3], pos [40, m, 3], perm [S, m] int32 (the enumerated pairs (idx1, idx2) as rows
perm[idx2[i]] = idx1[i]), applied [40] (the row each pose was built from), rmsd_per_ref [2, 40] and rmsd [40] float64 (symmrmsd, and
its min over references as evaluate.py:484).  Conditions asserted here: the isomorphism counts; a float64 restatement of the
kernel's formula over `perm` equals symmrmsd exactly; the plain RMSD differs from the symmetric one for every pose of sym576."""
import gzip
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from diffdock_amd import io as dio  # noqa: E402
from spyrmsd import graph as sgraph  # noqa: E402
from spyrmsd import rmsd as srmsd  # noqa: E402

OFFSET = np.array([20.0, -15.0, 30.0])
P = 40


def rotation(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def frame(d):
    """Two unit vectors orthogonal to d and to each other."""
    d = d / np.linalg.norm(d)
    a = np.cross(d, [0.3, -0.5, 0.8])
    a /= np.linalg.norm(a)
    return d, a, np.cross(d, a)


def sym576():
    """Coordinates [21, 3], atomic numbers, bonds of the synthetic molecule (rough tetrahedral geometry; only the graph matters)."""
    dirs = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64) / np.sqrt(3)
    xyz, z, bonds = [np.zeros(3)], [14], []
    for d in dirs[:2]:       # six-rings bound through one ring atom
        d, a, _ = frame(d)
        first = len(xyz)
        centre = d * (1.87 + 1.39)
        for i in range(6):
            ang = np.pi + i * np.pi / 3      # atom 0 of the ring points at the centre atom
            xyz.append(centre + 1.39 * (np.cos(ang) * d + np.sin(ang) * a))
            z.append(6)
            bonds.append((first + i, first + (i + 1) % 6))
        bonds.append((0, first))
    for d in dirs[2:]:       # CF3
        d, a, b = frame(d)
        c = len(xyz)
        xyz.append(d * 1.9)
        z.append(6)
        bonds.append((0, c))
        for i in range(3):
            ang = i * 2 * np.pi / 3
            xyz.append(d * 1.9 + 0.45 * d + 1.27 * (np.cos(ang) * a + np.sin(ang) * b))
            z.append(9)
            bonds.append((c, c + 1 + i))
    return np.array(xyz), np.array(z, dtype=np.int64), bonds


def ligand_1a0q():
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "1a0q_ligand.sdf")
        with gzip.open(os.path.join(HERE, "1a0q", "1a0q_ligand.sdf.gz"), "rb") as src, open(path, "wb") as dst:
            shutil.copyfileobj(src, dst)
        xyz, z, bonds = dio.read_sdf(path)
    return xyz, z, [(a, b) for a, b, _ in bonds]


def restated(ref, pos, perm):
    """The kernel's formula in float64: sqrt(min_s sum_j |ref[perm[s, j]] - pos[j]|^2 / m) -> [K, P]."""
    d = ref[:, None, perm] - pos[None, :, None]                    # [K, P, S, m, 3]
    return np.sqrt((d ** 2).sum(-1).sum(-1).min(-1) / ref.shape[1])


def molecule(name, xyz, z, bonds, n_iso, rng):
    m = len(z)
    A = np.zeros((m, m), dtype=np.int64)
    for a, b in bonds:
        A[a, b] = A[b, a] = 1
    G = sgraph.graph_from_adjacency_matrix(A, z)
    pairs = sgraph.match_graphs(G, G)                               # reference-executed enumeration
    assert len(pairs) == n_iso, (name, len(pairs))
    perm = np.empty((len(pairs), m), dtype=np.int32)
    for s, (idx1, idx2) in enumerate(pairs):
        perm[s, idx2] = idx1
    base = xyz - xyz.mean(0)
    ref0 = base + OFFSET
    ref1 = base @ rotation([0.2, 1.0, -0.4], 0.35).T + OFFSET + np.array([0.8, -0.5, 0.6])
    ref = np.stack([ref0, ref1]).astype(np.float32)
    applied = rng.integers(0, len(pairs), size=P)
    pos = (ref[0].astype(np.float64)[perm[applied]] + rng.normal(0.0, 1.0, size=(P, m, 3))).astype(np.float32)
    ref64, pos64 = ref.astype(np.float64), pos.astype(np.float64)
    per_ref = np.array([srmsd.symmrmsd(ref64[k], [p for p in pos64], z, z, A, A) for k in range(2)])   # reference-executed values
    mine = restated(ref64, pos64, perm)
    assert np.array_equal(mine, per_ref), (name, np.abs(mine - per_ref).max())
    plain = np.sqrt(((pos64[None] - ref64[:, None]) ** 2).sum(-1).mean(-1)).min(0)
    sym = per_ref.min(0)
    f32 = restated(ref, pos, perm)
    sums = ((ref64[:, None, perm] - pos64[None, :, None]) ** 2).sum(-1).sum(-1)          # [K, P, S]
    two = np.sort(sums.transpose(1, 0, 2).reshape(P, -1), axis=1)[:, :2]
    print(f"{name}: m = {m}, S = {len(pairs)}, rmsd {sym.min():.3f} .. {sym.max():.3f} A, plain != symmetric for "
          f"{int((plain != sym).sum())} of {P} poses, float32 restatement within {np.abs(f32 / per_ref - 1).max():.2e} relative, "
          f"smallest relative gap best / second-best triple {((two[:, 1] - two[:, 0]) / two[:, 0]).min():.2e}")
    return dict(z=torch.from_numpy(z), adjacency=torch.from_numpy(A.astype(np.uint8)), ref=torch.from_numpy(ref),
                pos=torch.from_numpy(pos), perm=torch.from_numpy(perm), applied=torch.from_numpy(applied),
                rmsd_per_ref=torch.from_numpy(per_ref), rmsd=torch.from_numpy(sym),
                plain_differs=int((plain != sym).sum())), bonds


def main():
    rng = np.random.default_rng(0)
    out = {"provenance": "isomorphisms: spyrmsd.graph.match_graphs executed; rmsd_per_ref: spyrmsd.rmsd.symmrmsd executed "
                         "(the reference's vendored spyrmsd, networkx backend)"}
    for name, (xyz, z, bonds), n_iso in (("1a0q", ligand_1a0q(), 8), ("sym576", sym576(), 576)):
        out[name], b = molecule(name, xyz, z, bonds, n_iso, rng)
        out[name]["bonds"] = torch.tensor(b, dtype=torch.int64)
    assert out["sym576"]["plain_differs"] == P
    torch.save(out, os.path.join(HERE, "pose_metrics.pt"))
    print("wrote", os.path.join(HERE, "pose_metrics.pt"), os.path.getsize(os.path.join(HERE, "pose_metrics.pt")), "bytes")


if __name__ == "__main__":
    main()
