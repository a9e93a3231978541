"""tests/golden/pose_metrics_min.pt: the fixture of the minimised-RMSD tests (tests/metrics_min_cases.py).  Data only.

    python tests/golden/make_golden_metrics_min.py    (on a machine that has the reference; the tests need only the fixture)

What is REFERENCE-EXECUTED: the reference's vendored spyrmsd, unmodified -- `spyrmsd.rmsd.symmrmsd(..., minimize=True)` (for every
graph isomorphism the QCP RMSD of spyrmsd/qcp.py after centring, then the min) and `spyrmsd.rmsd.rmsd(..., minimize=True)`, in
float64 on float32-stored inputs.  Three parts:

  1a0q, sym576   the molecules of tests/golden/pose_metrics.pt with the same ref / pos / perm (loaded from that fixture, not stored
                 again): rmsd_min_per_ref [2, 40] and rmsd_min [40] (its min over the known poses) of the 40 noisy poses, and `rigid`:
                 12 poses = ref[0] under a random isomorphism, a random rotation about its centroid and a N(0, 3 A) shift, plus
                 noise of sigma = 0, 1e-3, 0.3 A (four poses each) with their rmsd_min_per_ref [2, 12] and rmsd_min [12].  The
                 reference returns exactly 0.0 for sigma = 0 (against the known pose the copy was made from): its atol rule.
  small          asymmetric sets (identity permutation, spyrmsd.rmsd.rmsd): m = 1, 2, 3, a planar 6-ring, a collinear 4-atom chain
                 and a chiral 5-atom centre against its MIRROR image, where a Kabsch that allowed a reflection would return 0.

Conditions asserted here: no stored triple lies near the atol edge (|e| < 1e-10 or |e| > 1e-8 for e = Ga + Gb - 2 lambda); the float64
numpy restatement of the kernel's formula (`restated_e`: numpy.linalg.eigvalsh of the key matrix; tests/metrics_min_cases.py holds the
same function) agrees with every executed value -- exactly 0 where the atol rule gives 0, within 1e-12 relative elsewhere, except
where the reference's own Newton iteration is the less accurate of the two (NEWTON_LIMITED below: the sigma = 1e-3 copies, m = 2 and
the collinear chain)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from spyrmsd import rmsd as srmsd  # noqa: E402

ATOL = 1e-9
# Where the reference's own Newton iteration on the characteristic polynomial (qcp.py:164-203) limits ITS accuracy, 1e-12 relative
# cannot hold between it and an eigen-solver, and the bound is what the tests need instead: they compare the device with the executed
# values at 1e-5 relative, so the executed value itself must be good to a tenth of that.  Two such classes, both measured here:
#   near-perfect fits (sigma = 1e-3: e = m rmsd^2 ~ 5e-5 A^2): the polynomial has coefficients of size (Ga + Gb)^4 / 16 and leaves an
#     absolute error of about 1e-12 A^2 in e, 1e-9 .. 1.5e-8 relative in the RMSD;
#   a degenerate largest eigenvalue (m = 2, collinear atoms): a double root, where Newton converges linearly and stops at scipy's
#     step tolerance of 1.48e-8: 2e-8 .. 1e-7 relative.
NEWTON_LIMITED = 1e-6


def key_matrices(M):
    """[..., 3, 3] -> [..., 4, 4]: the symmetric key matrix of spyrmsd/qcp.py:55-122."""
    xx, xy, xz, yx, yy, yz, zx, zy, zz = (M[..., i, j] for i in range(3) for j in range(3))
    rows = [[xx + yy + zz, yz - zy, zx - xz, xy - yx], [yz - zy, xx - yy - zz, xy + yx, zx + xz],
            [zx - xz, xy + yx, -xx + yy - zz, yz + zy], [xy - yx, zx + xz, yz + zy, -xx - yy + zz]]
    return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)


def restated_e(pos, ref, perm=None, atom_index=None):
    """e = Ga + Gb - 2 lambda_max in float64 -> [P, K, S], for a_j = pos[p, atom_index[j]] and b_j = ref[k, perm[s, j]]."""
    pos, ref = np.asarray(pos, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    x = pos if atom_index is None else pos[:, np.asarray(atom_index)]
    perm = np.arange(ref.shape[1])[None] if perm is None else np.asarray(perm)
    A = x - x.mean(axis=1, keepdims=True)
    B = ref - ref.mean(axis=1, keepdims=True)
    Ga, Gb = (A ** 2).sum(axis=(1, 2)), (B ** 2).sum(axis=(1, 2))
    out = np.empty((x.shape[0], ref.shape[0], perm.shape[0]))
    for k in range(ref.shape[0]):
        M = np.einsum("pji,sjl->psil", A, B[k][perm])
        out[:, k] = Ga[:, None] + Gb[k] - 2.0 * np.linalg.eigvalsh(key_matrices(M))[..., -1]
    return out


def rmsd_of_e(e, m):
    return np.where(np.abs(e) < ATOL, 0.0, np.sqrt(np.maximum(e, 0.0) / m))


def off_the_edge(tag, e):
    """No triple of the restatement e [P, K, S] near the reference's atol."""
    m_edge = (np.abs(e) >= 1e-10) & (np.abs(e) <= 1e-8)
    assert not m_edge.any(), (tag, "a triple near the atol edge", e[m_edge])
    return e


def compare(tag, mine, executed, bound=1e-12):
    zero = executed == 0.0
    assert np.array_equal(mine == 0.0, zero), (tag, mine[zero], executed[mine == 0.0])
    dev = float(np.max(np.abs(mine[~zero] / executed[~zero] - 1.0))) if (~zero).any() else 0.0
    print(f"{tag}: {int(zero.sum())} exact zeros, restatement within {dev:.2e} relative of the executed values elsewhere")
    assert dev < bound, (tag, dev, bound)


def random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def executed_per_ref(ref, pos, z, A):
    ref64, pos64 = ref.astype(np.float64), pos.astype(np.float64)
    return np.array([srmsd.symmrmsd(ref64[k], [p for p in pos64], z, z, A, A, minimize=True) for k in range(ref.shape[0])])   # [K, P]


def molecule(name, mol, rng):
    ref, pos, perm = mol["ref"].numpy(), mol["pos"].numpy(), mol["perm"].numpy()
    z, A = mol["z"].numpy(), mol["adjacency"].numpy().astype(np.int64)
    m = ref.shape[1]
    out = {}
    # the 40 noisy poses of pose_metrics.pt
    per_ref = executed_per_ref(ref, pos, z, A)
    e = restated_e(pos, ref, perm)
    off_the_edge(name, e)
    compare(name, rmsd_of_e(e, m).min(-1).T, per_ref)
    out["rmsd_min_per_ref"], out["rmsd_min"] = torch.from_numpy(per_ref), torch.from_numpy(per_ref.min(0))
    print(f"{name}: rmsd_min {per_ref.min(0).min():.3f} .. {per_ref.min(0).max():.3f} A, unminimised "
          f"{mol['rmsd'].numpy().min():.3f} .. {mol['rmsd'].numpy().max():.3f} A")
    assert (per_ref.min(0) < mol["rmsd"].numpy() - 1e-3).all()
    # rigid copies of ref[0]
    sigma = np.repeat([0.0, 1e-3, 0.3], 4)
    r0 = ref[0].astype(np.float64)
    rigid = np.empty((len(sigma), m, 3), dtype=np.float32)
    for i, sg in enumerate(sigma):
        row = perm[rng.integers(0, len(perm))]
        c = r0.mean(0)
        x = (r0[row] - c) @ random_rotation(rng).T + c + rng.normal(0.0, 3.0, size=3)
        rigid[i] = (x + (rng.normal(0.0, sg, size=(m, 3)) if sg else 0.0)).astype(np.float32)
    per_ref = executed_per_ref(ref, rigid, z, A)
    e = restated_e(rigid, ref, perm)
    off_the_edge(name + " rigid", e)
    mine = rmsd_of_e(e, m).min(-1).T
    near = sigma == 1e-3
    compare(name + " rigid, sigma 0 and 0.3", mine[:, ~near], per_ref[:, ~near])
    compare(name + " rigid, sigma 1e-3", mine[:, near], per_ref[:, near], NEWTON_LIMITED)
    best = per_ref.min(0)
    assert (best[:4] == 0.0).all() and (best[4:] > 0).all(), best
    print(f"{name} rigid: sigma 0: e at the copy's own triple up to {np.abs(e[:4, 0]).min(-1).max():.1e}; sigma 1e-3: {best[4:8].min():.2e} .. "
          f"{best[4:8].max():.2e} A; sigma 0.3: {best[8:].min():.3f} .. {best[8:].max():.3f} A")
    out["rigid"] = dict(pos=torch.from_numpy(rigid), sigma=torch.from_numpy(sigma), rmsd_min_per_ref=torch.from_numpy(per_ref),
                        rmsd_min=torch.from_numpy(best))
    return out


def small_sets(rng):
    off = np.array([20.0, -15.0, 30.0])
    cloud = lambda m: rng.normal(0.0, 1.5, size=(m, 3))
    sets = {}
    sets["m1"] = (cloud(1) + off, cloud(1) + off)
    sets["m2"] = (np.array([[0.0, 0.0, 0.0], [1.1, 0.3, -0.2]]) + off, np.array([[0.5, 0.5, 0.5], [0.1, -1.6, 1.4]]) + off)   # bond lengths 1.16 / 2.33
    sets["m3"] = (cloud(3) + off, cloud(3) + off)
    ang = np.arange(6) * np.pi / 3
    ring = np.stack([1.39 * np.cos(ang), 1.39 * np.sin(ang), np.zeros(6)], axis=1)
    sets["ring6"] = ((ring + rng.normal(0.0, 0.2, size=(6, 3)) * np.array([1.0, 1.0, 0.0])) @ random_rotation(rng).T + off, ring + off)   # both planar
    d = np.array([0.6, -0.3, 0.74])
    chain_a = np.outer([0.0, 1.5, 3.1, 4.4], d / np.linalg.norm(d))
    chain_b = np.outer([0.0, 1.0, 2.5, 5.4], [0.0, 0.0, 1.0])
    sets["chain4"] = (chain_a + off, chain_b - off)
    tet = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64) / np.sqrt(3)
    chiral = np.concatenate([np.zeros((1, 3)), tet * np.array([[1.1], [1.5], [1.8], [2.2]])])
    sets["mirror5"] = (chiral @ random_rotation(rng).T + off, chiral * np.array([-1.0, 1.0, 1.0]) + off)
    out = {}
    for name, (a, b) in sets.items():
        a, b = a.astype(np.float32), b.astype(np.float32)
        m = len(a)
        z = np.arange(1, m + 1)
        val = float(srmsd.rmsd(b.astype(np.float64), a.astype(np.float64), z, z, minimize=True))   # reference-executed
        e = restated_e(a[None], b[None])
        off_the_edge(name, e)
        compare("small " + name, rmsd_of_e(e, m).reshape(1), np.array([val]), NEWTON_LIMITED if name in ("m2", "chain4") else 1e-12)
        print(f"small {name}: m = {m}, rmsd_min {val:.6f} A, e = {e.item():.3e}")
        out[name] = dict(pos=torch.from_numpy(a), ref=torch.from_numpy(b), rmsd_min=val)
    assert out["m1"]["rmsd_min"] == 0.0 and out["mirror5"]["rmsd_min"] > 0.1
    return out


def main():
    rng = np.random.default_rng(1)
    base = torch.load(os.path.join(HERE, "pose_metrics.pt"), weights_only=False)
    out = {"provenance": "rmsd_min*: spyrmsd.rmsd.symmrmsd(minimize=True) / spyrmsd.rmsd.rmsd(minimize=True) executed (the reference's "
                         "vendored spyrmsd) in float64 on these float32 inputs; ref / pos / perm of the molecules: pose_metrics.pt"}
    for name in ("1a0q", "sym576"):
        out[name] = molecule(name, base[name], rng)
    out["small"] = small_sets(rng)
    path = os.path.join(HERE, "pose_metrics_min.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
