"""Conformer matching (datasets/conformer_matching.py, called from get_lig_graph_with_matching, datasets/process_mols.py:323-384):
search the torsion angles of a generated conformer for the conformer closest to the known pose.

`match_conformers` runs every (ligand, try) as one job of ONE device call (MIScoreModel.match_conformer, ddmi_match_conformer).
`match_conformers_host` is the host route: scipy.optimize.differential_evolution called exactly as optimize_rotatable_bonds calls
it, on a float64 numpy restatement of the objective -- the comparison arm of the tests and of tools/matching_bench.py, and the
fallback without a device.  The objective E(theta) is the minimised RMSD between torsions(start, theta) and the target; the angles are
relative to the start conformer (the reference sets absolute dihedrals: the same conformers are reachable, include/ddmi.h)."""
import numpy as np
import torch


def torsion_table(graph):
    """rot_u, rot_v (int32 [R]: the rotatable bonds in edge order) and mask (bool [R, n]) of a ligand graph, from its bond
    edge_index, edge_mask and mask_rotate."""
    ei = graph["ligand", "ligand"].edge_index
    em = torch.as_tensor(graph["ligand"].edge_mask).bool()
    mr = graph["ligand"].mask_rotate
    mr = mr[0] if isinstance(mr, (list, tuple)) else mr
    mask = np.asarray(mr.cpu() if torch.is_tensor(mr) else mr, dtype=bool)
    rot = ei.cpu().numpy().T[em.cpu().numpy()]
    n = graph["ligand"].pos.shape[-2] if torch.is_tensor(graph["ligand"].pos) else len(graph["ligand"].x)
    mask = mask.reshape(len(rot), n)
    return rot[:, 0].astype(np.int32), rot[:, 1].astype(np.int32), mask


def _table(t):
    if isinstance(t, (tuple, list)) and len(t) == 3:
        u, v, mask = t
        return np.asarray(u, dtype=np.int32).reshape(-1), np.asarray(v, dtype=np.int32).reshape(-1), np.asarray(mask, dtype=bool)
    return torsion_table(t)


def _rotvec_matrix(v):
    th = np.linalg.norm(v)
    if th < 1e-12:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def torsions(start, rot_u, rot_v, mask, theta):
    """utils/torsion.py:48-72 in float64: the bonds in order, an angle of exactly 0 skipped, no re-alignment."""
    pos = np.array(start, dtype=np.float64)
    for j in range(len(rot_u)):
        if theta[j] == 0:
            continue
        u, v = rot_u[j], rot_v[j]
        vec = pos[u] - pos[v]
        R = _rotvec_matrix(vec * theta[j] / np.linalg.norm(vec))
        pos[mask[j]] = (pos[mask[j]] - pos[v]) @ R.T + pos[v]
    return pos


def _key_matrix(M):
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = M
    return np.array([[xx + yy + zz, yz - zy, zx - xz, xy - yx], [yz - zy, xx - yy - zz, xy + yx, zx + xz],
                     [zx - xz, xy + yx, -xx + yy - zz, yz + zy], [xy - yx, zx + xz, yz + zy, -xx - yy + zz]])


def fit(a, b):
    """(rmsd, R, t) of the proper rigid superposition of a [n, 3] onto b in float64: e = Ga + Gb - 2 lambda_max of Horn's key matrix
    (|e| < 1e-9 -> 0, the atol of ddmi_pose_fit), R a + t ~ b."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ca, cb = a.mean(0), b.mean(0)
    A, B = a - ca, b - cb
    w, V = np.linalg.eigh(_key_matrix(A.T @ B))
    e = (A ** 2).sum() + (B ** 2).sum() - 2.0 * w[-1]
    q0, x, y, z = V[:, -1]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * q0), 2 * (x * z + y * q0)],
                  [2 * (x * y + z * q0), 1 - 2 * (x * x + z * z), 2 * (y * z - x * q0)],
                  [2 * (x * z - y * q0), 2 * (y * z + x * q0), 1 - 2 * (x * x + y * y)]])
    return (0.0 if abs(e) < 1e-9 else float(np.sqrt(max(e, 0.0) / len(a)))), R, cb - R @ ca


def objective(start, target, rot_u, rot_v, mask, theta):
    """E(theta) in float64."""
    return fit(torsions(start, rot_u, rot_v, mask, theta), target)[0]


def _jobs(jobs, tries):
    out = []
    for table, starts, target in jobs:
        u, v, mask = _table(table)
        starts = np.asarray(starts.cpu() if torch.is_tensor(starts) else starts, dtype=np.float32)
        starts = starts[None] if starts.ndim == 2 else starts
        target = np.asarray(target.cpu() if torch.is_tensor(target) else target, dtype=np.float32)
        if starts.shape[1:] != target.shape or target.ndim != 2 or target.shape[1] != 3 or mask.shape != (len(u), len(target)):
            raise ValueError(f"match_conformers: starts {starts.shape}, target {target.shape} and mask {mask.shape} do not agree")
        out.append((u, v, mask, starts if tries is None else starts[:tries], target))
    return out


def match_conformers_host(jobs, popsize=15, maxiter=500, seed=0, tries=None):
    """The host route.  `jobs`: a list of (graph or (rot_u, rot_v, mask), start conformers [T, n, 3], target [n, 3]).  Every try is one
    scipy.optimize.differential_evolution call with the arguments of optimize_rotatable_bonds (bounds [-pi, pi] per bond, mutation
    (0.5, 1), recombination 0.8, `polish` at its default); a ligand without rotatable bonds is only superposed, as in the reference.
    Returns per ligand a dict: pos [n, 3] (the matched conformer of the best try, in the frame of target), angles [R], rmsd,
    rmsds [T], best (the try) and evaluations (objective calls of all tries)."""
    from scipy.optimize import differential_evolution
    out = []
    for u, v, mask, starts, target in _jobs(jobs, tries):
        res, nfev = [], 0
        for st in starts:
            theta = np.zeros(len(u))
            if len(u):
                r = differential_evolution(lambda x: objective(st, target, u, v, mask, x), [(-np.pi, np.pi)] * len(u), maxiter=maxiter,
                                           popsize=popsize, mutation=(0.5, 1), recombination=0.8, disp=False, seed=seed)
                theta, nfev = r.x, nfev + r.nfev
            moved = torsions(st, u, v, mask, theta)
            rmsd, R, t = fit(moved, target)
            res.append((rmsd, theta, moved @ R.T + t))
        best = int(np.argmin([r[0] for r in res]))
        out.append(dict(pos=torch.from_numpy(res[best][2].astype(np.float32)), angles=torch.from_numpy(res[best][1].astype(np.float32)),
                        rmsd=float(res[best][0]), rmsds=torch.tensor([r[0] for r in res], dtype=torch.float32), best=best, evaluations=nfev))
    return out


def match_conformers(jobs, model, popsize=15, maxiter=500, tol=0.01, seed=0, tries=None):
    """The device route: every (ligand, try) of `jobs` (as for match_conformers_host) is one job of ONE MIScoreModel.match_conformer
    call; the job id of try t of ligand l is its running number.  Returns per ligand a dict of device tensors: the try with the
    lowest rmsd (argmin on the device, process_mols.py:364-368) as pos [n, 3], angles [R], rmsd and best, and rmsds [T] of all tries.
    Nothing is copied back."""
    js = _jobs(jobs, tries)
    lig, tor, u_all, v_all, m_all, s_all, t_all = [0], [0], [], [], [], [], []
    for u, v, mask, starts, target in js:
        for st in starts:
            lig.append(lig[-1] + len(target)); tor.append(tor[-1] + len(u))
            u_all.append(u); v_all.append(v); m_all.append(mask.reshape(-1).astype(np.uint8)); s_all.append(st); t_all.append(target)
    cat = lambda parts, dt: torch.from_numpy(np.concatenate(parts).astype(dt)) if parts else torch.zeros(0)
    res = model.match_conformer(cat(s_all, np.float32), cat(t_all, np.float32), lig, tor, rot_u=cat(u_all, np.int32) if tor[-1] else None,
                                rot_v=cat(v_all, np.int32) if tor[-1] else None, mask_rotate=cat(m_all, np.uint8) if tor[-1] else None,
                                popsize=popsize, maxiter=maxiter, tol=tol, seed=seed)
    out, j = [], 0
    for u, v, mask, starts, target in js:
        T, n, R = len(starts), len(target), len(u)
        rmsds = res["rmsd"][j:j + T]
        best = rmsds.argmin()
        out.append(dict(pos=res["pos"][lig[j]:lig[j + T]].reshape(T, n, 3)[best], angles=res["angles"][tor[j]:tor[j + T]].reshape(T, R)[best],
                        rmsd=rmsds[best], rmsds=rmsds, best=best))
        j += T
    return out
