"""`sampling()` with the reference's signature (utils/sampling.py:69-72), running the step loop on the device.

    data_list, confidence = sampling(data_list, model, inference_steps, tr_schedule, rot_schedule,
                                     tor_schedule, device, t_to_sigma, model_args, ...)

Differences, all documented: the Gaussian draws come from a counter-based generator keyed by
(seed, global sample index, step, component) instead of the global torch RNG (so that a run sharded over GPUs
reproduces the single-GPU trajectories), or are injected through `noise=`; the confidence model is called after each
batch exactly as in the reference (sampling.py:208-227: fresh ligand positions copied into the confidence graphs,
t = 0) when it is a confidence-mode model of the built classes.  Per-step `crop_beyond` (sampling.py:104-109) runs on the device as a residue
mask + contact-graph re-compaction instead of the reference's deepcopy / to_data_list / from_data_list round trip.

`visualization_list` (sampling.py:193-206) is fed call for call as the reference feeds it, from the per-step record the device
loop writes (MIScoreModel.sample_batch(record=...)); `return_full_trajectory=True` returns the per-step poses as a third value
(see sampling()); the reference's NaN warning (sampling.py:117-124) is emitted through `logging` after each batch's loop from the
recorded per-step counts.  `pivot` and `return_features` raise NotImplementedError: the reference asserts them away too (:81).
"""
from __future__ import annotations

import logging

import numpy as np
import torch

from .hetero import HeteroBatch, set_time


logger = logging.getLogger(__name__)


def _check_hooks(model, want_steps, pivot, return_features):
    if return_features or pivot:
        raise NotImplementedError("pivot / feature returns are outside the built path (the reference asserts them away as well, "
                                  "utils/sampling.py:81)")
    if want_steps and not (hasattr(model, "sample_batch") or hasattr(model, "perturb")):
        raise NotImplementedError("per-step poses (visualization_list / return_full_trajectory) need a model with sample_batch "
                                  "(the device loop) or with perturb / modify_conformer_batch (the step-wise loop)")


def _sample_batch(model, want_steps, *args, **kw):
    """model.sample_batch with the per-step record -> (pos, step_pos or None, nan_count or None).  A model whose sample_batch
    does not take `record` (the signature of before the record) still samples: no NaN warnings, and per-step poses raise."""
    import inspect
    params = inspect.signature(model.sample_batch).parameters
    if "record" not in params and not any(p.kind is p.VAR_KEYWORD for p in params.values()):
        if want_steps:
            raise NotImplementedError("per-step poses (visualization_list / return_full_trajectory) on the device loop need a "
                                      "model.sample_batch that takes `record` (MIScoreModel.sample_batch); native_loop=False "
                                      "runs the step-wise loop instead")
        return model.sample_batch(*args, **kw), None, None
    pos, rec = model.sample_batch(*args, record={"nan", "pos"} if want_steps else {"nan"}, **kw)
    return pos, rec.pos, rec.nan_count


def _warn_nans(nan_count, names, batch_numbers, sizes):
    """The reference's warning (utils/sampling.py:117-124) for every step and NaN-guard group of one device batch whose guard
    fired.  nan_count: [steps, G] counts (one device-to-host copy here, after the loop); names / batch_numbers / sizes: the
    complex name, 1-based sampling() batch number and number of poses of each group."""
    if nan_count is None:
        return
    nan_count = torch.as_tensor(nan_count).detach().cpu()
    for t_idx, g in torch.nonzero(nan_count).tolist():
        logger.warning(f"Complex {names[g]} Batch {batch_numbers[g]} Inference Iteration {t_idx}: "
                       f"{int(nan_count[t_idx, g])} / {sizes[g]} samples failed")


def _complex_name(graph):
    name = getattr(graph, "name", "?")
    return name[0] if isinstance(name, list) else name


def _visualise_steps(visualization_list, data_list, lo, step_pos, bounds, first_step=0):
    """utils/sampling.py:193-198 for one sampling() batch: step_pos [steps, atoms, 3] on the host = the poses after steps
    first_step, first_step + 1, ..., bounds[i] = the atom range of pose lo + i in it."""
    for row in range(step_pos.shape[0]):
        for i, (a0, a1) in enumerate(bounds):
            visualization_list[lo + i].add(step_pos[row, a0:a1] + data_list[lo + i].original_center.detach().cpu(),
                                           part=1, order=first_step + row + 2)


def _visualise_final(visualization_list, data_list):
    """utils/sampling.py:203-206: after every batch the WHOLE list receives its entry's current pose with order=2 -- the poses
    of batches not yet sampled are their initial ones (kept as the reference does it)."""
    for idx, visualization in enumerate(visualization_list):
        visualization.add(data_list[idx]["ligand"].pos.detach().cpu() + data_list[idx].original_center.detach().cpu(),
                          part=1, order=2)


def _batches(data_list, batch_size):
    for lo in range(0, len(data_list), batch_size):
        yield lo, data_list[lo:lo + batch_size]


def _collate(chunk):
    try:  # real PyG objects collate themselves
        from torch_geometric.data import Batch  # type: ignore
        return Batch.from_data_list(chunk)
    except Exception:
        return HeteroBatch.from_data_list(chunk)


def _edge_store(g, a, b):
    """Edge store of node types (a, b) whatever the relation name (('receptor', 'rec_contact', 'receptor') in the reference)."""
    for et in g.edge_types:
        if et[0] == a and et[-1] == b:
            return g[et]
    return g[a, b]


def crop_beyond(graph, cutoff, all_atoms=False):
    """utils/utils.py:388-413 on ONE complex graph, in place: residues (and, all_atoms, their atoms) farther than `cutoff`
    from every ligand atom are removed, contact graphs restricted to the kept nodes and relabelled.  Host tensors: the
    reference applies it to the confidence graphs once per batch (utils/sampling.py:213-217); the per-step crop of the score
    model runs on the device instead (ddmi_set_crop_cutoff)."""
    lig, rec = graph["ligand"].pos, graph["receptor"].pos
    keep = torch.any(torch.sum((lig.unsqueeze(0) - rec.unsqueeze(1)) ** 2, -1) < cutoff ** 2, dim=1)
    if not bool(keep.any()):
        raise ValueError(f"crop_beyond({cutoff}) removes every residue of '{getattr(graph, 'name', '?')}': the ligand is farther than "
                         f"the cutoff from the whole receptor (an empty receptor graph cannot be scored)")

    def sub_graph(mask, edge_index):
        ok = mask[edge_index[0]] & mask[edge_index[1]]
        return (torch.cumsum(mask.long(), 0) - 1)[edge_index[:, ok]]
    if all_atoms:
        ar = _edge_store(graph, "atom", "receptor")
        a2r = ar.edge_index[1]
        atoms_keep = keep[a2r]
        new_a2r = (torch.cumsum(keep.long(), 0) - 1)[a2r][atoms_keep]
    graph["receptor"].pos = rec[keep]
    graph["receptor"].x = graph["receptor"].x[keep]
    if hasattr(graph["receptor"], "side_chain_vecs") and graph["receptor"].side_chain_vecs is not None:
        graph["receptor"].side_chain_vecs = graph["receptor"].side_chain_vecs[keep]
    rr = _edge_store(graph, "receptor", "receptor")
    rr.edge_index = sub_graph(keep, rr.edge_index)
    if all_atoms:
        graph["atom"].x = graph["atom"].x[atoms_keep]
        graph["atom"].pos = graph["atom"].pos[atoms_keep]
        aa = _edge_store(graph, "atom", "atom")
        aa.edge_index = sub_graph(atoms_keep, aa.edge_index)
        ar.edge_index = torch.stack([torch.arange(len(new_a2r), device=new_a2r.device), new_a2r])
    return graph


def step_coefficients(model_args, t_idx, inference_steps, schedules, ode=False, no_random=False, no_final_step_noise=False,
                      temp_sampling=1.0, temp_psi=0.0, temp_sigma_data=0.5):
    """Host float64 scalars of one step (utils/sampling.py:97-186): per component (score coefficient, noise
    coefficient).  Mirrors the in-library computation of ddmi_sample; used by the step-wise python loop."""
    three = lambda v: list(v) if hasattr(v, "__iter__") else [v] * 3
    T, psi, sdat = three(temp_sampling), three(temp_psi), three(temp_sigma_data)
    out = []
    last = t_idx == inference_steps - 1
    for i, (name, sched) in enumerate(zip(("tr", "rot", "tor"), schedules)):
        t = float(sched[t_idx])
        dt = t if last else t - float(sched[t_idx + 1])
        smin, smax = getattr(model_args, f"{name}_sigma_min"), getattr(model_args, f"{name}_sigma_max")
        sigma = smin ** (1 - t) * smax ** t
        g = sigma * np.sqrt(2 * np.log(smax / smin))
        a, z = (0.5 * g * g * dt if ode else g * g * dt), g * np.sqrt(dt)
        if T[i] != 1.0:
            sigma_data = np.exp(sdat[i] * np.log(smax) + (1 - sdat[i]) * np.log(smin))
            lam = (sigma_data + sigma) / (sigma_data + sigma / T[i])
            a, z = g * g * dt * (lam + T[i] * psi[i] / 2), g * np.sqrt(dt * (1 + psi[i]))
        if no_random or ode or (no_final_step_noise and last):
            z = 0.0
        out.append((float(a), float(z)))
    return out


def sampling(data_list, model, inference_steps, tr_schedule, rot_schedule, tor_schedule, device=None, t_to_sigma=None,
             model_args=None, no_random=False, ode=False, visualization_list=None, confidence_model=None,
             confidence_data_list=None, confidence_model_args=None, t_schedule=None, batch_size=32,
             no_final_step_noise=False, pivot=None, return_full_trajectory=False, temp_sampling=1.0, temp_psi=0.0,
             temp_sigma_data=0.5, return_features=False, seed=0, noise=None, sample_id_offset=0, native_loop=True):
    """utils/sampling.py:69-240.  Returns (data_list, confidence), or with `return_full_trajectory=True`
    (data_list, confidence, trajectory): float32 [inference_steps + 1, N, n, 3] on the poses' device, row 0 the initial poses,
    row k + 1 the poses after step k, coordinates centred as the model sees them (no original_center added; the reference
    asserts this flag away and never fills its `trajectory`).  `visualization_list`: one object with .add(coords, part, order)
    per pose, fed as utils/sampling.py:193-206 feeds PDBFile objects (host tensors, original_center added)."""
    want_steps = visualization_list is not None or return_full_trajectory
    _check_hooks(model, want_steps, pivot, return_features)
    trajectory = [] if return_full_trajectory else None
    confidence = [] if confidence_model is not None else None
    conf_batches = None
    conf_crop = getattr(confidence_model_args, "crop_beyond", None) if confidence_model_args is not None else None
    if confidence_model is not None and confidence_data_list is not None:
        conf_batches = iter([c for _, c in _batches(confidence_data_list, batch_size)])   # DataLoader order, sampling.py:87
    crop = getattr(model_args, "crop_beyond", None) if model_args is not None else getattr(model.cfg, "crop_beyond", None)
    N = len(data_list)
    schedules = (np.asarray(tr_schedule, dtype=np.float64), np.asarray(rot_schedule, dtype=np.float64),
                 np.asarray(tor_schedule, dtype=np.float64))
    cfg = model.cfg if model_args is None else model_args
    with torch.no_grad():
        for lo, chunk in _batches(data_list, batch_size):
            batch = _collate(chunk)
            b = batch.num_graphs
            n = batch["ligand"].pos.shape[0] // b
            if device is not None:
                batch = batch.to(device)
            ids = list(range(sample_id_offset + lo, sample_id_offset + lo + b))
            R = int(batch["ligand"].edge_mask.sum()) // b
            z = None
            if noise is not None:
                z = (noise[0][:, lo:lo + b], noise[1][:, lo:lo + b], noise[2][:, lo * R:(lo + b) * R])
            pos0 = batch["ligand"].pos
            bounds = [(i * n, (i + 1) * n) for i in range(b)]
            if native_loop and hasattr(model, "sample_batch"):
                # the device loop records the NaN counts always ([steps, 1] ints) and the per-step poses when they are asked for
                pos, step_pos, nan_count = _sample_batch(
                    model, want_steps, batch, inference_steps, schedules, noise=z, seed=seed, sample_ids=ids, ode=ode,
                    no_random=no_random, no_final_step_noise=no_final_step_noise, temp_sampling=temp_sampling, temp_psi=temp_psi,
                    temp_sigma_data=temp_sigma_data, crop_beyond=crop)
                if visualization_list is not None:   # one read of the device record after the loop
                    _visualise_steps(visualization_list, data_list, lo, step_pos.detach().cpu(), bounds)
            else:   # step-wise: model(batch) per step, exactly the reference's loop structure
                pos = batch["ligand"].pos
                step_list, nan_list = [], []
                try:
                    for t_idx in range(inference_steps):
                        set_time(batch, schedules[0][t_idx], schedules[1][t_idx], schedules[2][t_idx], b, device=pos.device)
                        batch["ligand"].pos = pos
                        if crop is not None:     # sampling.py:104-109: crop at 3*tr_sigma + crop_beyond, applied on the device
                            t = float(schedules[0][t_idx])
                            model.set_crop_cutoff(cfg.tr_sigma_min ** (1 - t) * cfg.tr_sigma_max ** t * 3 + crop)
                        tr, rot, tor = model(batch)[:3]
                        nan_list.append(torch.isnan(tr.mean(-1)).sum().reshape(1))
                        # NaN guard + update formulas (sampling.py:117-186) on the device, same kernel as the native loop
                        trp, rotp, torp = model.perturb(batch, tr, rot, tor, t_idx, inference_steps, schedules, noise=z, seed=seed,
                                                        sample_ids=ids, ode=ode, no_random=no_random,
                                                        no_final_step_noise=no_final_step_noise, temp_sampling=temp_sampling,
                                                        temp_psi=temp_psi, temp_sigma_data=temp_sigma_data)
                        pos = model.modify_conformer_batch(pos, batch, trp, rotp, torp)
                        if visualization_list is not None:   # sampling.py:193-198, fed as the loop goes
                            _visualise_steps(visualization_list, data_list, lo, pos.detach().cpu()[None], bounds, first_step=t_idx)
                        if return_full_trajectory:
                            step_list.append(pos)
                finally:
                    if crop is not None:
                        model.set_crop_cutoff(None)
                step_pos = torch.stack(step_list) if step_list else None
                nan_count = torch.stack(nan_list)
            _warn_nans(nan_count, [_complex_name(chunk[0])], [lo // batch_size + 1], [b])
            if return_full_trajectory:
                trajectory.append(torch.cat([pos0.to(step_pos.device, torch.float32)[None], step_pos], 0)
                                  .reshape(inference_steps + 1, b, n, 3))
            pos = pos.reshape(b, n, 3)
            for i in range(b):
                data_list[lo + i]["ligand"].pos = pos[i]
            if visualization_list is not None:
                _visualise_final(visualization_list, data_list)
            if confidence_model is not None:   # sampling.py:208-227
                if conf_batches is not None:
                    cgraphs = next(conf_batches)
                    alive = list(range(b))
                    if conf_crop is not None:   # sampling.py:213-217: every confidence graph cropped around ITS final pose
                        cgraphs = [g_.clone() for g_ in cgraphs]
                        alive = []
                        for i, g_ in enumerate(cgraphs):
                            g_["ligand"].pos = pos[i].detach().to(g_["receptor"].pos.device, g_["receptor"].pos.dtype)
                            try:
                                crop_beyond(g_, conf_crop, bool(getattr(confidence_model_args, "all_atoms", False)))
                                alive.append(i)
                            except ValueError:
                                # A pose that flew farther than the cutoff from EVERY residue has no receptor graph left to score.
                                # The reference hands such an empty graph to the confidence model; the built path cannot, so that
                                # ONE pose gets NaN (-> -1000 below, the value nan_to_num gives a failed pose) and the others of
                                # the batch are scored as usual.  Only a batch without any scorable pose raises.
                                pass
                        if not alive:
                            raise ValueError(f"crop_beyond({conf_crop}) removes every residue of every pose of the batch: nothing to score")
                    cbatch = _collate([cgraphs[i] for i in alive])
                    pos_alive = pos if len(alive) == b else pos[torch.as_tensor(alive, device=pos.device)]
                    cbatch["ligand"].pos = pos_alive.reshape(len(alive) * n, 3).to(cbatch["ligand"].pos.device)
                    if device is not None:
                        cbatch = cbatch.to(device)
                    set_time(cbatch, 0, 0, 0, len(alive), device=cbatch["ligand"].pos.device)
                    out = confidence_model(cbatch)
                    if len(alive) != b:   # graph-level outputs back in batch order, NaN for the poses that could not be scored
                        def scatter_rows(o):
                            full = torch.full((b,) + tuple(o.shape[1:]), float("nan"), device=o.device, dtype=o.dtype)
                            full[torch.as_tensor(alive, device=o.device)] = o
                            return full
                        out = (scatter_rows(out[0]),) + tuple(out[1:]) if isinstance(out, tuple) else scatter_rows(out)
                else:   # the sampling batch itself, still carrying the last step's times (sampling.py:113-114, 223)
                    batch["ligand"].pos = pos.reshape(b * n, 3)
                    set_time(batch, schedules[0][-1], schedules[1][-1], schedules[2][-1], b, device=batch["ligand"].pos.device)
                    out = confidence_model(batch)
                confidence.append(out[0] if isinstance(out, tuple) else out)
    if confidence is not None:
        confidence = torch.nan_to_num(torch.cat(confidence, dim=0), nan=-1000)
    if return_full_trajectory:
        return data_list, confidence, torch.cat(trajectory, 1)
    return data_list, confidence


def sample_poses(complex_graph, n_poses, model, inference_steps, tr_schedule, rot_schedule, tor_schedule, model_args=None,
                 batch_size=32, seed=0, sample_id_offset=0, initial_noise_std_proportion=-1.0, choose_residue=False, center=None,
                 confidence_model=None, confidence_graph=None, confidence_model_args=None, no_random=False, ode=False,
                 no_final_step_noise=False, temp_sampling=1.0, temp_psi=0.0, temp_sigma_data=0.5, return_full_trajectory=False,
                 visualization_list=None):
    """inference.py:239-242 + sampling() from ONE complex graph, with nothing per pose on the host: for each chunk of `batch_size`
    poses the batch is HeteroBatch.replicate(complex_graph, b) on the model's device, the initial poses are drawn there
    (model.randomize_position: no_torsion of the score model, no_random=False as inference.py passes them, sample ids
    sample_id_offset + lo + i), and model.sample_batch runs the step loop with the same ids, seed and crop_beyond handling as
    sampling().  Returns (pos, confidence) -- pos float32 [n_poses, n, 3] on the device, centred as the model sees it; confidence
    as sampling() returns it (None without a confidence model) -- and with `return_full_trajectory=True` a third value, the
    trajectory [inference_steps + 1, n_poses, n, 3] as sampling() defines it.  `no_random` ... `temp_sigma_data` are sampling()'s.

    With the initial poses of model.randomize_position written into n_poses clones, sampling(..., seed=seed,
    batch_size=batch_size) gives these poses bit for bit.

    center: None = mean residue position of the complex (the reference's default); or the pocket centre of `pocket_knowledge`.
    Confidence: the confidence model scores replicate(confidence_graph or complex_graph, b) with the final poses, at t = 0 with a
    confidence graph and at the last step's times without one (sampling()'s rule).  confidence_model_args.crop_beyond runs as the
    device crop (confidence_model.set_crop_cutoff) around each pose instead of sampling()'s per-graph host crop: the same kept
    residues, and a pose that keeps no residue is scored from its ligand rows alone instead of getting NaN.

    `visualization_list` is not served here (sampling() feeds it), nor are several complexes at once (sample_complexes)."""
    if visualization_list is not None:
        raise NotImplementedError("sample_poses does not feed a visualization_list: sampling() does (utils/sampling.py:193-206)")
    if n_poses < 1 or batch_size < 1:
        raise ValueError("n_poses and batch_size must be positive")
    if not hasattr(model, "randomize_position") or not hasattr(model, "sample_batch"):
        raise NotImplementedError("sample_poses needs a model with randomize_position and sample_batch (MIScoreModel)")
    cfg = model.cfg if model_args is None else model_args
    crop = getattr(model_args, "crop_beyond", None) if model_args is not None else getattr(model.cfg, "crop_beyond", None)
    conf_crop = getattr(confidence_model_args, "crop_beyond", None) if confidence_model_args is not None else None
    schedules = (np.asarray(tr_schedule, dtype=np.float64), np.asarray(rot_schedule, dtype=np.float64),
                 np.asarray(tor_schedule, dtype=np.float64))
    device = getattr(model, "device", None)
    n = int(complex_graph["ligand"].pos.shape[0])
    name = _complex_name(complex_graph)
    if center is None:
        center = complex_graph["receptor"].pos.mean(dim=0)
    batches, conf_batches = {}, {}   # one replicated batch per chunk size: the model keeps its static part between chunks

    def batch_of(cache, graph, b):
        if b not in cache:
            cache.clear()
            cache[b] = HeteroBatch.replicate(graph, b, device)
            cache[b]["ligand"].pos0 = cache[b]["ligand"].pos   # the conformer every chunk starts from
        return cache[b]
    poses, confidence, trajectory = [], [] if confidence_model is not None else None, []
    with torch.no_grad():
        for lo in range(0, n_poses, batch_size):
            b = min(batch_size, n_poses - lo)
            ids = list(range(sample_id_offset + lo, sample_id_offset + lo + b))
            batch = batch_of(batches, complex_graph, b)
            batch["ligand"].pos = batch["ligand"].pos0   # a batch kept from the chunk before carries that chunk's poses
            pos0 = model.randomize_position(batch, cfg.no_torsion, False, cfg.tr_sigma_max,
                                            initial_noise_std_proportion=initial_noise_std_proportion,
                                            choose_residue=choose_residue, center=center, seed=seed, sample_ids=ids)
            batch["ligand"].pos = pos0
            pos, step_pos, nan_count = _sample_batch(
                model, return_full_trajectory, batch, inference_steps, schedules, seed=seed, sample_ids=ids, ode=ode,
                no_random=no_random, no_final_step_noise=no_final_step_noise, temp_sampling=temp_sampling, temp_psi=temp_psi,
                temp_sigma_data=temp_sigma_data, crop_beyond=crop)
            _warn_nans(nan_count, [name], [lo // batch_size + 1], [b])
            if return_full_trajectory:
                trajectory.append(torch.cat([pos0[None], step_pos], 0).reshape(inference_steps + 1, b, n, 3))
            poses.append(pos.reshape(b, n, 3))
            if confidence_model is None:
                continue
            if confidence_graph is not None:
                cbatch = batch_of(conf_batches, confidence_graph, b)
                t = (0, 0, 0)
            else:   # the sampling graph, still carrying the last step's times (utils/sampling.py:113-114, 223)
                cbatch = batch
                t = (schedules[0][-1], schedules[1][-1], schedules[2][-1])
            cbatch["ligand"].pos = pos
            set_time(cbatch, *t, b, device=pos.device)
            if conf_crop is not None and confidence_graph is not None:   # sampling() crops confidence graphs only (utils/sampling.py:213-217)
                confidence_model.set_crop_cutoff(conf_crop)
            try:
                out = confidence_model(cbatch)
            finally:
                if conf_crop is not None and confidence_graph is not None:
                    confidence_model.set_crop_cutoff(None)
            confidence.append(out[0] if isinstance(out, tuple) else out)
    pos = torch.cat(poses, 0)
    if confidence is not None:
        confidence = torch.nan_to_num(torch.cat(confidence, dim=0), nan=-1000)
    if return_full_trajectory:
        return pos, confidence, torch.cat(trajectory, 1)
    return pos, confidence


def _pack(chunks, max_batch_graphs):
    """Whole chunks, in order, into device batches of at most max_batch_graphs graphs (a larger chunk runs alone)."""
    batches, cur, n = [], [], 0
    for ch in chunks:
        if cur and n + len(ch[2]) > max_batch_graphs:
            batches.append(cur)
            cur, n = [], 0
        cur.append(ch)
        n += len(ch[2])
    if cur:
        batches.append(cur)
    return batches


def sample_complexes(complex_data_lists, model, inference_steps, tr_schedule, rot_schedule, tor_schedule, device=None,
                     t_to_sigma=None, model_args=None, no_random=False, ode=False, visualization_list=None, confidence_model=None,
                     confidence_data_lists=None, confidence_model_args=None, batch_size=32, max_batch_graphs=40,
                     no_final_step_noise=False, pivot=None, return_full_trajectory=False, temp_sampling=1.0, temp_psi=0.0,
                     temp_sigma_data=0.5, return_features=False, seed=0, noise=None, native_loop=True):
    """`sampling()` over several complexes at once: returns [(data_list, confidence), ...], one entry per complex.

    Each complex's data_list is cut into the chunks of `batch_size` poses that sampling() would run; each chunk is one NaN-guard
    group (utils/sampling.py:117-131 runs per sampling() batch).  Whole chunks are packed, in order, into device batches of at
    most `max_batch_graphs` graphs, and every device batch runs one step loop (model.sample_batch, or the step-wise model(batch)
    loop with native_loop=False).  Final poses are written back into each data_list as sampling() does, and the confidence model
    scores each packed batch with sampling()'s per-pose crop handling.

    Sample ids: pose i of complex k uses sample id offset_k + i, offset_k = the number of poses of the complexes before it, so
    complex k gets exactly the draws of sampling(complex_data_lists[k], ..., seed=seed, sample_id_offset=offset_k).
    `noise` = one (z_tr [steps,N_k,3], z_rot [steps,N_k,3], z_tor [steps,N_k*R_k]) per complex, laid out as sampling()'s.

    `visualization_list` = one visualisation list per complex; each receives exactly the calls sampling() of that complex alone
    makes (utils/sampling.py:193-206, a chunk at a time: its steps, then the order=2 pass over the complex's whole list), fed
    after each device batch's loop on both routes.  `return_full_trajectory=True` appends a third entry to every complex's
    tuple: float32 [inference_steps + 1, N_k, n_k, 3] as sampling() defines it.  The NaN warning names the complex and the
    sampling() batch number of the chunk whose guard fired."""
    want_steps = visualization_list is not None or return_full_trajectory
    _check_hooks(model, want_steps, pivot, return_features)
    if max_batch_graphs < 1 or batch_size < 1:
        raise ValueError("batch_size and max_batch_graphs must be positive")
    lists = list(complex_data_lists)
    if visualization_list is not None and len(visualization_list) != len(lists):
        raise ValueError("visualization_list: one list per complex")
    trajectory = [[] for _ in lists] if return_full_trajectory else None
    if noise is not None and len(noise) != len(lists):
        raise ValueError("noise: one (z_tr, z_rot, z_tor) per complex")
    if confidence_data_lists is not None and len(confidence_data_lists) != len(lists):
        raise ValueError("confidence_data_lists: one list per complex")
    conf_crop = getattr(confidence_model_args, "crop_beyond", None) if confidence_model_args is not None else None
    crop = getattr(model_args, "crop_beyond", None) if model_args is not None else getattr(model.cfg, "crop_beyond", None)
    schedules = (np.asarray(tr_schedule, dtype=np.float64), np.asarray(rot_schedule, dtype=np.float64),
                 np.asarray(tor_schedule, dtype=np.float64))
    cfg = model.cfg if model_args is None else model_args
    offsets = np.concatenate([[0], np.cumsum([len(dl) for dl in lists])]).astype(int).tolist()
    chunks = [(k, lo, chunk) for k, dl in enumerate(lists) for lo, chunk in _batches(dl, batch_size)]
    confidence = [[] for _ in lists] if confidence_model is not None else None
    with torch.no_grad():
        for members in _pack(chunks, max_batch_graphs):
            graphs = [g for _, _, chunk in members for g in chunk]
            sizes = [len(chunk) for _, _, chunk in members]
            b = len(graphs)
            batch = _collate(graphs)
            if device is not None:
                batch = batch.to(device)
            ids = [offsets[k] + lo + i for k, lo, chunk in members for i in range(len(chunk))]
            z = None
            if noise is not None:
                parts = []
                for k, lo, chunk in members:
                    R = int(sum(int(g["ligand"].edge_mask.sum()) for g in chunk)) // len(chunk)
                    zk = noise[k]
                    parts.append((zk[0][:, lo:lo + len(chunk)], zk[1][:, lo:lo + len(chunk)], zk[2][:, lo * R:(lo + len(chunk)) * R]))
                z = tuple(torch.cat([torch.as_tensor(p[i]) for p in parts], 1) for i in range(3))
            pos0 = batch["ligand"].pos
            if native_loop and hasattr(model, "sample_batch"):
                pos, step_pos, nan_count = _sample_batch(
                    model, want_steps, batch, inference_steps, schedules, noise=z, seed=seed, sample_ids=ids, ode=ode,
                    no_random=no_random, no_final_step_noise=no_final_step_noise, temp_sampling=temp_sampling, temp_psi=temp_psi,
                    temp_sigma_data=temp_sigma_data, crop_beyond=crop, groups=sizes)
            else:   # step-wise, as sampling()'s: the NaN guard of model.perturb runs per chunk
                pos = batch["ligand"].pos
                step_list, nan_list = [], []
                group_of = torch.repeat_interleave(torch.arange(len(sizes)), torch.as_tensor(sizes))
                try:
                    for t_idx in range(inference_steps):
                        set_time(batch, schedules[0][t_idx], schedules[1][t_idx], schedules[2][t_idx], b, device=pos.device)
                        batch["ligand"].pos = pos
                        if crop is not None:
                            t = float(schedules[0][t_idx])
                            model.set_crop_cutoff(cfg.tr_sigma_min ** (1 - t) * cfg.tr_sigma_max ** t * 3 + crop)
                        tr, rot, tor = model(batch)[:3]
                        failed = torch.isnan(tr.mean(-1)).to(torch.int64)
                        nan_list.append(torch.zeros(len(sizes), dtype=torch.int64, device=failed.device)
                                        .index_add_(0, group_of.to(failed.device), failed))
                        trp, rotp, torp = model.perturb(batch, tr, rot, tor, t_idx, inference_steps, schedules, noise=z, seed=seed,
                                                        sample_ids=ids, ode=ode, no_random=no_random,
                                                        no_final_step_noise=no_final_step_noise, temp_sampling=temp_sampling,
                                                        temp_psi=temp_psi, temp_sigma_data=temp_sigma_data, groups=sizes)
                        pos = model.modify_conformer_batch(pos, batch, trp, rotp, torp)
                        if want_steps:
                            step_list.append(pos)
                finally:
                    if crop is not None:
                        model.set_crop_cutoff(None)
                step_pos = torch.stack(step_list) if step_list else None
                nan_count = torch.stack(nan_list)
            _warn_nans(nan_count, [_complex_name(chunk[0]) for _, _, chunk in members],
                       [lo // batch_size + 1 for _, lo, _ in members], sizes)
            n_l = [int(g["ligand"].pos.shape[0]) for g in graphs]
            pos_g = torch.split(pos, n_l)
            atom_ptr = np.concatenate([[0], np.cumsum(n_l)]).astype(int).tolist()
            step_host = step_pos.detach().cpu() if visualization_list is not None else None
            j = 0
            for k, lo, chunk in members:   # a chunk = one sampling() batch of complex k: steps, write-back, whole-list pass
                a0, a1 = atom_ptr[j], atom_ptr[j + len(chunk)]
                if visualization_list is not None:
                    _visualise_steps(visualization_list[k], lists[k], lo, step_host[:, a0:a1],
                                     [(atom_ptr[j + i] - a0, atom_ptr[j + i + 1] - a0) for i in range(len(chunk))])
                if return_full_trajectory:   # the poses of one complex have the same number of atoms
                    both = torch.cat([pos0[a0:a1].to(step_pos.device, torch.float32)[None], step_pos[:, a0:a1]], 0)
                    trajectory[k].append(both.reshape(inference_steps + 1, len(chunk), n_l[j], 3))
                for i in range(len(chunk)):
                    lists[k][lo + i]["ligand"].pos = pos_g[j]
                    j += 1
                if visualization_list is not None:
                    _visualise_final(visualization_list[k], lists[k])
            if confidence_model is None:
                continue
            if confidence_data_lists is not None:   # sampling.py:208-227 on the packed confidence graphs
                cgraphs = [g for k, lo, chunk in members for g in confidence_data_lists[k][lo:lo + len(chunk)]]
                alive = list(range(b))
                if conf_crop is not None:   # every confidence graph cropped around ITS final pose; see sampling()
                    cgraphs = [g_.clone() for g_ in cgraphs]
                    alive = []
                    for i, g_ in enumerate(cgraphs):
                        g_["ligand"].pos = pos_g[i].detach().to(g_["receptor"].pos.device, g_["receptor"].pos.dtype)
                        try:
                            crop_beyond(g_, conf_crop, bool(getattr(confidence_model_args, "all_atoms", False)))
                            alive.append(i)
                        except ValueError:
                            pass
                    if not alive:
                        raise ValueError(f"crop_beyond({conf_crop}) removes every residue of every pose of the batch: nothing to score")
                cbatch = _collate([cgraphs[i] for i in alive])
                cbatch["ligand"].pos = torch.cat([pos_g[i] for i in alive], 0).to(cbatch["ligand"].pos.device)
                if device is not None:
                    cbatch = cbatch.to(device)
                set_time(cbatch, 0, 0, 0, len(alive), device=cbatch["ligand"].pos.device)
                out = confidence_model(cbatch)
                out = out[0] if isinstance(out, tuple) else out
                if len(alive) != b:   # graph-level outputs back in batch order, NaN for the poses that could not be scored
                    full = torch.full((b,) + tuple(out.shape[1:]), float("nan"), device=out.device, dtype=out.dtype)
                    full[torch.as_tensor(alive, device=out.device)] = out
                    out = full
            else:   # the sampling batch itself, still carrying the last step's times
                batch["ligand"].pos = pos
                set_time(batch, schedules[0][-1], schedules[1][-1], schedules[2][-1], b, device=batch["ligand"].pos.device)
                out = confidence_model(batch)
                out = out[0] if isinstance(out, tuple) else out
            row = 0
            for (k, _, _), n in zip(members, sizes):
                confidence[k].append(out[row:row + n])
                row += n
    out = [(dl, None if confidence is None else torch.nan_to_num(torch.cat(confidence[k], dim=0), nan=-1000))
           for k, dl in enumerate(lists)]
    if return_full_trajectory:
        out = [o + (torch.cat(trajectory[k], 1),) for k, o in enumerate(out)]
    return out
