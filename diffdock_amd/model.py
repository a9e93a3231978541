"""`MIScoreModel`: drop-in for the reference score model object.

The reference boundary for this path is a Python duck type:
    model = get_model(args, device, t_to_sigma, no_parallel=True)      utils/utils.py:172
    model.load_state_dict(sd, strict=True); model.to(device); model.eval()   inference.py:202-205
    tr, rot, tor = model(batch)[:3]                                    utils/sampling.py:116
`MIScoreModel` keeps that surface (same state_dict keys, same call signature, same return
tuple `(tr[B,3], rot[B,3], tor[sum R], None)`) and forwards to libddmi.so through ctypes.
PyTorch is used only as the owner of device memory and of the current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import weakref
from types import SimpleNamespace
from typing import Dict, Optional

import numpy as np
import torch

from . import lib as _lib
from .config import ModelConfig, config_from_args
from .hetero import as_numpy_mask


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def time_frequencies(sigma_embed_dim: int) -> torch.Tensor:
    """Frequencies of sinusoidal_embedding, computed with the reference's exact fp32 op sequence
    (utils/diffusion_utils.py:101-103) so the device phases are bit-identical."""
    half = sigma_embed_dim // 2
    emb = math.log(10000) / (half - 1)
    return torch.exp(torch.arange(half, dtype=torch.float32) * -emb)


def _mask_fingerprint(mr):
    """Key of the rotatable-bond masks (numpy arrays / tensors, possibly a list per graph).  Host arrays are keyed by CONTENT (an
    id() can be recycled after the old list is collected, and in-place edits leave it unchanged; hashing them is a host-side
    memcpy).  DEVICE tensors are keyed by (storage address, in-place version counter, shape): hashing their content would put a
    blocking device-to-host copy in front of every forward of the step-wise loop."""
    import hashlib
    import numpy as np
    if mr is None:
        return None
    h = hashlib.sha1()
    for a in (mr if isinstance(mr, (list, tuple)) else [mr]):
        if torch.is_tensor(a) and a.device.type != "cpu":
            h.update(repr((a.data_ptr(), 0 if a.is_inference() else a._version, tuple(a.shape), str(a.dtype))).encode())
            continue
        a = a.detach().numpy() if torch.is_tensor(a) else np.asarray(a)
        h.update(str(a.shape).encode())
        h.update(np.ascontiguousarray(a).view(np.uint8).tobytes() if a.size else b"")
    return h.hexdigest()


def _graph_masks(mr_attr, B):
    """The rotatable-bond mask of every graph of a collated batch (a list with one entry per graph, each a [R_b, Nl_b] array
    or a list of one), as numpy bool arrays; None when the batch does not carry one mask per graph."""
    if isinstance(mr_attr, (list, tuple)) and len(mr_attr) == B:
        return [as_numpy_mask(x) for x in mr_attr]
    return None


class MIScoreModel:
    def __init__(self, cfg: ModelConfig, device="cuda:0", lib_path: str | None = None):
        self.cfg = cfg
        self.device = torch.device(device)
        self.lib = _lib.load(lib_path)
        self._h = C.c_void_p()
        dev_index = self.device.index or 0 if self.device.type == "cuda" else 0
        _lib.check(self.lib, self.lib.ddmi_create(C.byref(_lib.make_config(cfg)), dev_index, C.byref(self._h)))
        self._complex_key = None
        self._complex_ref = None
        self._keep = None
        self._layout = None   # ddmi_set_batch_layout state of the current complex (see _ensure_layout)
        self._state: Dict[str, torch.Tensor] = {}
        self._tables_set = False
        self.training = False

    # ------------------------------------------------------------------ nn.Module-like surface
    def eval(self):
        return self

    def to(self, device):
        assert torch.device(device).type == self.device.type, "a handle is bound to its device at construction"
        return self

    def parameters(self):
        return iter(self._state.values())

    def state_dict(self):
        return dict(self._state)

    def expected_keys(self):
        n = self.lib.ddmi_num_weights(self._h)
        out = {}
        for i in range(n):
            key, shape, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
            _lib.check(self.lib, self.lib.ddmi_weight_spec(self._h, i, C.byref(key), shape, C.byref(nd)))
            out[key.value.decode()] = tuple(shape[:nd.value])
        return out

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        expected = self.expected_keys()
        # e3nn keeps constant buffers under *.tp.* / final_tp_tor.* in real checkpoints, and nn.BatchNorm1d (confidence
        # predictors, cg_model.py:184-207) its `num_batches_tracked` step counter: neither is a weight
        # ... e3nn's o3.Linear registers an `output_mask` buffer (and an empty `bias`) next to `weight`; a confidence-mode module
        # built with sidechain_pred owns a sidechain_predictor its forward never calls (cg_model.py:173-178 vs 353-366)
        given = {k: v for k, v in sd.items() if ".tp." not in k and not k.startswith("final_tp_tor.")
                 and not k.endswith("num_batches_tracked") and not k.endswith(".output_mask")
                 and not (k.endswith((".linear_2.bias", "sidechain_predictor.bias")) and v.numel() == 0)
                 and not (self.cfg.confidence_mode and k.startswith("sidechain_predictor."))}
        missing = [k for k in expected if k not in given]
        unexpected = [k for k in given if k not in expected]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing[:5]} unexpected {unexpected[:5]}")
        freq = time_frequencies(self.cfg.sigma_embed_dim).contiguous()
        _lib.check(self.lib, self.lib.ddmi_set_time_frequencies(self._h, _ptr(freq), freq.numel()))
        for k in expected:
            if k not in given:
                continue
            t = given[k].detach().to("cpu", torch.float32).contiguous()
            shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
            _lib.check(self.lib, self.lib.ddmi_set_weight(self._h, k.encode(), _ptr(t), shape, t.dim()))
            self._state[k] = t
        _lib.check(self.lib, self.lib.ddmi_commit_weights(self._h))
        self.invalidate_complex()
        return self

    def invalidate_complex(self):
        """Forget the cached ddmi_set_complex: the next model(batch) rebuilds the static part of the batch."""
        self._complex_key = None
        self._complex_ref = None

    def set_tables(self, so3_exp_score_norms: np.ndarray, torus_score_norm: np.ndarray):
        """Score-norm tables (utils/so3.py:59, utils/torus.py:72-76); see diffdock_amd/tables.py."""
        for kind, tab in ((0, so3_exp_score_norms), (1, torus_score_norm)):
            tab = np.ascontiguousarray(tab, dtype=np.float64)
            _lib.check(self.lib, self.lib.ddmi_set_table(self._h, kind, tab.ctypes.data, tab.size))
        self._tables_set = True
        return self

    def __del__(self):
        try:
            if self._h:
                self.lib.ddmi_destroy(self._h)
        except Exception:
            pass

    # ------------------------------------------------------------------ batch -> ddmi_complex
    def _stream(self):
        if self.device.type == "cuda":
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return None

    def _keep_alive(self, tensors):
        """Tensors that enqueued work reads must outlive it: on a CUDA device they are recorded on the current stream."""
        if self.device.type == "cuda":
            for t in tensors:
                if t is not None:
                    t.record_stream(torch.cuda.current_stream(self.device))

    def _call_cfg(self, fn, cfg, inputs, outputs, empty_is_null=False):
        """fn(handle, cfg, stream) with the pointer fields of `cfg` set from the tensors of the two dicts by field name (None, and with
        `empty_is_null` an empty tensor, = NULL); the converted copies in `inputs` are kept alive.  Returns `outputs`."""
        for name, t in list(inputs.items()) + list(outputs.items()):
            setattr(cfg, name, None if t is None or (empty_is_null and t.numel() == 0) else t.data_ptr())
        _lib.check(self.lib, fn(self._h, C.byref(cfg), self._stream()))
        self._keep_alive(inputs.values())
        return outputs

    def _static_tensors(self, data):
        lig, rec = data["ligand"], data["receptor"]
        bond, rr = data["ligand", "ligand"], data["receptor", "receptor"]
        ts = [rec.x, rec.pos, lig.x, lig.batch, rec.batch, lig.edge_mask, bond.edge_index, bond.edge_attr, rr.edge_index]
        if self.cfg.all_atoms:
            ts += [data["atom"].x, data["atom"].pos, data["atom"].batch, data["atom", "atom"].edge_index, data["atom", "receptor"].edge_index]
        return ts

    def _ensure_complex(self, data):
        """ddmi_set_complex once per batch OBJECT.  One model is reused over many complexes (inference.py:224-303) and the
        caching allocator hands a freed batch's addresses to the next one, so addresses and shapes cannot identify a
        batch: the cache is keyed on the identity of the live batch object (weak reference) plus the in-place version
        counters of its static tensors; a batch type that cannot be weakly referenced is fingerprinted by content."""
        lig, rec = data["ligand"], data["receptor"]
        bond, rr = data["ligand", "ligand"], data["receptor", "receptor"]
        static = self._static_tensors(data)
        # (tensors created under torch.inference_mode() carry no version counter: their slot of the key is 0)
        key = tuple((t.data_ptr(), 0 if t.is_inference() else t._version, tuple(t.shape)) for t in static) + (int(data.num_graphs),)
        # rotatable-bond masks (numpy arrays / tensors, possibly a list per graph): keyed by CONTENT -- an id() can be recycled
        # after the old list is collected, and in-place edits leave it unchanged
        key = key + (_mask_fingerprint(getattr(lig, "mask_rotate", None)),)
        same_obj = self._complex_ref is not None and self._complex_ref() is data
        if same_obj and key == self._complex_key:
            return
        try:
            ref = weakref.ref(data)
        except TypeError:    # no weak references: content fingerprint of the static tensors (one host read-back per call)
            ref = None
            key = key + tuple(float(t.double().sum()) + float((t.double() * t.double()).sum()) for t in static)
            if key == self._complex_key:
                return
        if not self._tables_set:
            from .tables import default_tables
            self.set_tables(*default_tables())
        dev = self.device
        B = int(data.num_graphs)

        def ptr_of(batch_vec, n):
            cnt = torch.bincount(batch_vec.to("cpu"), minlength=B)
            p = torch.zeros(B + 1, dtype=torch.int32)
            p[1:] = torch.cumsum(cnt, 0)
            assert int(p[-1]) == n
            return p
        lig_ptr, rec_ptr = ptr_of(lig.batch, lig.pos.shape[0]), ptr_of(rec.batch, rec.pos.shape[0])
        i32 = lambda t: t.to(dev, torch.int32).contiguous()
        f32 = lambda t: t.to(dev, torch.float32).contiguous()
        edge_mask = lig.edge_mask.to(dev, torch.uint8).contiguous()
        n_tor = int(lig.edge_mask.sum())
        mask_rotate = None
        mr_attr = getattr(lig, "mask_rotate", None) if hasattr(lig, "mask_rotate") else None
        # per graph: atoms, rotatable bonds (graph-local ends, edge order) and mask -- a batch of copies of one complex keeps the
        # single-mask path of ddmi_set_complex; any other batch gets every graph's own mask through ddmi_set_batch_layout
        n_l = (lig_ptr[1:] - lig_ptr[:-1]).tolist()
        tor_ends = bond.edge_index[:, lig.edge_mask.to(bond.edge_index.device).bool()].to("cpu")
        tor_graph = lig.batch.to("cpu")[tor_ends[0]]
        tor_local = [(tor_ends[:, tor_graph == b] - int(lig_ptr[b])) for b in range(B)]
        masks = _graph_masks(mr_attr, B)
        if masks is not None and not all(m.shape == (t.shape[1], n) or (t.shape[1] == 0 and m.size == 0)
                                         for m, t, n in zip(masks, tor_local, n_l)):
            masks = None
        copies = all(n == n_l[0] and torch.equal(t, tor_local[0]) for n, t in zip(n_l, tor_local)) and \
            (masks is None or all(np.array_equal(m, masks[0]) for m in masks))
        if mr_attr is not None and copies:
            mr = as_numpy_mask(mr_attr)
            if mr.size and mr.shape[0] * B == n_tor and mr.shape[1] * B == lig.pos.shape[0]:
                mask_rotate = torch.from_numpy(np.ascontiguousarray(mr.astype(np.uint8))).to(dev)
        keep = dict(lig_ptr=lig_ptr, rec_ptr=rec_ptr, lig_x=i32(lig.x[:, :16]), bond_index=i32(bond.edge_index),
                    bond_attr=f32(bond.edge_attr), edge_mask=edge_mask,
                    rec_x=f32(rec.x * 0 if self.cfg.no_aminoacid_identities else rec.x), rec_pos=f32(rec.pos),   # cg_model.py:309-310
                    rec_edge_index=i32(rr.edge_index), mask_rotate=mask_rotate)
        c = _lib.Complex()
        c.num_graphs, c.n_lig, c.n_rec = B, lig.pos.shape[0], rec.pos.shape[0]
        c.n_bond_edges, c.n_rec_edges, c.n_tor = bond.edge_index.shape[1], rr.edge_index.shape[1], n_tor
        names = ["lig_ptr", "rec_ptr", "lig_x", "bond_index", "bond_attr", "edge_mask", "rec_x", "rec_pos",
                 "rec_edge_index", "mask_rotate"]
        if self.cfg.all_atoms:   # receptor heavy atoms and their static relations (models/aa_model.py:291-303)
            atom, aa, ar = data["atom"], data["atom", "atom"], data["atom", "receptor"]
            keep.update(atom_ptr=ptr_of(atom.batch, atom.pos.shape[0]), atom_x=i32(atom.x[:, :4]), atom_pos=f32(atom.pos),
                        atom_edge_index=i32(aa.edge_index), atom_rec_edge_index=i32(ar.edge_index))
            c.n_atom, c.n_atom_edges, c.n_atom_rec_edges = atom.pos.shape[0], aa.edge_index.shape[1], ar.edge_index.shape[1]
            names += ["atom_ptr", "atom_x", "atom_pos", "atom_edge_index", "atom_rec_edge_index"]
        for name in names:
            setattr(c, name, keep[name].data_ptr() if keep[name] is not None else None)
        self._complex_key = self._layout = None
        _lib.check(self.lib, self.lib.ddmi_set_complex(self._h, C.byref(c), self._stream()))
        self._keep, self._complex_key, self._complex_ref = keep, key, ref
        self._B, self._n_tor, self._n_lig = B, n_tor, lig.pos.shape[0]
        self._copies, self._graph_masks = copies, masks
        if not copies and (masks is not None or self.cfg.no_torsion or n_tor == 0):
            self._ensure_layout(None)

    def _ensure_layout(self, groups):
        """ddmi_set_batch_layout for the current complex when the step loop needs it: a batch that is not made of copies of one
        complex (every graph's own mask), or NaN-guard groups other than the whole batch.  `groups` = graphs per group in batch
        order (None = one group)."""
        sizes = (self._B,) if groups is None else tuple(int(g) for g in groups)
        if sum(sizes) != self._B or min(sizes) <= 0:
            raise ValueError(f"groups {sizes} do not partition the {self._B} graphs of the batch")
        if sizes == self._layout or (self._copies and self._layout is None and len(sizes) == 1):
            return
        mask = None
        if not self.cfg.no_torsion and self._n_tor > 0:
            if self._graph_masks is None:
                raise _lib.DdmiError("a batch of several complexes (or several NaN-guard groups) needs the batch's per-graph "
                                     "mask_rotate list with one [R_b, Nl_b] mask per graph")
            blocks = [np.ascontiguousarray(m.astype(np.uint8)).reshape(-1) for m in self._graph_masks]
            mask = torch.from_numpy(np.concatenate(blocks)).to(self.device)
        _lib.set_batch_layout(self.lib, self._h, sizes, mask, self._stream())
        self._layout = sizes

    # ------------------------------------------------------------------ model(batch)
    def __call__(self, data):
        self._ensure_complex(data)
        dev = self.device
        pos = data["ligand"].pos.to(dev, torch.float32).contiguous()
        t = [data.complex_t[k].to(dev, torch.float32).contiguous() for k in ("tr", "rot", "tor")]
        if self.cfg.confidence_mode:   # (confidence, atom_confidence) -- models/cg_model.py:353-366
            n_out = self.cfg.num_confidence_outputs + (1 if self.cfg.affinity_prediction else 0)
            conf = torch.empty(self._B, n_out, device=dev)
            atom = torch.empty(self._n_lig, self.cfg.atom_num_confidence_outputs, device=dev) if self.cfg.atom_confidence else None
            _lib.check(self.lib, self.lib.ddmi_confidence(self._h, _ptr(pos), _ptr(t[0]), _ptr(t[1]), _ptr(t[2]), _ptr(conf),
                                                          None if atom is None else _ptr(atom), self._stream()))
            if self.cfg.old:   # the legacy class returns the bare tensor (old_cg_model.py:287-291)
                return conf.squeeze(-1)
            return conf.squeeze(-1), (atom if atom is not None else torch.zeros(self._n_lig, device=dev))
        tr = torch.empty(self._B, 3, device=dev)
        rot = torch.empty(self._B, 3, device=dev)
        no_tor = self.cfg.no_torsion or self._n_tor == 0
        tor = torch.empty(0 if no_tor else self._n_tor, device=dev)
        _lib.check(self.lib, self.lib.ddmi_forward(self._h, _ptr(pos), _ptr(t[0]), _ptr(t[1]), _ptr(t[2]), _ptr(tr),
                                                   _ptr(rot), None if no_tor else _ptr(tor), self._stream()))
        if self.cfg.old:   # the legacy class returns a 3-tuple (old_cg_model.py:329,352)
            return tr, rot, tor
        side = None
        if self.cfg.sidechain_pred:   # models/cg_model.py:397-402: [n_rec, 10]
            side = torch.empty(int(data["receptor"].pos.shape[0]), 10, device=dev)
            _lib.check(self.lib, self.lib.ddmi_sidechain_pred(self._h, _ptr(side), self._stream()))
            if getattr(self, "_crop_cutoff", 0.0) > 0.0:   # the reference crops the graph first: rows of the kept residues only
                side = side[torch.from_numpy(self.debug_buffer("crop_keep") != 0).to(dev)]
        return tr, rot, tor, side

    forward = __call__

    def set_crop_cutoff(self, cutoff):
        """crop_beyond(graph, cutoff) for the following model(batch) calls (utils/utils.py:388-413); None / 0 = off."""
        self._crop_cutoff = float(cutoff or 0.0)
        _lib.check(self.lib, self.lib.ddmi_set_crop_cutoff(self._h, self._crop_cutoff))

    def modify_conformer_batch(self, pos, data, tr_update, rot_update, torsion_updates, mask_rotate=None):
        """utils/diffusion_utils.py:60-78 on the device (same argument order; mask_rotate comes from the batch)."""
        self._ensure_complex(data)
        dev = self.device
        out = pos.to(dev, torch.float32).contiguous().clone()
        f = lambda x: None if x is None else x.to(dev, torch.float32).contiguous()
        tr_u, rot_u, tor_u = f(tr_update), f(rot_update), f(torsion_updates)
        _lib.check(self.lib, self.lib.ddmi_modify_conformer(self._h, _ptr(out), _ptr(tr_u), _ptr(rot_u), _ptr(tor_u),
                                                            self._stream()))
        return out

    def randomize_position(self, data, no_torsion, no_random, tr_sigma_max, initial_noise_std_proportion=-1.0,
                           choose_residue=False, center=None, seed=0, sample_ids=None, draws=None):
        """randomize_position (utils/sampling.py:16-58, the argument order of the reference) for every graph of the collated
        batch, on the device (ddmi_randomize_position): returns the initial poses [n_lig, 3]; `data` is left as it is.

        center: None = the mean residue position of graph 0, used for every graph as the reference uses data_list[0]'s (the batch
        must then hold copies of one complex); or [3] / [B, 3], e.g. the pocket centre of `pocket_knowledge`, which the caller
        computes with the reference's rule (utils/sampling.py:20-29).  The translation std is computed here from the reference's two
        formulas (std_rec * prop / 1.73 with std_rec of graph 0's receptor, or -prop * tr_sigma_max).  Draws: keyed by
        (seed, sample id, step -1, component) as include/ddmi.h lists them, `sample_ids` = one id per graph (default 0..B-1), so a
        pose does not depend on how the run is batched or sharded; or injected through `draws` = dict(torsion=[per graph: R
        angles], rotation=[per graph: 3x3], tr=[per graph: (1,3) translation]) as synth.randomize_position takes them (any
        subset)."""
        self._ensure_complex(data)
        dev = self.device
        B = self._B
        n0 = int(self._keep["rec_ptr"][1])
        rec0 = None   # graph 0's residues on the host (float32 torch arithmetic there, as the reference's: the same on every device)
        if center is None or initial_noise_std_proportion >= 0.0:
            rec0 = data["receptor"].pos[:n0].detach().to("cpu", torch.float32)
        if center is None:
            if not self._copies:
                raise ValueError("randomize_position: a batch of several complexes needs an explicit center [B, 3]")
            center = rec0.mean(dim=0)
        ctr = torch.as_tensor(center).detach().to("cpu", torch.float32).reshape(-1, 3)
        ctr = np.ascontiguousarray(ctr.expand(B, 3).numpy() if ctr.shape[0] == 1 else ctr.numpy())
        if ctr.shape != (B, 3):
            raise ValueError(f"center: [3] or [{B}, 3] expected, got {tuple(ctr.shape)}")
        rc = _lib.RandomizeCfg()
        rc.struct_size = C.sizeof(_lib.RandomizeCfg)
        rc.no_torsion, rc.no_random, rc.choose_residue = int(bool(no_torsion)), int(bool(no_random)), int(bool(choose_residue))
        if initial_noise_std_proportion >= 0.0:   # utils/sampling.py:52-54
            if not self._copies and not choose_residue and not no_random:
                raise ValueError("randomize_position: initial_noise_std_proportion >= 0 scales by one receptor's extent; a batch of "
                                 "several complexes takes tr_sigma_max (a negative proportion) or injected translations")
            std_rec = float(torch.sqrt(torch.mean(torch.sum(rec0 ** 2, dim=1))))
            rc.tr_std = std_rec * initial_noise_std_proportion / 1.73
        else:
            rc.tr_std = -initial_noise_std_proportion * tr_sigma_max
        rc.center = ctr.ctypes.data
        rc.seed = int(seed)
        ids = None
        if sample_ids is not None:
            ids = np.ascontiguousarray(np.asarray(sample_ids, dtype=np.int64))
            assert ids.size == B, "one sample id per graph of the batch"
            rc.sample_ids = ids.ctypes.data
        injected = []
        if draws is not None:
            def dev_f32(parts, shape):
                t = torch.cat([torch.as_tensor(np.asarray(p, dtype=np.float64)).reshape(-1) for p in parts]) if len(parts) else torch.zeros(0)
                assert t.numel() == shape, (t.numel(), shape)
                t = t.to(dev, torch.float32).contiguous()
                injected.append(t)
                return t.data_ptr() if t.numel() else None
            n_tor = 0 if no_torsion else self._n_tor
            if draws.get("torsion") is not None and n_tor:
                rc.tor_updates = dev_f32(draws["torsion"], n_tor)
            if draws.get("rotation") is not None:
                rc.rotations = dev_f32(draws["rotation"], 9 * B)
            if draws.get("tr") is not None:
                rc.tr_updates = dev_f32(draws["tr"], 3 * B)
        pos = data["ligand"].pos.to(dev, torch.float32).contiguous().clone()
        _lib.check(self.lib, self.lib.ddmi_randomize_position(self._h, _ptr(pos), C.byref(rc), self._stream()))
        self._keep_alive(injected)   # the injected draws must outlive the enqueued kernel
        return pos

    def _pose_inputs(self, pos, ref, perm, atom_index):
        """The shared inputs of pose_metrics / pose_fit on the device, checked: pos, ref [K, m, 3], perm, atom_index, lead, n, m."""
        dev = self.device
        pos = torch.as_tensor(pos).to(dev, torch.float32).contiguous()
        if pos.dim() not in (3, 4) or pos.shape[-1] != 3:
            raise ValueError(f"pos: [P, n, 3] or [T, P, n, 3] expected, got {tuple(pos.shape)}")
        lead, n = tuple(pos.shape[:-2]), pos.shape[-2]
        ref = torch.as_tensor(ref).to(dev, torch.float32).contiguous()
        ref = ref.unsqueeze(0) if ref.dim() == 2 else ref
        i32 = lambda t: None if t is None else torch.as_tensor(t).to(dev, torch.int32).contiguous()
        perm, atom_index = i32(perm), i32(atom_index)
        m = n if atom_index is None else atom_index.numel()
        if ref.dim() != 3 or tuple(ref.shape[1:]) != (m, 3):
            raise ValueError(f"ref: [K, {m}, 3] expected, got {tuple(ref.shape)}")
        if perm is not None and (perm.dim() != 2 or perm.shape[1] != m):
            raise ValueError(f"perm: [S, {m}] expected, got {tuple(perm.shape)}")
        return pos, ref, perm, atom_index, lead, n, m

    def pose_fit(self, pos, ref, perm=None, atom_index=None, per_ref=False):
        """The minimised symmetric RMSD and the fitting transform (ddmi_pose_fit; spyrmsd.rmsd.symmrmsd with minimize=True): inputs
        as for `pose_metrics`.  Returns a dict of device tensors with the leading shape of `pos`: rmsd_min (the RMSD after the best
        rigid superposition, min over references and rows of perm; exactly 0 where the reference's atol rule gives 0), best_min
        [.., 2] int32 (the reference and the row attaining it; ties go to the lowest), rotation [.., 3, 3] and translation [.., 3]
        of that superposition (`metrics.superpose` applies them), and with per_ref rmsd_min_per_ref [.., K].  The call needs no
        complex and does not synchronise."""
        dev = self.device
        pos, ref, perm, atom_index, lead, n, m = self._pose_inputs(pos, ref, perm, atom_index)
        P, K = int(np.prod(lead)), ref.shape[0]
        f = lambda *shape, dtype=torch.float32: torch.empty(lead + shape, dtype=dtype, device=dev)
        out = dict(rmsd_min=f(), best_min=f(2, dtype=torch.int32), rotation=f(3, 3), translation=f(3))
        if per_ref:
            out["rmsd_min_per_ref"] = f(K)
        fc = _lib.PoseFitCfg()
        fc.struct_size = C.sizeof(_lib.PoseFitCfg)
        fc.n_poses, fc.n_atoms, fc.n_kept, fc.n_refs = P, n, m, K
        fc.n_perms = 0 if perm is None else perm.shape[0]
        return self._call_cfg(self.lib.ddmi_pose_fit, fc, dict(pos=pos, ref=ref, perm=perm, atom_index=atom_index), out)

    def match_conformer(self, start, target, lig_ptr, tor_ptr=None, rot_u=None, rot_v=None, mask_rotate=None, popsize=15, maxiter=500,
                        tol=0.01, seed=0, job_ids=None, init_angles=None, n_init=0):
        """Conformer matching on the device (ddmi_match_conformer; datasets/conformer_matching.py): a ragged batch of J jobs, job j
        owning the atoms lig_ptr[j]:lig_ptr[j + 1] of `start` / `target` [sum n, 3] and the rotatable bonds tor_ptr[j]:tor_ptr[j + 1]
        of `rot_u` / `rot_v` (job-local atom indices); `mask_rotate` holds every job's [R_j, n_j] block, flattened, in job order
        (`matching.torsion_table` builds the three).  `init_angles` [sum_j n_init * R_j] gives job j's first n_init population rows;
        they must lie in [-pi, pi] and are used as given, neither clamped nor wrapped.
        Returns a dict of device tensors: angles [sum R], rmsd [J], pos [sum n, 3] (the matched conformer in the frame of target),
        best_history [J, maxiter + 1], n_generations [J] and, with n_init, init_energy [J, n_init].  Needs no complex and does not
        synchronise; the result of a job depends on its inputs, its `job_ids` entry (default: its index) and `seed` alone."""
        dev = self.device
        start = torch.as_tensor(start).to(dev, torch.float32).contiguous()
        target = torch.as_tensor(target).to(dev, torch.float32).contiguous()
        lig = np.ascontiguousarray(np.asarray(lig_ptr).reshape(-1), dtype=np.int32)
        J = len(lig) - 1
        tor = np.zeros(J + 1, dtype=np.int32) if tor_ptr is None else np.ascontiguousarray(np.asarray(tor_ptr).reshape(-1), dtype=np.int32)
        if len(tor) != J + 1:
            raise ValueError(f"tor_ptr: [{J + 1}] expected, got {len(tor)}")
        N, nT = (int(lig[-1]), int(tor[-1])) if J >= 1 else (0, 0)
        if start.dim() != 2 or start.shape[1] != 3 or (J >= 1 and start.shape[0] != N):
            raise ValueError(f"start: [{N}, 3] expected, got {tuple(start.shape)}")
        if target.shape != start.shape:
            raise ValueError(f"target: {tuple(start.shape)} expected, got {tuple(target.shape)}")
        i32 = lambda t: None if t is None else torch.as_tensor(t).to(dev, torch.int32).reshape(-1).contiguous()
        rot_u, rot_v = i32(rot_u), i32(rot_v)
        for name, t in (("rot_u", rot_u), ("rot_v", rot_v)):
            if t is not None and t.numel() != nT:
                raise ValueError(f"{name}: [{nT}] expected, got {t.numel()}")
        mask_bytes = int(np.sum(np.diff(tor.astype(np.int64)) * np.diff(lig.astype(np.int64)))) if J >= 1 else 0
        if mask_rotate is not None:
            mask_rotate = torch.as_tensor(mask_rotate).to(dev, torch.uint8).reshape(-1).contiguous()
            if mask_rotate.numel() != mask_bytes:
                raise ValueError(f"mask_rotate: {mask_bytes} bytes (every job's [R, n] block) expected, got {mask_rotate.numel()}")
        n_init = int(n_init)
        if init_angles is not None:
            init_angles = torch.as_tensor(init_angles).to(dev, torch.float32).reshape(-1).contiguous()
            if n_init < 1 or init_angles.numel() != n_init * nT:
                raise ValueError(f"init_angles: n_init >= 1 and {max(n_init, 0) * nT} angles expected, got n_init = {n_init}, {init_angles.numel()}")
        ids = None if job_ids is None else np.ascontiguousarray(np.asarray(job_ids).reshape(-1), dtype=np.int64)
        if ids is not None and len(ids) != J:
            raise ValueError(f"job_ids: [{J}] expected, got {len(ids)}")
        H = max(int(maxiter), 0) + 1
        f = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
        out = dict(angles=f(nT), rmsd=f(max(J, 0)), pos=f(N, 3), best_history=f(max(J, 0), H), n_generations=f(max(J, 0), dtype=torch.int32))
        if n_init > 0:
            out["init_energy"] = f(max(J, 0), n_init)
        mc = _lib.MatchCfg()
        mc.struct_size = C.sizeof(_lib.MatchCfg)
        mc.n_jobs, mc.popsize, mc.maxiter, mc.n_init, mc.tol, mc.seed = J, int(popsize), int(maxiter), n_init, float(tol), int(seed)
        mc.lig_ptr, mc.tor_ptr = lig.ctypes.data, tor.ctypes.data
        mc.job_ids = None if ids is None else ids.ctypes.data
        inputs = dict(start=start, target=target, rot_u=rot_u, rot_v=rot_v, mask_rotate=mask_rotate, init_angles=init_angles)
        return self._call_cfg(self.lib.ddmi_match_conformer, mc, inputs, out, empty_is_null=True)

    def pose_metrics(self, pos, ref, perm=None, atom_index=None, points=None, per_ref=False):
        """Judge poses on the device (ddmi_pose_metrics; evaluate.py:474-505): `pos` [P, n, 3] or a trajectory [T, P, n, 3], `ref`
        [K, m, 3] (or [m, 3]) known poses, `perm` int [S, m] graph isomorphisms as metrics.isomorphisms returns them (None = the
        identity), `atom_index` int [m] the atoms of a pose that are compared, in the order of `ref` (None = all n; the reference's
        filterHs), `points` [Q, 3] anything to keep clear of.  Returns a dict of device tensors with the leading shape of `pos`:
        rmsd (symmetry-corrected, min over references), best [.., 2] int32 (the reference and the row of perm attaining it; ties go
        to the lowest), rmsd_plain (identity only), centroid_distance, min_self_distance (+inf for one atom), min_point_distance
        (+inf without points), and with per_ref rmsd_per_ref [.., K].  The call needs no complex and does not synchronise."""
        dev = self.device
        pos, ref, perm, atom_index, lead, n, m = self._pose_inputs(pos, ref, perm, atom_index)
        if points is not None:
            points = torch.as_tensor(points).to(dev, torch.float32).reshape(-1, 3).contiguous()
            points = points if points.numel() else None
        P, K = int(np.prod(lead)), ref.shape[0]
        f = lambda *shape, dtype=torch.float32: torch.empty(lead + shape, dtype=dtype, device=dev)
        out = dict(rmsd=f(), best=f(2, dtype=torch.int32), rmsd_plain=f(), centroid_distance=f(), min_self_distance=f(),
                   min_point_distance=f())
        if per_ref:
            out["rmsd_per_ref"] = f(K)
        mc = _lib.PoseMetricsCfg()
        mc.struct_size = C.sizeof(_lib.PoseMetricsCfg)
        mc.n_poses, mc.n_atoms, mc.n_kept, mc.n_refs = P, n, m, K
        mc.n_perms = 0 if perm is None else perm.shape[0]
        mc.n_points = 0 if points is None else points.shape[0]
        inputs = dict(pos=pos, ref=ref, perm=perm, atom_index=atom_index, points=points)
        return self._call_cfg(self.lib.ddmi_pose_metrics, mc, inputs, out)

    def neighbor_graph(self, pos, cutoff, max_neighbors=None, ptr=None):
        """Capped neighbour lists on the device (ddmi_neighbor_graph; the loop of new_extract_receptor_structure,
        datasets/process_mols.py:171-192 and :207-228): `pos` [N, 3]; `ptr` [G + 1] (host integers) splits the rows into G
        independent point sets (None = one set); `cutoff` and `max_neighbors` are one value or one per set (None / 0 = the
        reference's 1000).  Returns (edge_index [2, E] int64 = [neighbour; centre] ordered by centre, global row numbers, and deg [N]
        int32) as device tensors.  The library call does not synchronise; this wrapper reads the edge total once to shape the result
        (an uncapped set: once to size the buffer, before the columns are written).  The call needs no complex."""
        dev = self.device
        pos = torch.as_tensor(pos).to(dev, torch.float32).reshape(-1, 3).contiguous()
        N = pos.shape[0]
        ptr = np.ascontiguousarray([0, N] if ptr is None else np.asarray(ptr).reshape(-1), dtype=np.int32)
        G = len(ptr) - 1
        per_set = lambda v, dt: None if np.ndim(v) == 0 else np.ascontiguousarray(np.asarray([0 if x is None else x for x in v]), dtype=dt)
        cut, cap = per_set(cutoff, np.float32), per_set(max_neighbors, np.int32)
        for name, arr in (("cutoff", cut), ("max_neighbors", cap)):
            if arr is not None and len(arr) != G:
                raise ValueError(f"{name}: one value or one per set ({G}) expected, got {len(arr)}")
        caps = np.full(max(G, 0), int(max_neighbors or 0), dtype=np.int64) if cap is None else cap.astype(np.int64)
        n = np.diff(ptr.astype(np.int64)) if G >= 1 else np.zeros(0, dtype=np.int64)
        bound = int(np.sum(np.maximum(n, 0) * np.minimum(np.where(caps > 0, caps, 1000), np.maximum(n - 1, 0))))
        deg = torch.empty(N, dtype=torch.int32, device=dev)
        n_edges = torch.zeros(1, dtype=torch.int32, device=dev)
        nc = _lib.NeighborGraphCfg()
        nc.struct_size = C.sizeof(_lib.NeighborGraphCfg)
        nc.n_nodes, nc.n_sets = N, G
        nc.max_neighbors = 0 if cap is not None else int(max_neighbors or 0)
        nc.cutoff = 0.0 if cut is not None else float(cutoff)
        nc.pos, nc.ptr = pos.data_ptr() if N else None, ptr.ctypes.data
        nc.set_cutoff = None if cut is None else cut.ctypes.data
        nc.set_max_neighbors = None if cap is None else cap.ctypes.data
        nc.deg, nc.n_edges = deg.data_ptr() if N else None, n_edges.data_ptr()

        def call(edge):
            nc.capacity = 0 if edge is None else edge.shape[1]
            nc.edge_index = None if edge is None or edge.numel() == 0 else edge.data_ptr()
            _lib.check(self.lib, self.lib.ddmi_neighbor_graph(self._h, C.byref(nc), self._stream()))
        if bool((caps > 0).all()) and 0 < bound < (1 << 31):     # E <= bound is known before the call: one call, nothing read before it
            edge = torch.empty(2, bound, dtype=torch.int64, device=dev)
            call(edge)
            E = int(n_edges.item())
            edge = edge[:, :E].contiguous()
        else:
            call(None)
            E = int(n_edges.item())
            edge = torch.empty(2, E, dtype=torch.int64, device=dev)
            if E:
                call(edge)
        self._keep_alive([pos])
        return edge, deg

    def _sample_cfg(self, inference_steps, schedules, noise, seed, sample_ids, ode, no_random, no_final_step_noise,
                    temp_sampling, temp_psi, temp_sigma_data, crop_beyond):
        """ddmi_sample_cfg + the host / device arrays it points into (returned so that they outlive the call)."""
        dev = self.device
        sc = _lib.SampleCfg()
        sched = [np.ascontiguousarray(np.asarray(s, dtype=np.float64)) for s in schedules]
        sc.inference_steps = inference_steps
        sc.tr_schedule, sc.rot_schedule, sc.tor_schedule = (s.ctypes.data for s in sched)
        sc.ode, sc.no_random, sc.no_final_step_noise = int(ode), int(no_random), int(no_final_step_noise)
        three = lambda v: list(v) if hasattr(v, "__iter__") else [v] * 3
        for name, v in (("temp_sampling", temp_sampling), ("temp_psi", temp_psi), ("temp_sigma_data", temp_sigma_data)):
            arr = getattr(sc, name)
            for i, x in enumerate(three(v)):
                arr[i] = float(x)
        sc.seed = int(seed)
        sc.use_crop, sc.crop_beyond = (0, 0.0) if crop_beyond is None else (1, float(crop_beyond))
        ids = None
        if sample_ids is not None:
            ids = np.ascontiguousarray(np.asarray(sample_ids, dtype=np.int64))
            assert ids.size == self._B, "one sample id per graph of the batch"
            sc.sample_ids = ids.ctypes.data
        zs = [None, None, None]
        if noise is not None:
            zs = [None if z is None else z.to(dev, torch.float32).contiguous() for z in noise]
            sc.z_tr, sc.z_rot, sc.z_tor = (None if z is None else z.data_ptr() for z in zs)
        return sc, (sched, ids, zs)

    def sample_batch(self, data, inference_steps, schedules, noise=None, seed=0, sample_ids=None, ode=False,
                     no_random=False, no_final_step_noise=False, temp_sampling=1.0, temp_psi=0.0, temp_sigma_data=0.5,
                     crop_beyond=None, groups=None, record=None):
        """The whole step loop of sampling() (utils/sampling.py:96-191) for one collated batch, on the device.  `groups` = graphs
        per NaN-guard group in batch order (default: the whole batch is one group, as one sampling() batch).

        `record` = True, or a subset of {"pos", "scores", "nan"}: the kernels of the loop also write what they hold at every step
        into device tensors (ddmi_set_sample_record; no extra launch or synchronisation, final poses bit-identical), and the call
        returns (pos, rec) with rec.pos [steps, n_lig, 3] the poses AFTER step k, rec.tr / rec.rot [steps, B, 3] and rec.tor
        [steps, n_tor] the scores of step k behind the NaN guard, rec.nan_count [steps, G] int32 the poses per NaN-guard group
        whose mean tr score was NaN; parts not requested are None.  Without `record` the return value is the poses alone."""
        self._ensure_complex(data)
        self._ensure_layout(groups)
        pos = data["ligand"].pos.to(self.device, torch.float32).contiguous().clone()
        sc, keep = self._sample_cfg(inference_steps, schedules, noise, seed, sample_ids, ode, no_random, no_final_step_noise,
                                    temp_sampling, temp_psi, temp_sigma_data, crop_beyond)
        rec = None
        if record:
            rec = self._new_record(inference_steps, {"pos", "scores", "nan"} if record is True else set(record))
            _lib.set_sample_record(self.lib, self._h, inference_steps, rec.pos, rec.tr, rec.rot, rec.tor, rec.nan_count)
        try:
            _lib.check(self.lib, self.lib.ddmi_sample(self._h, _ptr(pos), C.byref(sc), self._stream()))
        finally:
            if rec is not None:
                _lib.set_sample_record(self.lib, self._h, off=True)
        self._keep_alive(keep[2])   # the injected draws must outlive the enqueued steps
        return pos if rec is None else (pos, rec)

    def _new_record(self, steps, parts):
        """Device tensors of a per-step record of the current complex (see sample_batch); zero-filled."""
        if not parts <= {"pos", "scores", "nan"}:
            raise ValueError(f"record: True or a subset of 'pos', 'scores', 'nan', got {sorted(parts)}")
        dev, B = self.device, self._B
        n_tor = 0 if self.cfg.no_torsion else self._n_tor
        G = len(self._layout) if self._layout is not None else 1
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
        sc = "scores" in parts
        return SimpleNamespace(pos=z(steps, self._n_lig, 3) if "pos" in parts else None,
                               tr=z(steps, B, 3) if sc else None, rot=z(steps, B, 3) if sc else None,
                               tor=z(steps, n_tor) if sc else None,
                               nan_count=z(steps, G, dtype=torch.int32) if "nan" in parts else None)

    def perturb(self, data, tr_score, rot_score, tor_score, t_idx, inference_steps, schedules, noise=None, seed=0,
                sample_ids=None, ode=False, no_random=False, no_final_step_noise=False, temp_sampling=1.0, temp_psi=0.0,
                temp_sigma_data=0.5, groups=None):
        """Scores of step t_idx -> (tr_perturb, rot_perturb, tor_perturb): NaN guard + update formulas of
        utils/sampling.py:117-186 on the device (ddmi_perturb).  `noise` = (z_tr [steps,B,3], z_rot [steps,B,3], z_tor [steps,n_tor]).
        `groups` = graphs per NaN-guard group (the guard runs per group; default one group)."""
        self._ensure_complex(data)
        self._ensure_layout(groups)
        dev = self.device
        f = lambda x: x.to(dev, torch.float32).contiguous().clone()
        tr, rot = f(tr_score), f(rot_score)
        tor = f(tor_score) if (tor_score is not None and tor_score.numel()) else None
        sc, keep = self._sample_cfg(inference_steps, schedules, noise, seed, sample_ids, ode, no_random, no_final_step_noise,
                                    temp_sampling, temp_psi, temp_sigma_data, None)
        _lib.check(self.lib, self.lib.ddmi_perturb(self._h, _ptr(tr), _ptr(rot), _ptr(tor), C.byref(sc), int(t_idx), self._stream()))
        self._keep_alive(keep[2])
        return tr, rot, tor

    # ------------------------------------------------------------------ introspection
    def set_kernel_timing(self, enabled, level: int | None = None):
        """level 1 = one row per kernel name, 2 = k_conv_fused per edge group, 3 = per (layer, edge group); the harness variable
        DDMI_TIME_GROUPS=1|2 selects level 2 | 3 (profiling scripts under tools/)."""
        if level is None:
            tg = os.environ.get("DDMI_TIME_GROUPS")
            level = 1 if not tg else (3 if int(tg) >= 2 else 2)
        _lib.check(self.lib, self.lib.ddmi_set_kernel_timing(self._h, level if enabled else 0))

    def kernel_timings(self):
        """{phase: (total_ms, launches)} measured with HIP events on the launch stream."""
        out, i = {}, 0
        while True:
            name, ms, n = C.c_char_p(), C.c_double(), C.c_int64()
            if self.lib.ddmi_kernel_timings(self._h, i, C.byref(name), C.byref(ms), C.byref(n)) != 0:
                break
            out[name.value.decode()] = (ms.value, n.value)
            i += 1
        return out

    def debug_buffer(self, name: str) -> np.ndarray:
        shape, nd, is_int = (C.c_int64 * 4)(), C.c_int(), C.c_int()
        _lib.check(self.lib, self.lib.ddmi_debug_shape(self._h, name.encode(), shape, C.byref(nd), C.byref(is_int)))
        arr = np.empty(tuple(shape[:nd.value]), dtype=np.int32 if is_int.value else np.float32)
        _lib.check(self.lib, self.lib.ddmi_debug_read(self._h, name.encode(), arr.ctypes.data, arr.nbytes, self._stream()))
        return arr


def get_model(args, device, t_to_sigma=None, no_parallel=True, confidence_mode=False, old=False, lib_path=None):
    """Same signature as the reference factory (utils/utils.py:172).  `t_to_sigma` is accepted for
    compatibility; the geometric schedule it implements (utils/diffusion_utils.py:28-32) is evaluated
    in-library from the sigma bounds in `args`."""
    cfg = args if isinstance(args, ModelConfig) else config_from_args(args)
    if old:   # utils/utils.py:180-219: CGOldModel, or AAOldModel on all-atom graphs; no sh_lmax / embedding-layer / pseudoscalar
        # arguments reach either; rec_max_radius and center_max_distance keep the class defaults (30 / 30 = ModelConfig's)
        parallel = getattr(args, "parallel", 1) if not isinstance(args, ModelConfig) else 1
        if parallel not in (1, None):   # (config_from_args refuses it for a namespace; kept here for any other args object)
            raise NotImplementedError("get_model arguments outside the built path: parallel > 1")
        cfg = cfg.replace(old=True, confidence_mode=bool(confidence_mode), sh_lmax=2, num_prot_emb_layers=0,
                          depthwise_convolution=False, sidechain_pred=False,   # (not among the arguments get_model(old=True) passes, utils/utils.py:180-219)
                          reduce_pseudoscalars=False,
                          # CGOldModel has one confidence output; AAOldModel as many as get_model passes (old_aa_model.py:120-127)
                          num_confidence_outputs=cfg.num_confidence_outputs if cfg.all_atoms else 1,
                          use_old_atom_encoder=getattr(args, "use_old_atom_encoder", True) if not isinstance(args, ModelConfig)
                          else cfg.use_old_atom_encoder)
        if not cfg.use_old_atom_encoder:
            raise NotImplementedError(("AAOldModel" if cfg.all_atoms else "CGOldModel") + " with the new AtomEncoder cannot be "
                                      "constructed by the reference either (AtomEncoder has no lm_embedding_type argument)")
    elif not cfg.embed_also_ligand and not cfg.all_atoms:
        # CGModel.ligand_embedding asserts it on every forward (models/cg_model.py:263, "otherwise reimplement padding").
        # AAModel has no such assert: without ligand embedding layers it zero-pads the ligand rows to the receptor width
        # (models/aa_model.py:351-357) -- a no-op when num_prot_emb_layers == 0, which is the case accepted here (config.py)
        raise AssertionError("embed_also_ligand must be set for the CGModel class (models/cg_model.py:263)")
    if confidence_mode != cfg.confidence_mode:
        cfg = cfg.replace(confidence_mode=bool(confidence_mode))
    return MIScoreModel(cfg, device=device, lib_path=lib_path)
