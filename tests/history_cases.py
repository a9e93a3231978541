"""History scripts: ONE model handle serves many complexes, forwards, step loops, crops, guard groups and in-place edits in a row, and
every call must equal the same call on a handle created for that call alone, bit for bit (the library is deterministic: no atomics on
the numeric path).  Backend-independent like tests/cases.py: `make(cfg, sd)` returns a loaded MIScoreModel, `place` moves a batch to
the model's device; tests/test_emu_history.py runs the scripts on the CPU emulation build, tests/test_gpu_history.py on the MI355X.

A script is a list of steps `(batch key, operation, arguments)` run by `History.run`.  The used handle keeps one live batch object per
key (collated again only by a "new" step); the fresh twin of a step is a new handle on a batch collated from the same seeds with the
same in-place edits applied.  Besides the outputs every step compares the device's edge / virtual-node lists with the fresh handle's
and asserts the state it claims to exercise (shared rec-rec list, crop mask, batch layout), and the first step of every operation
kind of a script is also compared with the float64 oracle, so "used and new agree" cannot mean "both wrong".

Poison pass: `("poison", ...)` runs a forward of a LARGER complex on the used handle whose language-model columns of `receptor.x` are
NaN (where the configuration reads them) and whose bond `edge_attr` is 1e30.  No index is derived from either (edge_attr feeds the
ligand edge MLP only; column 0 of receptor.x, the residue type, stays), positions and times stay finite.  edge_attr carries 1e30 and
not NaN because the ReLU of the edge MLPs is an fmaxf, which turns NaN into 0: NaN bond features leave every score finite, 1e30
overflows in the layers behind.  Non-finite values then fill the pool's edge embeddings, hidden rows, messages and node tables, so a
later read of memory the current complex did not write shows up as NaN / inf or as a bit difference.  (Configurations without
language-model columns -- cases._ddl, the DDL width -- are poisoned through edge_attr alone.)

Where a step must NOT run the shared layer-0 rec-rec list, `vn_off_rr0` is all zero (or does not exist) on the fresh handle and on a
used handle whose complex is new.  On a LIVE batch that has shared before, the list stays built (it is a static_topo list, built
once per complex), so there the offsets cannot tell; a step that shares where it must not reads graph 0's messages for every graph,
under other times or another crop, and fails the bit comparison."""
import copy

import numpy as np
import pytest
import torch

from diffdock_amd import lib as _l
from diffdock_amd.config import TINY
from diffdock_amd.hetero import HeteroBatch
from diffdock_amd.lib import DdmiError
from diffdock_amd.synth import make_complex, make_pose_list
from diffdock_amd.weights import init_state_dict
from oracle.conformer import get_t_schedule
from oracle.conformer import modify_conformer_batch as oracle_modify
from oracle.sampling import crop_beyond as oracle_crop
from oracle.sampling import nan_guard, perturbations
from oracle.sampling import sampling as oracle_sampling
from cases import MIXED_T, TEMP, _ddl
from util import assert_scores_close, oracle_model, rmsd, set_times

F64 = torch.float64
# (the full rec-rec list, vn_off_rr, is not among them: a two-layer model whose first layer shares never builds it)
LISTS = ("offs_l", "goff_ll", "vn_off_cross", "vn_off_rl", "vn_off_ll")
# all-atom models: the ligand<->atom pair lists (per forward) and the three static atom relations (static_topo: built once per complex)
ATOM_LISTS = ("offs_la_l", "offs_la_a", "vn_off_la", "vn_off_al", "vn_off_ra", "vn_off_aa", "vn_off_ar")
STATIC_ATOM_LISTS = ("vn_off_ra", "vn_off_aa", "vn_off_ar")


# ---------------------------------------------------------------------------------------------------------------- batches
def copies(seed, n_res, n_lig, B, all_atoms=False, atoms_per_res=(2, 5)):
    """B poses of one synthetic complex (a batch of copies: the uniform kernels, the shared rec-rec list)."""
    return dict(kind="copies", seed=seed, n_res=n_res, n_lig=n_lig, B=B, all_atoms=all_atoms, atoms_per_res=atoms_per_res)


def packed(n_poses=(2, 1, 2)):
    """Poses of three DIFFERENT ligands in one batch (pack_cases.ragged_complexes: R_b = 2, 5, 2): the ragged kernels."""
    return dict(kind="packed", n_poses=tuple(n_poses))


def graphs_of(spec, cfg):
    if spec["kind"] == "packed":
        from pack_cases import ragged_complexes
        out = []
        for k, (g, n) in enumerate(zip(ragged_complexes()[1:], spec["n_poses"])):
            if not cfg.lm_embedding_type:
                g["receptor"].x = g["receptor"].x[:, :1].clone()
            out += make_pose_list(g, n, tr_sigma_max=5.0, seed=10 + k, initial_noise_std_proportion=0.4)
        return out
    kw = dict(all_atoms=True, atoms_per_res=spec["atoms_per_res"]) if spec["all_atoms"] else {}
    g = make_complex(seed=spec["seed"], n_res=spec["n_res"], n_lig=spec["n_lig"], lm_dim=cfg.lm_embedding_dim, **kw)
    return make_pose_list(g, spec["B"], tr_sigma_max=5.0, seed=spec["seed"] + 1000, initial_noise_std_proportion=0.3)


# ---- in-place edits of a collated batch (script 4); each works on the batch's own tensors, on whichever device they live
def _rows(batch, nt, b):
    idx = torch.nonzero(batch[nt].batch == b).flatten()
    return int(idx[0]), int(idx[-1]) + 1


def edit_rec_x_one(batch):        # graph 1's residues get other features: not a batch of receptor copies any more
    lo, hi = _rows(batch, "receptor", 1)
    x = batch["receptor"].x
    x[lo:hi] = x[lo:hi].roll(1, 0).clone()


def edit_rec_pos_one(batch):      # one residue of graph 1 moved (the contact graph, an input, stays)
    lo, _ = _rows(batch, "receptor", 1)
    batch["receptor"].pos[lo + 2, 0] += 0.25


def edit_rec_pos_back(batch):
    lo, _ = _rows(batch, "receptor", 1)
    lo0, _ = _rows(batch, "receptor", 0)
    batch["receptor"].pos[lo + 2] = batch["receptor"].pos[lo0 + 2].clone()


def edit_rec_x_back(batch):       # graph 0's rows written over graph 1's: copies again
    lo, hi = _rows(batch, "receptor", 1)
    lo0, hi0 = _rows(batch, "receptor", 0)
    batch["receptor"].x[lo:hi] = batch["receptor"].x[lo0:hi0].clone()


def edit_mask_rotate(batch):      # the first rotatable bond of every graph turns its other side
    for m in batch["ligand"].mask_rotate:
        m = m[0] if isinstance(m, (list, tuple)) else m
        m[0] = ~m[0]


def edit_edge_mask(batch):        # the last rotatable bond of every graph becomes rigid (mask rows follow)
    lig = batch["ligand"]
    em = lig.edge_mask
    eb = lig.batch[batch["ligand", "ligand"].edge_index[0]]
    for b in range(batch.num_graphs):
        idx = torch.nonzero(em & (eb == b)).flatten()
        em[idx[-1]] = False
    lig.mask_rotate = [np.ascontiguousarray((m[0] if isinstance(m, (list, tuple)) else m)[:-1]) for m in lig.mask_rotate]


def bits_equal(a, b):
    """Bit-for-bit equality (NaN included)."""
    a, b = a.contiguous(), b.contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def max_diff(x, y):
    """For a failure message: the largest difference of two outputs (NaN counts as 1e30), or their shapes."""
    if x.shape != y.shape or not x.numel():
        return f"shapes {tuple(x.shape)} / {tuple(y.shape)}"
    return f"max |d| {float((x.double() - y.double()).abs().nan_to_num(nan=1e30).max()):.3e}"


def _freeze(x):
    if isinstance(x, dict):
        return tuple(sorted((k, _freeze(v)) for k, v in x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(_freeze(v) for v in x)
    return x


class History:
    def __init__(self, make, place, cfg, sd_seed=3, make_fresh=None, listing=None, share="auto", name="", route_lines=True):
        """`share`: whether the loops of a batch of >= 2 copies must run the shared layer-0 rec-rec list ("auto": yes; False: the
        route options of this run switch it off; None: the model class has no such list, only equality with the fresh handle)."""
        self.make, self.place, self.cfg, self.name = make, place, cfg, name
        self.make_fresh = make_fresh or make
        self.sd = init_state_dict(cfg, seed=sd_seed)
        self.used = make(cfg, self.sd)
        self.listing = listing          # () -> text printed since the last call (the `ddmi route` lines under DDMI_DEBUG_GRAN)
        self.share = share
        self.route_lines = route_lines  # False: the grouped dispatch (exec.grouped = 2) prints no per-group route line; None: a width
                                        # where only some layers take the grouped dispatch (equality with the fresh handle only)
        self.spec, self.edits, self.live = {}, {}, {}
        self.fresh = {}                 # (spec, edits, op, args) -> (outputs, state)
        self.oracle_done = set()
        self.owner = None               # key of the batch the used handle's complex was built from
        self.shared_built = False       # the live complex of the used handle has run the shared group since it was built
        self.poison_twin = False
        self.log = []

    # ------------------------------------------------------------------------------------------------------------ batches
    def collate(self, key, device=True):
        b = HeteroBatch.from_data_list(graphs_of(self.spec[key], self.cfg))
        for e in self.edits[key]:
            e(b)
        return self.place(b) if device else b

    def graphs(self, key):
        """The batch's graphs on the host, edits included (for the oracle): the edits run on a collated host batch, and what they
        touch (receptor features and positions, edge_mask, mask_rotate) is written back into the graphs."""
        graphs = graphs_of(self.spec[key], self.cfg)
        if not self.edits[key]:
            return graphs
        hb = self.collate(key, device=False)
        eb = hb["ligand"].batch[hb["ligand", "ligand"].edge_index[0]]
        for b, g in enumerate(graphs):
            lo, hi = _rows(hb, "receptor", b)
            g["receptor"].x, g["receptor"].pos = hb["receptor"].x[lo:hi].clone(), hb["receptor"].pos[lo:hi].clone()
            g["ligand"].edge_mask = hb["ligand"].edge_mask[eb == b].clone()
            m = hb["ligand"].mask_rotate[b]
            g["ligand"].mask_rotate = [np.asarray(m[0] if isinstance(m, (list, tuple)) else m)]
        return graphs

    # ------------------------------------------------------------------------------------------------------------ operations
    def _times(self, B, t):
        if t == "mixed":
            return [[MIXED_T[k][i % 3] for i in range(B)] for k in ("tr", "rot", "tor")]
        return [t, t, t]

    def _noise(self, batch, steps, seed):
        B, R = batch.num_graphs, int(batch["ligand"].edge_mask.sum())
        gen = torch.Generator().manual_seed(seed)
        return (torch.randn(steps, B, 3, generator=gen), torch.randn(steps, B, 3, generator=gen), torch.randn(steps, R, generator=gen))

    def _scores(self, batch, seed, nan=True):
        B, R = batch.num_graphs, int(batch["ligand"].edge_mask.sum())
        gen = torch.Generator().manual_seed(seed)
        tr, rot, tor = torch.randn(B, 3, generator=gen), torch.randn(B, 3, generator=gen), torch.randn(R, generator=gen)
        if nan:
            tr[B - 1, 1] = float("nan")
            rot[B - 1, 0] = float("nan")
            if R > 1:
                tor[R - 1] = float("nan")
                tor[0] = float("inf")
        return tr, rot, tor

    def apply(self, model, batch, op, a):
        """One operation on (model, batch): the list of its output tensors, on the host."""
        B = batch.num_graphs
        if op == "forward":
            set_times(batch, *self._times(B, a.get("t", 0.6)))
            if a.get("crop"):
                model.set_crop_cutoff(a["crop"])
            try:
                out = model(batch)
            finally:
                if a.get("crop"):
                    model.set_crop_cutoff(None)
            out = out if isinstance(out, tuple) else (out,)
        elif op == "sample":
            steps = a.get("steps", 2)
            s = get_t_schedule(steps)
            noise = self._noise(batch, steps, a.get("noise_seed", 4)) if a.get("noise", True) else None
            out = (model.sample_batch(batch, steps, (s, s, s), noise=noise, seed=a.get("seed", 11), sample_ids=list(range(B)),
                                      no_final_step_noise=True, crop_beyond=a.get("crop_beyond"), groups=a.get("groups"), **TEMP),)
        elif op == "perturb":
            steps, k = 5, a.get("k", 1)
            s = get_t_schedule(steps)
            out = model.perturb(batch, *self._scores(batch, 8), k, steps, (s, s, s), noise=self._noise(batch, steps, 9),
                                no_final_step_noise=True, groups=a.get("groups"), **TEMP)
        elif op == "modify":
            tr, rot, tor = self._scores(batch, 17, nan=False)
            out = (model.modify_conformer_batch(batch["ligand"].pos, batch, tr, rot * 0.7, tor if tor.numel() else None),)
        else:
            raise ValueError(op)
        return [o.detach().cpu().clone() for o in out if o is not None]

    def state(self, model, op):
        """What the device holds after a forward or a loop: edge / virtual-node list offsets, the crop mask, the shared list."""
        st = {}
        if op not in ("forward", "sample"):
            return st
        for n in LISTS + ATOM_LISTS + ("crop_keep",):
            try:
                st[n] = model.debug_buffer(n).copy()
            except DdmiError:     # (a list this model class does not build)
                st[n] = None
        try:
            st["rr0"] = model.debug_buffer("vn_off_rr0").copy()
        except DdmiError:         # not a batch of >= 2 receptor copies: the list does not exist
            st["rr0"] = None
        if self.listing is not None:
            st["routes"] = sorted(set(ln for ln in self.listing().splitlines() if ln.startswith("ddmi route")))
        return st

    def resolve_crop(self, key, a):
        """crop="median" / crop_beyond="median": the cutoff that keeps about half of the residues of the batch as it stands (for a
        loop: at the last step's 3 sigma_tr + crop_beyond, utils/sampling.py:107), from the host copy of the inputs."""
        for name in ("crop", "crop_beyond"):
            if a.get(name) == "median":
                d = torch.cat([torch.cdist(g["ligand"].pos, g["receptor"].pos).min(0).values for g in self.graphs(key)])
                cut = float(d.sort().values[len(d) // 2]) + 1e-3
                if name == "crop_beyond":
                    t = float(get_t_schedule(a.get("steps", 2))[-1])
                    cut -= 3 * self.cfg.tr_sigma_min ** (1 - t) * self.cfg.tr_sigma_max ** t
                a = dict(a, **{name: round(cut, 3)})
        return a

    # ------------------------------------------------------------------------------------------------------------ the runner
    def step(self, key, op, a=None):
        a = dict(a or {})
        expect = a.pop("expect", {})
        what = f"{self.name} step {len(self.log)} ({key}, {op}, {a})"
        self.log.append(what)
        if op == "new":                      # a new complex: its spec replaces the key's, the old batch object is dropped
            self.spec[key], self.edits[key] = a["spec"], []
            self.live.pop(key, None)
            self.live[key] = self.collate(key)
            if self.owner == key:
                self.owner = None
            return
        if op == "edit":                     # in place, on the LIVE batch object (and on every later twin)
            a["fn"](self.live[key])
            self.edits[key].append(a["fn"])
            if self.owner == key:            # (the version counters / the mask fingerprint changed: the next call sets the complex again)
                self.owner = None
            return
        if op == "poison":
            return self.poison(a["spec"])
        if op == "sidechain_raises":         # ddmi_sidechain_pred belongs to the ddmi_forward directly before it
            side = self.place(torch.empty(int(self.live[key]["receptor"].pos.shape[0]), 10))
            with pytest.raises(DdmiError):
                _l.check(self.used.lib, self.used.lib.ddmi_sidechain_pred(self.used._h, side.data_ptr(), None))
            return
        batch = self.live[key]
        a = self.resolve_crop(key, a)
        if self.listing is not None:
            self.listing()
        got = self.apply(self.used, batch, op, a)
        st_used = self.state(self.used, op)
        ck = (_freeze(self.spec[key]), tuple(e.__name__ for e in self.edits[key]), op, _freeze(a))
        if ck not in self.fresh:
            m = self.make_fresh(self.cfg, self.sd)
            if self.listing is not None:
                self.listing()
            want = self.apply(m, self.collate(key), op, a)
            self.fresh[ck] = (want, self.state(m, op))
            del m
        want, st_new = self.fresh[ck]
        assert len(got) == len(want), what
        for i, (x, y) in enumerate(zip(got, want)):
            assert bits_equal(x, y), f"{what}: output {i} of the used handle differs from a fresh handle's ({max_diff(x, y)})"
        self.check_state(key, op, a, expect, st_used, st_new, what)
        self.check_oracle(key, op, a, got, what)
        return got

    def check_state(self, key, op, a, expect, used, new, what):
        if op not in ("forward", "sample"):
            return
        if self.owner != key:                # another batch object: ddmi_set_complex ran, every list is new
            self.owner, self.shared_built = key, False
        for n in LISTS + ATOM_LISTS:
            if new[n] is None:
                assert used[n] is None, (what, n)
            else:
                assert used[n] is not None and np.array_equal(used[n], new[n]), f"{what}: {n} differs from the fresh handle's"
        assert int(new["goff_ll"][-1]) > 0, what
        if self.cfg.all_atoms:               # the static atom relations are there and hold edges
            for n in STATIC_ATOM_LISTS:
                assert used[n] is not None and int(used[n][-1]) > 0, (what, n)
        if "routes" in new:
            assert used["routes"] == new["routes"], (what, used["routes"], new["routes"])
            assert self.route_lines is None or bool(new["routes"]) == self.route_lines, (what, "route lines", new["routes"])
        cropped = bool(a.get("crop") or a.get("crop_beyond"))
        if cropped:                           # the crop did remove residues, and not all of them
            keep = used["crop_keep"]
            assert 0 < int((keep != 0).sum()) < keep.size, (what, int((keep != 0).sum()), keep.size)
            assert np.array_equal(keep != 0, new["crop_keep"] != 0), what
        B = self.live[key].num_graphs
        must = expect.get("share", self.share if self.share is None else
                          bool(self.share) and op == "sample" and not cropped and B >= 2 and expect.get("copies", True))
        ran = lambda st: st["rr0"] is not None and int(st["rr0"][-1]) > 0
        if must is None:
            assert ran(used) == ran(new) or self.shared_built, what
        elif must:
            assert ran(new) and ran(used), f"{what}: the shared rec-rec list must have run (vn_off_rr0[-1] > 0)"
            self.shared_built = True
        else:
            assert not ran(new) and (new["rr0"] is None or not new["rr0"].any()), f"{what}: the shared rec-rec list must not run"
            # The used handle builds list 9 once per complex (static_topo), so on a live batch that has shared before the offsets stay;
            # a step that shared where it must not reads graph 0's messages for every graph and fails the bit comparison above.
            if not self.shared_built:
                assert not ran(used) and (used["rr0"] is None or not used["rr0"].any()), f"{what}: shared list on the used handle"
        if "layout" in expect:                # ddmi_set_batch_layout state of the Python side: None = the uniform kernels
            assert self.used._layout == expect["layout"], (what, self.used._layout)
            assert self.used._copies == expect.get("copies", True), what

    def check_oracle(self, key, op, a, got, what):
        """The first step of every kind of operation in a script against the float64 oracle (loops: the float32 oracle loop with the
        same injected draws, at the bound of cases.config0_case)."""
        kind = (op, bool(a.get("crop") or a.get("crop_beyond")), a.get("t") == "mixed", _freeze(a.get("groups")))
        if kind in self.oracle_done or self.cfg.confidence_mode and op != "forward":
            return
        loop_with_oracle = a.get("noise", True) and a.get("groups") is None and self.spec[key]["kind"] == "copies"
        if op == "sample" and not loop_with_oracle:   # (grouped / packed loops and library draws: no oracle loop to compare with)
            return
        self.oracle_done.add(kind)
        cfg, graphs = self.cfg, self.graphs(key)
        B = len(graphs)
        if op == "forward":
            if a.get("crop"):
                graphs = [oracle_crop(copy.deepcopy(g), a["crop"]) for g in graphs]
            ob = HeteroBatch.from_data_list(graphs)
            set_times(ob, *self._times(B, a.get("t", 0.6)))
            ref = oracle_model(cfg, self.sd, dtype=F64)(ob)
            ref = ref if isinstance(ref, tuple) else (ref,)
            ref = [r for r in ref if r is not None and torch.is_tensor(r)]
            names = ("tr", "rot", "tor", "sidechain") if not cfg.confidence_mode else ("confidence", "atom_confidence")
            n = min(len(got), len(ref))
            pairs = [(g, r, nm) for g, r, nm in zip(got[:n], ref[:n], names) if r.numel()]
            assert pairs, what
            assert_scores_close([p[0] for p in pairs], [p[1].reshape(p[0].shape) for p in pairs], names=[p[2] for p in pairs], what=what)
        elif op == "sample":
            steps = a.get("steps", 2)
            s = get_t_schedule(steps)
            ocfg = cfg.replace(crop_beyond=a.get("crop_beyond"))
            ref = oracle_sampling([g.clone() for g in graphs], oracle_model(ocfg, self.sd), steps, ocfg,
                                  self._noise(self.live[key], steps, a.get("noise_seed", 4)), schedules=(s, s, s), batch_size=B,
                                  no_final_step_noise=True, **TEMP)
            ref_pos = torch.stack([x["ligand"].pos for x in ref])
            r = rmsd(got[0].reshape(B, -1, 3), ref_pos)
            assert float(r.max()) < 2e-3, (what, r)
        elif op == "perturb":
            steps, k = 5, a.get("k", 1)
            s = get_t_schedule(steps)
            tr, rot, tor = self._scores(self.live[key], 8)
            z = self._noise(self.live[key], steps, 9)
            sizes = a.get("groups") or [B]
            R = [int(g["ligand"].edge_mask.sum()) for g in graphs]
            lo = 0
            for n in sizes:                   # the guard and its eps = 0.01 nanmean|x| run per group
                t0, t1 = sum(R[:lo]), sum(R[:lo + n])
                guarded = nan_guard(tr[lo:lo + n].clone(), rot[lo:lo + n].clone(), tor[t0:t1].clone())
                ref = perturbations(cfg, k, steps, (s, s, s), guarded, (z[0][k, lo:lo + n], z[1][k, lo:lo + n], z[2][k, t0:t1]),
                                    no_final_step_noise=True, **TEMP)
                for x, y, nm in zip((got[0][lo:lo + n], got[1][lo:lo + n], got[2][t0:t1]), ref, ("tr", "rot", "tor")):
                    x, y = x.double(), y.double()
                    assert torch.equal(torch.isfinite(x), torch.isfinite(y)), (what, nm, lo)
                    fin = torch.isfinite(y)
                    assert not fin.any() or (x[fin] - y[fin]).abs().max() <= 1e-6 * y[fin].abs().max(), (what, nm, lo)
                lo += n
        elif op == "modify":
            tr, rot, tor = self._scores(self.live[key], 17, nan=False)
            a0 = t0 = 0
            for b, g in enumerate(graphs):
                n, r = g["ligand"].pos.shape[0], int(g["ligand"].edge_mask.sum())
                mr = g["ligand"].mask_rotate
                mask = torch.from_numpy(np.asarray(mr[0] if isinstance(mr, (list, tuple)) else mr).astype(bool))
                rot_edges = g["ligand", "ligand"].edge_index.T[g["ligand"].edge_mask]
                ref = oracle_modify(g["ligand"].pos.double(), 1, rot_edges, mask, tr[b:b + 1].double(), (rot * 0.7)[b:b + 1].double(),
                                    tor[t0:t0 + r].double()[None] if r else None)
                assert (got[0][a0:a0 + n].double() - ref).abs().max() < 5e-5, (what, b)
                a0, t0 = a0 + n, t0 + r

    def poison(self, spec):
        """A forward of a larger complex with NaN features on the used handle (see the module docstring).  The first pass of a script
        also runs the clean twin on a handle of its own: same edge counts, finite scores."""
        def batch_of(dirty):
            b = self.place(HeteroBatch.from_data_list(graphs_of(spec, self.cfg)))
            if dirty:     # into the COLLATED tensors: the complex's own are copied by make_pose_list before they are read
                b["ligand", "ligand"].edge_attr.fill_(1e30)
                if self.cfg.lm_embedding_type:
                    b["receptor"].x[:, 1:] = float("nan")
            return set_times(b, 0.6, 0.6, 0.6)
        out = self.used(batch_of(True))
        out = out if isinstance(out, tuple) else (out,)
        if self.cfg.confidence_mode:   # (the ReLU of the confidence predictors is an fmaxf too: NaN node rows give finite outputs)
            assert not np.isfinite(self.used.debug_buffer("x1")).all(), (self.name, "the poison did not reach the node tables")
        else:
            assert not torch.isfinite(out[0]).any(), (self.name, "the poison did not reach the scores")
        counts = {n: self.used.debug_buffer(n).copy() for n in ("offs_l", "goff_ll")}
        if not self.poison_twin:
            self.poison_twin = True
            m = self.make_fresh(self.cfg, self.sd)
            clean = m(batch_of(False))
            clean = clean if isinstance(clean, tuple) else (clean,)
            assert torch.isfinite(clean[0]).all()
            for n, v in counts.items():
                assert np.array_equal(v, m.debug_buffer(n)), (self.name, "poison changed the graph", n)
        self.owner, self.shared_built = None, False

    def run(self, script):
        for key, op, a in script:
            self.step(key, op, a)
        return self.log


# ================================================================================================================== scripts
GPU_SIZES = dict(poison=(60, 40, 4), seq=[(12, 6, 2), (25, 33, 1), (40, 20, 3), (12, 6, 2), (3, 4, 2)], live=(25, 14, 3), long=(25, 14, 3))
# reduced for the emulator (one fiber per thread: a step at ns = 48 takes tens of seconds at the sizes above)
EMU_SIZES = dict(poison=(26, 17, 3), seq=[(12, 6, 2), (16, 17, 1), (20, 10, 3), (12, 6, 2), (3, 4, 2)], live=(16, 10, 3), long=(4, 4, 2))
EMU_SIZES_ROUTES = dict(poison=(12, 8, 2), live=(8, 6, 3))     # script 2 once per route variable
EMU_SIZES_48 = dict(poison=(20, 12, 2), seq=[(10, 6, 2), (14, 9, 1), (10, 6, 2), (3, 4, 2)], live=(12, 8, 3))


def sizes_script(S, all_atoms=False, loop=True, forward_args=None):
    """Script 1: poison -> complexes of changing size (big -> small -> big -> the first again -> tiny), forward and a 2-step loop at
    each, a second poison pass in the middle."""
    sc = [(None, "poison", dict(spec=copies(90, *S["poison"], all_atoms=all_atoms)))]
    for i, (nr, nl, B) in enumerate(S["seq"]):
        first = S["seq"].index((nr, nl, B))      # a size that comes again is the same complex again
        sc.append(("c", "new", dict(spec=copies(20 + first, nr, nl, B, all_atoms=all_atoms, atoms_per_res=(2, 5) if first % 2 == 0 else (3, 4)))))
        order = ("forward", "sample") if i % 2 == 0 else ("sample", "forward")
        for op in order:
            if op == "sample" and not loop:
                continue
            sc.append(("c", op, dict(forward_args or {}) if op == "forward" else {}))
        if i == len(S["seq"]) // 2:
            sc.append((None, "poison", dict(spec=copies(91, *S["poison"], all_atoms=all_atoms))))
    return sc


def live_batch_script(S, sidechain=False):
    """Script 2: ONE live batch object, changing mode: loop (shares the layer-0 rec-rec messages) -> forward with one time per graph
    (must not share) -> loop with crop_beyond -> forward under a crop cutoff -> forward without -> loop (shares again)."""
    nr, nl, B = S["live"]
    sc = [(None, "poison", dict(spec=copies(90, *S["poison"]))),
          ("b", "new", dict(spec=copies(31, nr, nl, B))),
          ("b", "sample", {}),
          ("b", "forward", dict(t="mixed")),
          ("b", "sample", dict(crop_beyond="median")),
          ("b", "forward", {}),                  # (no set_crop_cutoff in between: the loop's own crop must be gone)
          (None, "poison", dict(spec=copies(91, *S["poison"]))),
          ("b", "sample", dict(crop_beyond="median", noise_seed=5)),
          ("b", "forward", dict(crop="median")),
          ("b", "forward", {}),
          ("b", "sample", {})]
    if sidechain:
        sc += [("b", "sidechain_raises", {}), ("b", "forward", dict(t=0.4))]
    return sc


def guard_groups_script(S):
    """Script 3: NaN-guard groups and batch layouts on one handle: copies with one group, groups [2, 1], one group again; perturb with
    NaN scores under both groupings; the conformer update; a packed batch of different ligands; copies again (the uniform kernels
    and graph 0's mask must be back in use)."""
    nr, nl, _ = S["live"]
    one, two = dict(layout=None, copies=True), dict(layout=(2, 1), copies=True)
    return [(None, "poison", dict(spec=copies(90, *S["poison"]))),
            ("a", "new", dict(spec=copies(41, nr, nl, 3))),
            ("a", "sample", dict(expect=one)),
            ("a", "sample", dict(groups=[2, 1], expect=two)),
            ("a", "perturb", dict(groups=[2, 1])),
            ("a", "sample", dict(groups=[3], expect=dict(layout=(3,), copies=True))),
            ("a", "perturb", {}),
            ("a", "modify", {}),
            (None, "poison", dict(spec=copies(91, *S["poison"]))),
            ("p", "new", dict(spec=packed())),
            ("p", "sample", dict(groups=[2, 1, 2], expect=dict(layout=(2, 1, 2), copies=False, share=False))),
            ("p", "modify", {}),
            ("p", "perturb", dict(groups=[2, 1, 2])),
            ("p", "forward", dict(expect=dict(share=False))),
            ("a", "sample", dict(expect=one)),
            ("a", "modify", {}),
            ("a", "perturb", {}),
            ("a", "new", dict(spec=copies(41, nr, nl, 3))),
            ("a", "modify", {}),
            ("a", "sample", dict(expect=one))]


def edits_script(S):
    """Script 4: in-place edits of a live batch: one graph's receptor features / positions (copies -> not copies -> copies again: the
    shared list must flip with them), the mask_rotate list, ligand.edge_mask."""
    nr, nl, B = S["live"]
    no = dict(share=False)
    return [(None, "poison", dict(spec=copies(90, *S["poison"]))),
            ("e", "new", dict(spec=copies(51, nr, nl, B))),
            ("e", "sample", {}),
            ("e", "edit", dict(fn=edit_rec_x_one)), ("e", "sample", dict(expect=no)), ("e", "forward", {}),
            ("e", "edit", dict(fn=edit_rec_x_back)), ("e", "sample", {}),
            ("e", "edit", dict(fn=edit_rec_pos_one)), ("e", "sample", dict(expect=no)),
            (None, "poison", dict(spec=copies(91, *S["poison"]))),
            ("e", "edit", dict(fn=edit_rec_pos_back)), ("e", "sample", {}), ("e", "modify", {}),
            ("e", "edit", dict(fn=edit_mask_rotate)), ("e", "modify", {}), ("e", "sample", {}),
            ("e", "edit", dict(fn=edit_edge_mask)), ("e", "forward", {}), ("e", "sample", {}), ("e", "modify", {})]


def run_script(make, place, cfg, script, name, **kw):
    return History(make, place, cfg, name=name, **kw).run(script)


# ---- configurations
def width48(layers=3, lmax=1, **kw):
    return _ddl(num_conv_layers=layers, sh_lmax=lmax, **kw)


def calm(cfg):
    """Translation noise small against the pocket (as cases.fused_node_update_case): a step moves a pose by less than an angstrom, so
    the crop of a loop's last step still cuts the receptor roughly in half instead of losing every residue."""
    return cfg.replace(tr_sigma_min=0.1, tr_sigma_max=0.5)


TINY_AA = TINY.replace(all_atoms=True, sh_lmax=2, num_conv_layers=3, dynamic_max_cross=False, cross_max_distance=60.0)


def confidence_and_score_case(make, place, S, old=False, cfg=TINY):
    """Script 6: a confidence handle and a score handle alive at once, used alternately over the sizes script."""
    if old:
        ccfg = cfg.replace(old=True, confidence_mode=True, sh_lmax=2, num_prot_emb_layers=0, depthwise_convolution=False,
                           sidechain_pred=False, reduce_pseudoscalars=False, num_confidence_outputs=1, use_old_atom_encoder=True)
    else:
        ccfg = cfg.replace(confidence_mode=True, atom_confidence=True)
    hc = History(make, place, ccfg, name=f"confidence old={old}", share=None)
    hs = History(make, place, cfg, name="score next to confidence")
    for (k1, op1, a1), (k2, op2, a2) in zip(sizes_script(S, loop=False, forward_args=dict(t=0.0)), sizes_script(S, loop=False)):
        hc.step(k1, op1, a1)
        hs.step(k2, op2, a2)
        if op2 == "forward":
            hs.step(k2, "sample", {})
    return hc.log + hs.log


def two_handles_case(make, place, S, cfg_a, cfg_b):
    """Script 7: two handles in one process, interleaved (device globals, tables, exec options of one must not reach the other)."""
    ha, hb = History(make, place, calm(cfg_a), name="handle A"), History(make, place, calm(cfg_b), sd_seed=5, name="handle B")
    nr, nl, B = S["live"]
    ha.step("x", "new", dict(spec=copies(61, nr, nl, B)))
    hb.step("y", "new", dict(spec=copies(62, nr + 3, nl + 2, 2)))
    for a in ({}, dict(t="mixed"), dict(crop="median")):
        ha.step("x", "forward", a)
        hb.step("y", "sample", {})
        hb.step("y", "forward", a)
        ha.step("x", "sample", dict(crop_beyond="median") if a.get("crop") else {})
    return ha.log + hb.log


def long_loop_case(make, place, S, cfg=TINY, steps=66):
    """Script 8: a 66-step device loop (more than STEP_TIMES_MAX = 64 steps: the times of every step are filled per step) equals the
    step-wise Python loop bit for bit; then a 20-step loop on the same live batch (the one-launch path again, same time buffer)
    equals a fresh handle's."""
    from diffdock_amd.sampling import sampling
    h = History(make, place, cfg, name="long loop")
    nr, nl, B = S["long"]
    h.step("l", "new", dict(spec=copies(71, nr, nl, B)))
    got = h.step("l", "sample", dict(steps=steps, noise=False))[0]
    s = get_t_schedule(steps)
    dev = place(torch.zeros(1)).device
    out, _ = sampling(graphs_of(h.spec["l"], cfg), h.make(cfg, h.sd), steps, s, s, s, device=dev, model_args=cfg, seed=11, batch_size=B,
                      no_final_step_noise=True, native_loop=False, **TEMP)
    stepwise = torch.cat([d["ligand"].pos.cpu() for d in out])
    assert torch.isfinite(got).all() and bits_equal(got, stepwise.reshape(got.shape)), float((got - stepwise.reshape(got.shape)).abs().max())
    h.step("l", "sample", dict(steps=20, noise=False))
    h.step("l", "forward", {})
    return h.log
