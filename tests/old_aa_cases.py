"""Cases of the legacy all-atom class (get_model(old=True) with all_atoms -> models/old_aa_model.py, AAOldModel), run on the CPU
emulation build by tests/test_old_aa_emu.py and on the MI355X by tests/test_gpu_old_aa.py through the same C ABI.
`make(cfg, sd)` returns a loaded MIScoreModel, `place` moves a batch or tensor to the model's device.

The yardstick is the reference's own class, executed by tests/golden/make_golden_old_aa.py: outputs, the node tables entering every
interaction layer and a 4-step sampling() trajectory.  Bounds are the project's: 1e-4 relative (max-norm) for forward outputs and
node tables, 2e-3 Angstrom for the trajectory."""
import copy
import ctypes

import torch

from diffdock_amd import lib as L
from diffdock_amd.hetero import HeteroBatch
from diffdock_amd.sampling import crop_beyond
from diffdock_amd.weights import init_state_dict
from util import (check_seeded_inputs, fixture_case, fixture_schedules, load_fixture, rel_err, seeded_case, set_fixture_time,
                  split_draws)

REL = 1e-4
XS = 160     # row stride of node tables and message rows (ddmi_debug_reduce_bn_sum, include/ddmi.h)
TINY_FIXTURES = ["tiny_oldaa_conf", "tiny_oldaa_conf_2l", "tiny_oldaa_conf_far", "tiny_oldaa_score", "tiny_oldaa_score_mixt"]
_cache = {}


def case_of(name):
    """(fixture, cfg, state_dict, data_list) of a fixture; loaded once, handed out as it is (nobody writes to it)."""
    if name not in _cache:
        if name == "fwd_oldaa_full":
            fx = load_fixture(name)
            cfg, sd, g, dl = seeded_case(fx["spec"])
            check_seeded_inputs(fx, sd, g)
            for d, p in zip(dl, fx["poses"]):     # the poses the reference saw (the pose generator's rounding differs between hosts)
                assert (d["ligand"].pos - p).abs().max() < 1e-4
                d["ligand"].pos = p.clone()
        else:
            fx, cfg, dl = fixture_case(name)
            sd = fx["state_dict"]
        _cache[name] = (fx, cfg, sd, dl)
    return _cache[name]


def batch_of(dl, t):
    b = HeteroBatch.from_data_list([g.clone() for g in dl])
    return set_fixture_time(b, t)


def assert_tables(m, fx, batch, report=None):
    """The x{l} debug buffers, row block by row block [lig | rec | atom], against the tables the reference's modules were fed."""
    nL, nR = batch["ligand"].pos.shape[0], batch["receptor"].pos.shape[0]
    worst = 0.0
    for l, tb in enumerate(fx["forward"]["tables"]):
        mine = torch.from_numpy(m.debug_buffer(f"x{l}"))
        for kind, base in (("lig", 0), ("rec", nL), ("atom", nL + nR)):
            if kind not in tb:     # the last layer runs the ligand modules only
                continue
            ref = tb[kind]
            rows = torch.arange(ref.shape[0]) if kind != "atom" or "atom_rows" not in fx else fx["atom_rows"]
            e = rel_err(mine[base + rows, :ref.shape[1]], ref)
            worst = max(worst, e)
            assert e < REL, (l, kind, e)
            assert not mine[base + rows, ref.shape[1]:].any(), (l, kind)     # the zero padding past the layer's irreps
    if report is not None:
        report["tables"] = worst


def fixture_parity_case(make, place, name, report=None):
    """Forward outputs, per-layer node tables and (score mode) the device loop against a reference-executed fixture."""
    fx, cfg, sd, dl = case_of(name)
    m = make(cfg, sd)
    batch = batch_of(dl, fx["t"])
    out = m(place(batch))
    ref = fx["forward"]
    report = {} if report is None else report
    for k, n in fx["edge_counts"].items():
        assert n > 0, k
    if cfg.confidence_mode:
        assert torch.is_tensor(out) and out.shape == ref["confidence"].shape     # the legacy class returns the bare tensor
        report["confidence"] = rel_err(out.cpu(), ref["confidence"])
        print(name, report)
        assert report["confidence"] < REL
        assert_tables(m, fx, batch, report)
        print(name, report)
        return m
    assert isinstance(out, tuple) and len(out) == 3
    for mine, key in zip(out, ("tr", "rot", "tor")):
        assert mine.shape == ref[key].shape
        report[key] = rel_err(mine.cpu(), ref[key])
    print(name, report)
    assert max(report[k] for k in ("tr", "rot", "tor")) < REL
    assert_tables(m, fx, batch, report)
    s = fx["sampling"]
    B, R = len(dl), int(dl[0]["ligand"].edge_mask.sum())
    pos = m.sample_batch(place(batch_of(dl, fx["t"])), s["steps"], fixture_schedules(s), noise=split_draws(s["draws"], s["steps"], B, R),
                         no_final_step_noise=True, **s["temp"])
    report["trajectory_A"] = float((pos.cpu().reshape(B, -1, 3) - s["final_pos"]).abs().max())
    print(name, report)
    assert report["trajectory_A"] < 2e-3
    return m


def far_pose_case(make, place):
    """tiny_oldaa_conf_far: the last pose has no receptor atom within lig_max_radius, so its ligand rows take BatchNorm(0) of the
    lig<-atom module (not 0) and its atoms no message from the ligand; the fixture parity holds, and the device graph agrees."""
    fx, cfg, sd, dl = case_of("tiny_oldaa_conf_far")
    m = fixture_parity_case(make, place, "tiny_oldaa_conf_far")
    offs = m.debug_buffer("offs_la_l")
    n = dl[0]["ligand"].pos.shape[0]
    assert offs[-1] == fx["edge_counts"][2] and offs[-1] == offs[-1 - n] > 0     # no lig<-atom edge in the last graph, some before it


def single_pose_case(make, place):
    """A batch of one pose: the confidence of a pose does not depend on its batch (eval-mode BatchNorm, per-graph mean)."""
    fx, cfg, sd, dl = case_of("tiny_oldaa_conf")
    m = make(cfg, sd)
    for b in (0, 2):
        out = m(place(batch_of(dl[b:b + 1], fx["t"])))
        assert out.shape == (1,)
        assert rel_err(out.cpu(), fx["forward"]["confidence"][b:b + 1]) < REL, b


def crop_case(make, place, name="tiny_oldaa_conf"):
    """ddmi_set_crop_cutoff on the full graphs against the same model on graphs cropped on the host by crop_beyond(all_atoms=True):
    a cutoff that keeps about half of the residues of pose 0."""
    fx, cfg, sd, dl = case_of(name)
    d = torch.cdist(dl[0]["ligand"].pos, dl[0]["receptor"].pos).min(0).values
    cutoff = float(d.sort().values[len(d) // 2]) + 1e-3
    cropped = [crop_beyond(copy.deepcopy(g), cutoff, all_atoms=True) for g in dl]
    n_kept, n_all = sum(g["receptor"].pos.shape[0] for g in cropped), sum(g["receptor"].pos.shape[0] for g in dl)
    assert 0 < n_kept < n_all and all(g["receptor"].pos.shape[0] > 0 for g in cropped)
    m = make(cfg, sd)
    want = m(place(batch_of(cropped, fx["t"])))
    want = [w.cpu() for w in (want if isinstance(want, tuple) else (want,))]
    m.set_crop_cutoff(cutoff)
    try:
        got = m(place(batch_of(dl, fx["t"])))
    finally:
        m.set_crop_cutoff(None)
    got = [g.cpu() for g in (got if isinstance(got, tuple) else (got,))]
    keep = m.debug_buffer("crop_keep")
    assert 0 < int((keep != 0).sum()) == n_kept < keep.size
    for a, b in zip(got, want):
        e = rel_err(a, b)
        print(name, "crop", e)
        assert e < REL
    full = m(place(batch_of(dl, fx["t"])))      # the crop really changed the result, and the handle drops it again
    full = [f.cpu() for f in (full if isinstance(full, tuple) else (full,))]
    assert rel_err(full[0], want[0]) > 10 * REL
    ref = fx["forward"]["confidence"] if cfg.confidence_mode else fx["forward"]["tr"]
    assert rel_err(full[0], ref) < REL


def reused_handle_case(make, place):
    """One handle evaluating two different complexes in a row equals two fresh handles, bit for bit."""
    fx, cfg, sd, dl = case_of("tiny_oldaa_conf")
    fx2, cfg2, _, dl2 = case_of("tiny_oldaa_conf_far")
    assert cfg == cfg2
    b1, b2 = batch_of(dl, fx["t"]), batch_of(dl2[1:], 0.2)      # other poses, another batch size, another time
    m = make(cfg, sd)
    first, second = m(place(b1)).cpu(), m(place(b2)).cpu()
    assert torch.equal(first, make(cfg, sd)(place(b1)).cpu())
    assert torch.equal(second, make(cfg, sd)(place(b2)).cpu())
    assert not torch.equal(first[1:], second)


def sampling_confidence_case(make, place):
    """sampling(..., confidence_model=<AAOldModel>, confidence_data_list=<all-atom graphs>) behind a CG score model ("Confidence model
    uses different type of graphs than the score model", inference.py:183-195): the confidences it returns are the model's own on the
    all-atom graphs at the final poses, t = 0."""
    from diffdock_amd.config import TINY
    from diffdock_amd.sampling import sampling
    from oracle.conformer import get_t_schedule
    fx, cfg_c, sd_c, dl = case_of("tiny_oldaa_conf")
    cfg_s = TINY.replace(tr_sigma_max=2.0)      # CG score model on the same complex (it ignores the atom arrays)
    score, conf_m = make(cfg_s, init_state_dict(cfg_s, seed=3)), make(cfg_c, sd_c)
    dev = place(torch.zeros(1)).device
    s = get_t_schedule(2)
    out_list, conf = sampling([g.clone() for g in dl], score, 2, s, s, s, device=dev, model_args=cfg_s, confidence_model=conf_m,
                              confidence_data_list=[g.clone() for g in dl], confidence_model_args=cfg_c, batch_size=len(dl), seed=4,
                              no_final_step_noise=True)
    final = [g.clone() for g in dl]
    for g, o in zip(final, out_list):
        g["ligand"].pos = o["ligand"].pos.detach().cpu()
        assert not torch.equal(g["ligand"].pos, dl[0]["ligand"].pos) and torch.isfinite(g["ligand"].pos).all()
    want = conf_m(place(batch_of(final, 0.0)))
    assert conf.shape == (len(dl),) and torch.equal(conf.cpu(), want.cpu())


def stepwise_loop_case(make, place, name="tiny_oldaa_score"):
    """The step-wise python loop (model(batch) + ddmi_perturb + ddmi_modify_conformer per step) of the score-mode class reaches the
    reference trajectory's final poses as the device loop does."""
    from diffdock_amd.sampling import sampling
    fx, cfg, sd, dl = case_of(name)
    s = fx["sampling"]
    B, R = len(dl), int(dl[0]["ligand"].edge_mask.sum())
    m = make(cfg, sd)
    dev = place(torch.zeros(1)).device
    out_list, _ = sampling([g.clone() for g in dl], m, s["steps"], *fixture_schedules(s), device=dev, model_args=cfg, batch_size=B,
                           noise=split_draws(s["draws"], s["steps"], B, R), no_final_step_noise=True, native_loop=False)
    pos = torch.stack([o["ligand"].pos.detach().cpu() for o in out_list])
    e = float((pos - s["final_pos"]).abs().max())
    print(name, "step-wise loop", e)
    assert e < 2e-3


# --------------------------------------------------------------------------------------------------------- k_reduce_bn_sum
def _reduce_inputs(n_groups, n_nodes, d_in, d_out, seed, max_deg=41):
    """Random message rows in target order: per group and node 0 .. max_deg rows (some nodes without any, some past the 16-row
    unrolled loop of the kernel), a folded BatchNorm per group."""
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, max_deg, (n_groups, n_nodes), generator=g)
    deg[:, 0] = 0
    deg[0, 1] = 0
    deg[-1, 2] = max_deg + 23
    toff = torch.zeros(n_groups, n_nodes + 1, dtype=torch.int32)
    total = 0
    for k in range(n_groups):      # the groups own disjoint row ranges of one message buffer
        toff[k] = total + torch.cat([torch.zeros(1, dtype=torch.long), deg[k].cumsum(0)]).int()
        total = int(toff[k, -1])
    msg = torch.randn(total, XS, generator=g)
    bn = [torch.randn(n_groups, d_out, generator=g) * s + o for s, o in ((0.3, 0.0), (0.4, 1.0), (0.2, 0.0))]
    x_in = torch.randn(n_nodes, XS, generator=g)
    return toff, msg, bn, x_in


def _run_reduce(lib, place, stream, toff, msg, bn, x_in, d_in, d_out, ref):
    n_groups, n_nodes = toff.shape[0], toff.shape[1] - 1
    dev = [place(t.contiguous()) for t in (toff, msg, bn[0], bn[1], bn[2], x_in)]
    out = place(torch.full((n_nodes, XS), float("nan")))
    ref_out = place(torch.full((n_nodes, XS), float("nan"))) if ref else None
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    L.check(lib, lib.ddmi_debug_reduce_bn_sum(n_groups, n_nodes, d_in, d_out, *[p(t) for t in dev], p(out), p(ref_out), stream))
    if out.is_cuda:
        torch.cuda.synchronize()
    return out.cpu(), None if ref_out is None else ref_out.cpu()


def reduce_one_group_case(lib, place, stream=None):
    """One group through k_reduce_bn_sum equals k_reduce_bn (with the residual) bit for bit: same rows per wave, same order."""
    for d_in, d_out, seed in ((8, 17, 1), (34, 34, 2), (60, 84, 3), (160, 160, 4)):
        toff, msg, bn, x_in = _reduce_inputs(1, 37, d_in, d_out, seed)
        out, ref = _run_reduce(lib, place, stream, toff, msg, bn, x_in, d_in, d_out, True)
        assert torch.isfinite(out).all() and torch.equal(out, ref), (d_in, d_out)
        assert not out[:, d_out:].any()


def reduce_three_groups_case(lib, place, stream=None):
    """x + sum_g BN_g(mean_g), a node without rows in a group contributing BN_g(0): against float64 torch.  Bound: a float32 sum of
    at most 64 rows and three terms, 2^-24 * (64 + 8) relative to the largest partial sum < 1e-5 of the output's magnitude."""
    d_in, d_out = 17, 34
    toff, msg, bn, x_in = _reduce_inputs(3, 29, d_in, d_out, 7)
    out, _ = _run_reduce(lib, place, stream, toff, msg, bn, x_in, d_in, d_out, False)
    want = torch.zeros(29, XS, dtype=torch.float64)
    want[:, :d_in] = x_in[:, :d_in].double()
    for k in range(3):
        for i in range(29):
            rows = msg[int(toff[k, i]):int(toff[k, i + 1]), :d_out].double()
            mean = rows.mean(0) if rows.shape[0] else torch.zeros(d_out, dtype=torch.float64)
            want[i, :d_out] += (mean - bn[0][k].double()) * bn[1][k].double() + bn[2][k].double()
    assert int(toff[0, 1]) == int(toff[0, 2]) and int(toff[1, 0]) == int(toff[1, 1])      # empty (node, group) pairs are in the data
    assert rel_err(out, want) < 1e-5
    assert not out[:, d_out:].any()


# ------------------------------------------------------------------------------------------------------------- factory
def factory_case(lib_path, device):
    """get_model(args, old=True) with all_atoms builds the class in both modes, with the reference module's key counts at two layers with language-model
    columns (214 / 235: the module's state_dict has 216 / 235 entries, two of them the num_batches_tracked counters of the confidence
    head's BatchNorm1d, which are not weights; make_golden_old_aa.py asserts the key sets equal); parallel > 1 and the new AtomEncoder stay refused."""
    import pytest
    from diffdock_amd.config import TINY
    from diffdock_amd.model import MIScoreModel, get_model
    from diffdock_amd.weights import state_dict_spec
    base = TINY.replace(all_atoms=True, num_conv_layers=2, num_confidence_outputs=3)
    for conf, n_keys in ((True, 214), (False, 235)):
        m = get_model(base.to_namespace(), device, confidence_mode=conf, old=True, lib_path=lib_path)
        assert isinstance(m, MIScoreModel) and m.cfg.old and m.cfg.all_atoms and m.cfg.sh_lmax == 2 and m.cfg.confidence_mode == conf
        assert m.cfg.num_confidence_outputs == 3 and m.cfg.rec_max_radius == 30.0 and m.cfg.center_max_distance == 30.0
        spec = state_dict_spec(m.cfg)
        assert len(spec) == n_keys
        assert m.expected_keys() == {k: tuple(v[0]) for k, v in spec.items()}
        sd = init_state_dict(m.cfg, seed=1)
        m.load_state_dict(sd)
        sd.pop("conv_layers.17.fc.0.weight")      # a module the forward never runs is a key all the same
        with pytest.raises(RuntimeError):
            m.load_state_dict(sd)
    args = base.to_namespace()
    args.parallel = 2
    with pytest.raises(NotImplementedError, match="parallel"):
        get_model(args, device, confidence_mode=True, old=True, lib_path=lib_path)
    args = base.to_namespace()
    args.use_old_atom_encoder = False
    with pytest.raises(NotImplementedError, match="AtomEncoder"):
        get_model(args, device, confidence_mode=True, old=True, lib_path=lib_path)
