"""Model options at the DDL-synth widths (ns = 48, nv = 10, six interaction layers), where the production kernel routes run.

The reference-executed tiny_* fixtures pin what every option means, but at ns = 8 every layer walks generic granules and
no first Linear runs inside the hidden-row kernel.  Here each option is switched on at width, on a 100-residue complex
with a 40-atom ligand (residues with two virtual nodes) and one (tr, rot, tor) time per pose, against the float64 oracle.
Every case states the route it was written for and asserts it from the library's own report (DDMI_DEBUG_GRAN: the granule
list of each layer and a `ddmi route <layer> g<group>: hidden mm|gemm|deep granules static|generic` line per edge group),
so a later change of the route rules cannot quietly turn a case into a test of another path.

`make(cfg, sd)` returns a loaded MIScoreModel, `place` moves a batch to the model's device, `setenv` sets a DDMI_* variable
before a handle is made, `listing()` returns what the library printed to stderr since the last call (capfd)."""
import math
import re

import torch

from diffdock_amd.config import DDL_SYNTH
from diffdock_amd.hetero import HeteroBatch
from diffdock_amd.synth import make_complex, make_pose_list
from diffdock_amd.weights import init_state_dict
from oracle.conformer import get_t_schedule
from util import assert_scores_close, oracle_model, set_times

F64 = torch.float64
# one time per pose and noise type; with dynamic_max_cross the cross cutoffs 3 sigma_tr + 20 are 64 / 27 / 20 A
TIMES = {"tr": (0.95, 0.6, 0.05), "rot": (0.3, 0.85, 0.6), "tor": (0.55, 0.1, 0.9)}

# Option cases: id -> (config change from DDL_SYNTH, route).  route = (hidden rows, granule loops) of every interaction layer:
#   hidden "mm":   first Linear inside the hidden-row kernel (k_edge_hidden_mm: ns % 16 == 0, ns <= 64, two-layer edge MLP)
#          "gemm": per-edge rows from GEMMs, then k_edge_hidden (ns outside that set)
#          "deep": tp_weights_layers > 2: plain first-layer rows, hidden Linear layers as GEMMs
#   granules "static":  the statically shaped loops of k_conv_fused (12-step scalar, 3-step vector chains: ns 45..48, nv 9..12,
#                       sh_lmax 1, ns % 16 == 0 ... the listing holds no `[shape 0 ` granule)
#            "generic": the compiler-scheduled / predicated variant (classic 4-slot granules)
# Every case runs k_conv_fused: depthwise layers too (their 'uvu' product is packed as the equivalent fully connected table).
OPTIONS = {
    "smooth_dyn":      (dict(smooth_edges=True), ("mm", "static")),
    "smooth_dyn_bf":   (dict(smooth_edges=True, edge_product="bf16x4"), ("mm", "static")),
    "smooth_static":   (dict(smooth_edges=True, dynamic_max_cross=False, cross_max_distance=20.0, crop_beyond=6.0), ("mm", "static")),
    "nv9":             (dict(nv=9), ("mm", "static")),
    "nv9_bf":          (dict(nv=9, edge_product="bf16x4"), ("mm", "static")),
    "ns40":            (dict(ns=40, nv=10), ("gemm", "generic")),     # ns % 16 != 0: no MFMA first layer, H = 120 not in pairs of 8-k groups
    "ns64_nv4":        (dict(ns=64, nv=4), ("mm", "generic")),        # the widest ns the first-Linear kernel takes; 16-step chains
    "tpw3":            (dict(tp_weights_layers=3), ("deep", "static")),
    "reduce_ps":       (dict(reduce_pseudoscalars=True), ("mm", "static")),
    "odd_parity":      (dict(odd_parity=True), ("mm", "static")),
    "one_group":       (dict(differentiate_convolutions=False), ("mm", "static")),
    "nobn_noscale":    (dict(batch_norm=False, scale_by_sigma=False), ("mm", "static")),
    "emb2_lig":        (dict(num_prot_emb_layers=2, embed_also_ligand=True), ("mm", "static")),
    "depthwise_l1":    (dict(depthwise_convolution=True, sh_lmax=1), ("mm", "static")),
    "depthwise_l2":    (dict(depthwise_convolution=True, sh_lmax=2), ("mm", "static")),   # (5, 9) / (3, 9) instantiations
    # second order at nv = 4 (nv = 10 is refused, below): 1-step vector chains, so every layer after the first is generic
    "second_order":    (dict(use_second_order_repr=True, sh_lmax=2, nv=4), ("mm", ("static",) + ("generic",) * 5)),
    "confidence":      (dict(confidence_mode=True), ("mm", "static")),
    "confidence_atom": (dict(confidence_mode=True, atom_confidence=True, affinity_prediction=True), ("mm", "static")),
}
# Combinations the library refuses when the model is created (DDMI_REQUIRE in weights.cpp), with the exact message.  The node
# tables have a fixed row stride of 160 floats (ddmi_common.h XS): the last irreps stage ns + 6 nv + ns (second order:
# ns + 16 nv + ns) must fit, which rules out nv 11 / 12 at ns = 48, ns = 80 at nv = 10, and second order at nv = 10.
STRIDE = "irreps wider than the node-table stride"
REFUSED = {
    "nv11":             (dict(nv=11), STRIDE),
    "nv12":             (dict(nv=12), STRIDE),
    "nv12_bf":          (dict(nv=12, edge_product="bf16x4"), STRIDE),
    "ns80":             (dict(ns=80, nv=10), STRIDE),
    "second_order_nv10": (dict(use_second_order_repr=True, sh_lmax=2), STRIDE),
    "tpw1":             (dict(tp_weights_layers=1), "tp_weights_layers must be >= 2 (FCBlock asserts it, models/layers.py:12)"),
    "emb2_nolig":       (dict(num_prot_emb_layers=2, embed_also_ligand=False),
                         "embed_also_ligand=False with embedding layers is rejected by the reference's CGModel (cg_model.py:263)"),
}


def refused_case(make, change, message):
    from diffdock_amd.lib import DdmiError
    cfg = option_config(change)
    sd = init_state_dict(cfg, seed=3)
    try:
        make(cfg, sd)
    except DdmiError as e:
        assert str(e).endswith(message), str(e)
        return
    raise AssertionError(f"{change}: the library accepted a combination it was expected to refuse ({message})")


def option_config(change, **extra):
    return DDL_SYNTH.replace(lm_embedding_type=None, **{**change, **extra})


def option_batch(cfg, n_res=100, n_lig=40, B=3, seed=5):
    g = make_complex(seed=seed, n_res=n_res, n_lig=n_lig, lm_dim=0)
    dl = make_pose_list(g, B, tr_sigma_max=5.0, seed=seed + 1, initial_noise_std_proportion=0.3)
    batch = HeteroBatch.from_data_list(dl)
    set_times(batch, *([list(TIMES[k]) * (B // 3) + list(TIMES[k][:B % 3]) for k in ("tr", "rot", "tor")]))
    return g, dl, batch


def _routes(text):
    """{layer: [(hidden, granules) per group]} from the `ddmi route` lines, {layer: granule line} from the listing."""
    routes, grans = {}, {}
    for ln in text.splitlines():
        m = re.match(r"ddmi route (\S+) g(\d+): hidden (\w+) granules (\w+)", ln)
        if m:
            routes.setdefault(m.group(1), {})[int(m.group(2))] = (m.group(3), m.group(4))
        elif ln.startswith("ddmi granules "):
            name, rest = ln[len("ddmi granules "):].split(":", 1)
            grans[name] = rest
    return routes, grans


def assert_route(cfg, text, route, what):
    """Every edge group of every interaction layer took `route` = (hidden, granules) (granules: one for all layers, or a
    tuple per layer); static granules: no `[shape 0 ` in that layer's listing."""
    routes, grans = _routes(text)
    for l in range(cfg.num_conv_layers):
        name = f"conv_layers.{l}"
        want = (route[0], route[1] if isinstance(route[1], str) else route[1][l])
        assert name in grans, (what, name, sorted(grans))
        # edge groups as run: without differentiate_convolutions they share one weight set but still run one by one
        assert name in routes and len(routes[name]) == cfg.replace(differentiate_convolutions=True).conv_groups(l), (what, name, routes.get(name))
        for gi, r in routes[name].items():
            assert r == want, (what, name, gi, r, want)
        if want[1] == "static":
            assert "[shape 0 " not in grans[name], (what, name, grans[name])
    return routes, grans


def run_option(make, place, setenv, listing, cfg, sd, batch, route, env=None):
    """One forward of a fresh handle under DDMI_DEBUG_GRAN (and `env`): outputs on the host, the route asserted."""
    setenv("DDMI_DEBUG_GRAN", "1")
    for k, v in (env or {}).items():
        setenv(k, v)
    listing()
    m = make(cfg, sd)
    m.set_kernel_timing(True)
    out = m(place(batch))
    timers = m.kernel_timings()
    m.set_kernel_timing(False)
    text = listing()
    assert "k_conv_fused" in timers, (sorted(timers), env)
    if route is not None and not (env or {}).get("DDMI_GROUPED"):   # the grouped dispatch bypasses the per-group route lines
        assert_route(cfg, text, route, env)
    return m, out, text


def compare(cfg, out, ref, what):
    """Scores against the oracle; confidence mode: the confidence rows, and the per-atom rows when atom_confidence."""
    if cfg.confidence_mode:
        assert_scores_close(out[:1], ref[:1], names=("confidence",), what=what)
        if cfg.atom_confidence:
            assert_scores_close(out[1:2], ref[1:2], names=("atom_confidence",), what=what)
        else:
            assert not out[1].any()
    else:
        assert ref[2].numel() > 0
        assert_scores_close(out[:3], ref[:3], what=what)


def smooth_edges_bite(m, cfg, batch, n_lig):
    """The cosine weights of the cross edges are far from 1 and depend on the pose's own cutoff."""
    offs = m.debug_buffer("offs_l").astype(int)
    dist = torch.from_numpy(m.debug_buffer("cross_dist")).double()[:offs[-1]]
    deg = torch.from_numpy(offs[1:] - offs[:-1])
    pose = torch.repeat_interleave(torch.arange(len(deg)) // n_lig, deg)
    if cfg.dynamic_max_cross:
        cut = torch.from_numpy(m.debug_buffer("cross_cutoff")).double()
        assert len(set(cut.tolist())) == batch.num_graphs
    else:
        cut = torch.full((batch.num_graphs,), cfg.cross_max_distance, dtype=F64)
    w = 0.5 * (torch.cos(math.pi * dist / cut[pose]) + 1)
    assert float((w < 0.9).double().mean()) > 0.1 and float(w.min()) < 0.5, ("smooth_edges: cross weights near 1", float(w.min()))
    if cfg.dynamic_max_cross:   # pose 0's cutoff would give other weights to the edges of the other poses
        w0 = 0.5 * (torch.cos(math.pi * dist / cut[0]) + 1)
        assert float((w - w0).abs().max()) > 0.1


def trajectory_case(make, place, cfg, sd, dl, steps=4, tol_pos=2e-3):
    """`steps` steps of the native device loop (ddmi_sample through diffdock_amd.sampling) against oracle.sampling fed the same
    draws, with three different schedules: the final positions, and the scores of every step on the oracle's own inputs."""
    from diffdock_amd.sampling import sampling
    from oracle.sampling import sampling as oracle_sampling
    from diffdock_amd.hetero import set_time
    from oracle.conformer import t_to_sigma
    B, R = len(dl), int(dl[0]["ligand"].edge_mask.sum())
    assert R > 0
    s = get_t_schedule(steps)
    scheds = (s, s ** 1.5, s ** 0.7)
    gen = torch.Generator().manual_seed(11)
    noise = (torch.randn(steps, B, 3, generator=gen), torch.randn(steps, B, 3, generator=gen), torch.randn(steps, B * R, generator=gen))
    record = []
    ref = oracle_sampling([d.clone() for d in dl], oracle_model(cfg, sd, dtype=F64), steps, cfg, noise, scheds, batch_size=B,
                          no_final_step_noise=True, record=record)
    ref_pos = torch.stack([d["ligand"].pos for d in ref]).double()
    m = make(cfg, sd)
    out, _ = sampling([d.clone() for d in dl], m, steps, *scheds, None, None, cfg, batch_size=B, noise=noise,
                      no_final_step_noise=True, native_loop=True)
    pos = torch.stack([d["ligand"].pos.cpu() for d in out]).double()
    assert len(record) == steps
    for r in record:   # the scores of every step, on the positions the oracle's loop reached at that step
        k = r["t_idx"]
        b = HeteroBatch.from_data_list(dl)
        b["ligand"].pos = r["pos_in"].float()
        set_time(b, scheds[0][k], scheds[1][k], scheds[2][k], B)
        if cfg.crop_beyond is not None:   # the oracle's step k ran on the graph cropped at 3 sigma_tr(t_k) + crop_beyond
            m.set_crop_cutoff(3 * float(t_to_sigma(cfg, scheds[0][k], scheds[1][k], scheds[2][k])[0]) + cfg.crop_beyond)
        assert_scores_close(m(place(b))[:3], (r["tr"], r["rot"], r["tor"]), what=f"step {k}")
    m.set_crop_cutoff(None)
    err = float((pos - ref_pos).abs().max())
    assert err < tol_pos, err
    assert float((pos - torch.stack([d["ligand"].pos for d in dl]).double()).abs().max()) > 0.1   # the poses did move
    return err


def option_inputs(name, n_res=100, n_lig=40, B=3, **extra):
    """Configuration, weights, complex, pose list, batch and float64 oracle outputs of option case `name`."""
    change, route = OPTIONS[name]
    cfg = option_config(change, **extra)
    sd = init_state_dict(cfg, seed=17)
    g, dl, batch = option_batch(cfg, n_res=n_res, n_lig=n_lig, B=B)
    ref = oracle_model(cfg, sd, dtype=F64)(batch)
    return dict(name=name, cfg=cfg, sd=sd, route=route, g=g, dl=dl, batch=batch, ref=ref, n_lig=n_lig)


def option_forward_case(make, place, setenv, listing, inp, env=None):
    """One forward of option case `inp` (option_inputs) on its claimed route, against the float64 oracle."""
    cfg = inp["cfg"]
    what = f"{inp['name']} {env or ''}"
    m, out, _ = run_option(make, place, setenv, listing, cfg, inp["sd"], inp["batch"], inp["route"], env)
    out = tuple(o.cpu() if o is not None else None for o in out)
    compare(cfg, out, inp["ref"], what)
    if cfg.smooth_edges:
        smooth_edges_bite(m, cfg, inp["batch"], inp["n_lig"])
    return out
