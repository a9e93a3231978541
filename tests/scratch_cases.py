"""Cases of the handle's staged uploads and grow-only scratch (PinnedStage / GrowScratch, diffdock_amd/csrc/model.h): sequences of
calls on ONE handle whose pinned staging buffers and device scratch grow, are reused at the larger size, and -- for the stagings that
belong to the complex -- are replaced with it.  Run on the CPU emulation build by tests/test_scratch_emu.py and on the MI355X by
tests/test_gpu_scratch.py through the same C ABI; `make(cfg, sd)` returns a loaded MIScoreModel, `place` moves a tensor or batch to
the model's device.

Every result of a sequence is compared with torch.equal against the same single call on a FRESH handle; nothing synchronises between
the library calls beyond what the wrappers do themselves.  The emulator does not model asynchrony: there the cases check ownership
and sizes (a buffer freed twice, or a table written past a stale capacity, breaks the host heap); the wait for the previous upload
before a staging buffer is refilled is exercised on the GPU only.

Inputs: point sets as tests/neighbor_cases.py draws them; 12-atom clouds and permutation rows (the identity first) in the manner of
tests/metrics_cases.py edge_inputs; jobs and budgets of tests/matching_cases.py; the synthetic complex of tests/randpos_cases.py."""
import numpy as np
import torch

from diffdock_amd.config import TINY
from diffdock_amd.hetero import HeteroBatch
from diffdock_amd.synth import make_complex
from diffdock_amd.weights import init_state_dict
from oracle.conformer import get_t_schedule
import matching_cases as M
import neighbor_cases as N
from metrics_cases import some_points


def fresh(make):
    return make(TINY, init_state_dict(TINY, seed=3))


def tensors_of(result):
    if torch.is_tensor(result):
        return [result]
    return [t for t in (result.values() if isinstance(result, dict) else result) if torch.is_tensor(t)]


def sequence_case(make, calls, sequence):
    """calls: {name: f(model) -> a tensor, a tuple or a dict of tensors}; sequence: the names in the order one handle runs them."""
    one = fresh(make)
    got = [calls[name](one) for name in sequence]
    want = {name: calls[name](fresh(make)) for name in dict.fromkeys(sequence)}
    for at, (name, result) in enumerate(zip(sequence, got)):
        a, b = tensors_of(result), tensors_of(want[name])
        assert len(a) == len(b) and len(a) >= 1
        for i, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape and torch.equal(x, y), (at, name, i)
    return got


# ------------------------------------------------------------------ 1. neighbour search: table 4 -> 271 words, scratch with it
def neighbor_case(make, place):
    small = N._normals(20)
    G = 90
    sizes = np.array([8] * 70 + [7] * 20)
    np.random.default_rng(5).shuffle(sizes)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    big = N._normals(700, seed=1)
    assert ptr[-1] == 700 and len(ptr) == G + 1 and 3 * G + 1 == 271
    cuts = [(4.0, 5.0, 6.5)[g % 3] for g in range(G)]
    caps = [(3, 8, None)[g % 3] for g in range(G)]
    assert not N.under_margin(small, 5.0, 8).any()
    for g in range(G):   # no decision within MARGIN of a cutoff or between kept neighbours: the comparison below is meaningful
        assert not N.under_margin(big[ptr[g]:ptr[g + 1]], cuts[g], caps[g]).any(), g
    calls = {"small": lambda m: m.neighbor_graph(place(torch.from_numpy(small)), 5.0, 8),
             "big": lambda m: m.neighbor_graph(place(torch.from_numpy(big)), cuts, caps, ptr=ptr)}
    got = sequence_case(make, calls, ["small", "big", "small"])
    assert got[0][0].shape[1] > 0 and got[1][0].shape[1] > got[0][0].shape[1]


# ------------------------------------------------------------------ 2. pose metrics and fit in one scratch
def metrics_case(make, place):
    """Scratch bytes: metrics round_up(8 P K C, 256) + 8 P K, fit 8 P K C with C = ceil(S / 64): 272 -> 576 -> (272 in 576) -> 1664."""
    rng = np.random.default_rng(23)
    cloud = lambda *s: place(torch.from_numpy((rng.normal(0.0, 2.0, size=s + (3,)) + np.array([20.0, -15.0, 30.0])).astype(np.float32)))
    perm = place(torch.from_numpy(np.stack([np.arange(12)] + [rng.permutation(12) for _ in range(129)]).astype(np.int32)))
    pos2, pos8, pos16, ref1, ref3 = cloud(2, 12), cloud(8, 12), cloud(16, 12), cloud(1, 12), cloud(3, 12)
    points = place(torch.from_numpy(some_points(9)))
    assert perm.shape == (130, 12)
    calls = {"metrics_small": lambda m: m.pose_metrics(pos2, ref1, per_ref=True),
             "fit": lambda m: m.pose_fit(pos8, ref3, perm=perm, per_ref=True),
             "metrics_big": lambda m: m.pose_metrics(pos16, ref3, perm=perm, points=points, per_ref=True)}
    sequence_case(make, calls, ["metrics_small", "fit", "metrics_small", "metrics_big"])


# ------------------------------------------------------------------ 3. matching: the table grows, a population moves into the scratch
def match(m, place, jobs, **kw):
    """matching_cases.run on a given handle."""
    lig = np.cumsum([0] + [len(j["start"]) for j in jobs])
    tor = np.cumsum([0] + [len(j["u"]) for j in jobs])
    cat = lambda key, dt: place(torch.from_numpy(np.concatenate([np.asarray(j[key]).reshape(-1) for j in jobs]).astype(dt)))
    args = dict(rot_u=cat("u", np.int32), rot_v=cat("v", np.int32), mask_rotate=cat("mask", np.uint8)) if tor[-1] else {}
    return m.match_conformer(cat("start", np.float32).reshape(-1, 3), cat("target", np.float32).reshape(-1, 3), lig, tor, **args, **kw)


def matching_case(make, place):
    job, big = M.synth_job(0, 12), M.synth_job(1, 65)
    batch = [M.synth_job(s, n) for s, n in M.BATCH]
    calls = {"one": lambda m: match(m, place, [job], popsize=4, maxiter=2, tol=0.0),
             "scratch": lambda m: match(m, place, [job, big], popsize=12, maxiter=2, tol=0.0),
             "batch": lambda m: match(m, place, batch, **M.SMALL)}
    got = sequence_case(make, calls, ["one", "scratch", "batch", "one"])
    assert got[1]["n_generations"].cpu().tolist() == [2, 2]


# ------------------------------------------------------------------ 4. the stagings that belong to the complex
def complex_stagings_case(make, place):
    """Centres and sample ids ride through stagings of the complex: back-to-back uploads, and new stagings with every ddmi_set_complex."""
    g = make_complex(seed=31, n_res=50, n_lig=16)
    R = int(g["ligand"].edge_mask.sum())
    steps = 3
    s = get_t_schedule(steps)
    gen = torch.Generator().manual_seed(12)
    one = fresh(make)
    for B in (2, 5, 2):
        batch = place(HeteroBatch.from_data_list([g.clone() for _ in range(B)]))
        centres = [torch.randn(B, 3, generator=gen) * 4.0 for _ in range(2)]
        ids = [torch.randint(0, 1 << 40, (B,), generator=gen).tolist() for _ in range(3)]
        scores = [place(torch.randn(B, 3, generator=gen)), place(torch.randn(B, 3, generator=gen)), place(torch.randn(B * R, generator=gen))]
        calls = [lambda m, k=k: m.randomize_position(batch, False, False, TINY.tr_sigma_max, center=centres[k], seed=7, sample_ids=ids[k])
                 for k in range(2)]
        calls.append(lambda m: m.perturb(batch, *scores, 1, steps, (s, s, s), seed=7, sample_ids=ids[2]))
        got = [call(one) for call in calls]
        assert not torch.equal(got[0], got[1])
        for k, call in enumerate(calls):
            want = call(fresh(make))
            for x, y in zip(tensors_of(got[k]), tensors_of(want)):
                assert torch.equal(x, y), (B, k)
