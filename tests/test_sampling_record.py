"""sampling() / sample_complexes(): visualization_list, return_full_trajectory and the hooks that still raise, on a stub model
whose sample_batch returns a scripted (pos, rec) -- no library, no device.  The expected visualisation calls are a plain
restatement of utils/sampling.py:193-206."""
from types import SimpleNamespace

import pytest
import torch

from diffdock_amd.hetero import HeteroData
from diffdock_amd.sampling import sample_complexes, sampling

STEPS = 3


def graph(n_lig, tag, name="cx"):
    g = HeteroData()
    g["ligand"].pos = torch.arange(n_lig * 3, dtype=torch.float32).reshape(n_lig, 3) + 1000.0 * tag
    g["ligand"].x = torch.zeros(n_lig, 1)
    g["ligand"].edge_mask = torch.zeros(0, dtype=torch.bool)
    g["receptor"].pos = torch.zeros(2, 3)
    g["receptor"].x = torch.zeros(2, 1)
    g["ligand", "lig_bond", "ligand"].edge_index = torch.zeros(2, 0, dtype=torch.long)
    g["receptor", "rec_contact", "receptor"].edge_index = torch.zeros(2, 0, dtype=torch.long)
    g.name = name
    g.original_center = torch.tensor([[0.5 + tag, -2.0, 7.0]])
    return g


class StubModel:
    """Step k adds k + 1 to the first coordinate and 0.25 to the second of every atom: the poses after step k are a known
    function of the initial ones."""
    cfg = SimpleNamespace(crop_beyond=None)

    def __init__(self):
        self.calls = []

    @staticmethod
    def step(pos, k):
        return pos + torch.tensor([k + 1.0, 0.25, 0.0])

    def sample_batch(self, data, inference_steps, schedules, record=None, groups=None, **kw):
        self.calls.append(dict(record=set(record), groups=groups, B=data.num_graphs))
        pos, rows = data["ligand"].pos.clone(), []
        for k in range(inference_steps):
            pos = self.step(pos, k)
            rows.append(pos)
        G = 1 if groups is None else len(groups)
        return pos, SimpleNamespace(pos=torch.stack(rows) if "pos" in record else None, tr=None, rot=None, tor=None,
                                    nan_count=torch.zeros(inference_steps, G, dtype=torch.int32))


class Visualisation:
    def __init__(self, log, idx):
        self.log, self.idx = log, idx

    def add(self, coords, part, order):
        assert coords.device.type == "cpu" and not coords.requires_grad
        self.log.append((self.idx, coords.clone(), part, order))


def reference_calls(init, centers, batch_size, steps):
    """utils/sampling.py:91-206 restated for the stub's dynamics: per batch, per step the poses of the batch (order t_idx + 2),
    then the whole list with order 2 -- entries of batches not yet sampled with their initial pose."""
    N, log = len(init), []
    current = [p.clone() for p in init]
    for batch_id, lo in enumerate(range(0, N, batch_size)):
        b = min(batch_size, N - lo)
        pos = [current[lo + i] for i in range(b)]
        for t_idx in range(steps):
            pos = [StubModel.step(p, t_idx) for p in pos]
            for idx_b in range(b):
                log.append((batch_id * batch_size + idx_b, pos[idx_b] + centers[batch_id * batch_size + idx_b], 1, t_idx + 2))
        for i in range(b):
            current[batch_id * batch_size + i] = pos[i]
        for idx in range(N):
            log.append((idx, current[idx] + centers[idx], 1, 2))
    return log


def assert_same_calls(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g[0], g[2], g[3]) == (w[0], w[2], w[3]), i
        assert g[1].shape == w[1].shape and torch.equal(g[1], w[1]), i


SCHED = [1.0, 0.6, 0.3]


def test_visualization_list_is_fed_call_for_call():
    dl = [graph(4, tag) for tag in range(5)]           # 5 poses, batch_size 2: three batches, the last one short
    init, centers = [g["ligand"].pos.clone() for g in dl], [g.original_center.clone() for g in dl]
    log = []
    m = StubModel()
    out, conf = sampling(dl, m, STEPS, SCHED, SCHED, SCHED, batch_size=2, visualization_list=[Visualisation(log, i) for i in range(5)])
    assert conf is None and [c["B"] for c in m.calls] == [2, 2, 1] and all(c["record"] == {"nan", "pos"} for c in m.calls)
    want = reference_calls(init, centers, 2, STEPS)
    assert len(want) == (2 + 2 + 1) * STEPS + 3 * 5
    assert_same_calls(log, want)
    assert m.calls and sampling([graph(4, 0)], StubModel(), STEPS, SCHED, SCHED, SCHED)[1] is None
    plain = StubModel()
    sampling([graph(4, 0)], plain, STEPS, SCHED, SCHED, SCHED)
    assert plain.calls[0]["record"] == {"nan"}         # without hooks only the NaN counts are recorded


def test_full_trajectory_rows():
    dl = [graph(4, tag) for tag in range(5)]
    init = torch.stack([g["ligand"].pos for g in dl])
    out, conf, traj = sampling(dl, StubModel(), STEPS, SCHED, SCHED, SCHED, batch_size=2, return_full_trajectory=True)
    assert traj.shape == (STEPS + 1, 5, 4, 3) and traj.dtype == torch.float32
    assert torch.equal(traj[0], init)                                              # row 0: the initial poses
    want = init
    for k in range(STEPS):
        want = StubModel.step(want, k)
        assert torch.equal(traj[k + 1], want)                                      # row k + 1: after step k
    assert torch.equal(traj[-1], torch.stack([g["ligand"].pos for g in out]))      # last row: the returned poses, model frame


def test_sample_complexes_slices_per_complex():
    sizes, counts = [4, 7], [3, 2]                      # unequal ligand sizes; chunks of 2: [2, 1] [2] in ONE device batch
    lists = [[graph(n, 10 * k + i, name=f"cx{k}") for i in range(c)] for k, (n, c) in enumerate(zip(sizes, counts))]
    init = [[g["ligand"].pos.clone() for g in dl] for dl in lists]
    centers = [[g.original_center.clone() for g in dl] for dl in lists]
    logs = [[], []]
    m = StubModel()
    out = sample_complexes(lists, m, STEPS, SCHED, SCHED, SCHED, batch_size=2, max_batch_graphs=8, return_full_trajectory=True,
                           visualization_list=[[Visualisation(logs[k], i) for i in range(c)] for k, c in enumerate(counts)])
    assert [c["groups"] for c in m.calls] == [[2, 1, 2]]
    for k, (dl, conf, traj) in enumerate(out):
        assert conf is None and traj.shape == (STEPS + 1, counts[k], sizes[k], 3)
        assert torch.equal(traj[0], torch.stack(init[k]))
        assert torch.equal(traj[-1], torch.stack([g["ligand"].pos for g in dl]))
        want = torch.stack(init[k])
        for s in range(STEPS):
            want = StubModel.step(want, s)
            assert torch.equal(traj[s + 1], want)
        # each complex's visualisation list receives what sampling() of that complex alone feeds it
        assert_same_calls(logs[k], reference_calls(init[k], centers[k], 2, STEPS))
    with pytest.raises(ValueError):
        sample_complexes(lists, m, STEPS, SCHED, SCHED, SCHED, visualization_list=[[]])


def test_step_wise_route_feeds_the_list_too():
    class StepModel:                                    # model(batch) / perturb / modify_conformer_batch, the stub's dynamics
        cfg = SimpleNamespace(crop_beyond=None)

        def __call__(self, batch):
            B = batch.num_graphs
            return torch.zeros(B, 3), torch.zeros(B, 3), torch.zeros(0)

        def perturb(self, batch, tr, rot, tor, t_idx, *a, **kw):
            return tr + t_idx, rot, None

        def modify_conformer_batch(self, pos, batch, trp, rotp, torp):
            return StubModel.step(pos, int(trp[0, 0]))
    dl = [graph(4, tag) for tag in range(3)]
    init, centers = [g["ligand"].pos.clone() for g in dl], [g.original_center.clone() for g in dl]
    log = []
    _, _, traj = sampling(dl, StepModel(), STEPS, SCHED, SCHED, SCHED, batch_size=2, native_loop=False, return_full_trajectory=True,
                          visualization_list=[Visualisation(log, i) for i in range(3)])
    assert_same_calls(log, reference_calls(init, centers, 2, STEPS))
    assert traj.shape == (STEPS + 1, 3, 4, 3) and torch.equal(traj[0], torch.stack(init))


def test_a_sample_batch_without_record_still_samples():
    class OldModel:                                     # sample_batch as it was before the record: returns the poses alone
        cfg = SimpleNamespace(crop_beyond=None)

        def sample_batch(self, data, inference_steps, schedules, noise=None, seed=0, sample_ids=None, ode=False, no_random=False,
                         no_final_step_noise=False, temp_sampling=1.0, temp_psi=0.0, temp_sigma_data=0.5, crop_beyond=None,
                         groups=None):
            pos = data["ligand"].pos.clone()
            for k in range(inference_steps):
                pos = StubModel.step(pos, k)
            return pos
    dl = [graph(4, tag) for tag in range(3)]
    want = torch.stack([g["ligand"].pos for g in sampling([graph(4, tag) for tag in range(3)], StubModel(), STEPS, SCHED, SCHED, SCHED)[0]])
    out, conf = sampling(dl, OldModel(), STEPS, SCHED, SCHED, SCHED, batch_size=2)
    assert conf is None and torch.equal(torch.stack([g["ligand"].pos for g in out]), want)
    (out, conf), = sample_complexes([[graph(4, tag) for tag in range(3)]], OldModel(), STEPS, SCHED, SCHED, SCHED, batch_size=2)
    assert torch.equal(torch.stack([g["ligand"].pos for g in out]), want)
    with pytest.raises(NotImplementedError):            # per-step poses need the record
        sampling(dl, OldModel(), STEPS, SCHED, SCHED, SCHED, return_full_trajectory=True)


@pytest.mark.parametrize("kw", [dict(pivot=object()), dict(return_features=True)])
def test_pivot_and_return_features_still_raise(kw):
    with pytest.raises(NotImplementedError):
        sampling([graph(4, 0)], StubModel(), STEPS, SCHED, SCHED, SCHED, **kw)
    with pytest.raises(NotImplementedError):
        sample_complexes([[graph(4, 0)]], StubModel(), STEPS, SCHED, SCHED, SCHED, **kw)
