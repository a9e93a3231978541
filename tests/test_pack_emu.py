"""The ragged step loop (ddmi_set_batch_layout, sampling.sample_complexes) on the CPU emulation build (tests/hipemu), plus the
ABI of ddmi_batch_layout.  Case bodies live in tests/pack_cases.py; tests/test_gpu_pack.py runs them on the MI355X."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import diffdock_amd.lib as L
from diffdock_amd.config import TINY
from diffdock_amd.hetero import HeteroBatch
from diffdock_amd.model import MIScoreModel
from diffdock_amd.synth import make_complex, make_pose_list
from diffdock_amd.weights import init_state_dict
from oracle.conformer import get_t_schedule
from util import tables
import pack_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "hipemu", "libddmi_emu.so")


@pytest.fixture(scope="module")
def emu_lib():
    r = subprocess.run(["make", "-j8", "-C", os.path.join(ROOT, "diffdock_amd", "csrc"), "emu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return EMU


@pytest.fixture(scope="module")
def make(emu_lib):
    def mk(cfg, sd):
        m = MIScoreModel(cfg, device="cpu", lib_path=emu_lib)
        m.load_state_dict(sd)
        m.set_tables(*tables())
        return m
    return mk


def place(x):
    return x


def test_ragged_conformer_update_matches_oracle_per_graph(make):
    P.conformer_update_case(make, place)


def test_nan_guard_runs_per_group(make):
    P.grouped_nan_guard_case(make, place)


def test_packed_complexes_equal_sampling_alone_cg(make):
    P.packed_equals_alone_case(make, place)


def test_packed_complexes_equal_sampling_alone_all_atom(make):
    P.packed_equals_alone_case(make, place, all_atoms=True)


def test_packed_step_wise_loop_equals_device_loop(make):
    """native_loop=False (model(batch), model.perturb(groups=...), model.modify_conformer_batch per step) = the device loop."""
    cfg = TINY.replace(fixed_center_conv=True, exec_options=(("tile_per_pose", 1),))
    gs = P.ragged_complexes()[1:]
    a = P.packed_run(make, place, cfg, gs, [3, 2, 4], noise=False, crop=4.0, native_loop=True)
    b = P.packed_run(make, place, cfg, gs, [3, 2, 4], noise=False, crop=4.0, native_loop=False)
    for (da, _), (db, _) in zip(a, b):
        for x, y in zip(da, db):
            assert torch.equal(x["ligand"].pos, y["ligand"].pos)


def test_packed_confidence_is_returned_per_complex(make):
    """The confidence model scores the packed batch: one row per pose, each complex's rows in its own entry, equal to
    sampling()'s confidence of that complex alone up to float32 summation order."""
    from diffdock_amd.sampling import sample_complexes, sampling
    cfg = TINY.replace(fixed_center_conv=True, exec_options=(("tile_per_pose", 1),))
    ccfg = cfg.replace(confidence_mode=True)
    m, cm = make(cfg, init_state_dict(cfg, seed=4)), make(ccfg, init_state_dict(ccfg, seed=6))
    gs = P.ragged_complexes()[1:]
    lists = [make_pose_list(c, n, tr_sigma_max=cfg.tr_sigma_max, seed=k) for k, (c, n) in enumerate(zip(gs, [3, 2, 4]))]
    s = get_t_schedule(2)
    for conf_crop in (None, 15.0):
        common = dict(seed=1, batch_size=2, confidence_model=cm, confidence_model_args=ccfg.replace(crop_beyond=conf_crop))
        packed = sample_complexes([[g.clone() for g in dl] for dl in lists], m, 2, s, s, s, max_batch_graphs=5,
                                  confidence_data_lists=[[g.clone() for g in dl] for dl in lists], **common)
        off = 0
        for k, dl in enumerate(lists):
            _, conf = sampling([g.clone() for g in dl], m, 2, s, s, s, sample_id_offset=off,
                               confidence_data_list=[g.clone() for g in dl], **common)
            assert packed[k][1].shape == conf.shape == (len(dl),)
            assert torch.allclose(packed[k][1], conf, rtol=1e-4, atol=1e-5), (k, packed[k][1], conf)
            off += len(dl)


def test_sample_complexes_packs_whole_chunks_in_order():
    from diffdock_amd.sampling import _pack
    chunks = [(0, 0, [1] * 10), (0, 10, [1] * 5), (1, 0, [1] * 10), (2, 0, [1] * 10), (3, 0, [1] * 10), (3, 10, [1] * 10)]
    packed = _pack(chunks, 40)
    assert [[(k, lo) for k, lo, _ in b] for b in packed] == [[(0, 0), (0, 10), (1, 0), (2, 0)], [(3, 0), (3, 10)]]
    assert [[(k, lo) for k, lo, _ in b] for b in _pack([(0, 0, [1] * 50), (1, 0, [1] * 3)], 40)] == [[(0, 0)], [(1, 0)]]


def test_hooks_raise(make):
    from diffdock_amd.sampling import sample_complexes
    with pytest.raises(NotImplementedError):
        sample_complexes([], None, 1, [1.0], [1.0], [1.0], visualization_list=[])


def header_fields(struct):
    header = open(os.path.join(ROOT, "include", "ddmi.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(\w+)$", decl)
        assert m, decl
        out.append((m.group(4), "ptr" if m.group(3) else m.group(2)))
    return out


def test_batch_layout_mirror_matches_the_header():
    ctype = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "ptr": ctypes.c_void_p}
    assert [(n, ctype[t]) for n, t in header_fields("ddmi_batch_layout")] == list(L.BatchLayout._fields_)
    assert ctypes.sizeof(L.BatchLayout) == 32
    assert "ddmi_set_batch_layout" in L.EXPORTED_SYMBOLS


def test_batch_layout_arguments_are_checked(make):
    sd = init_state_dict(TINY, seed=3)
    m = make(TINY, sd)
    gs = P.ragged_complexes()[:3]                    # R_b = 0, 2, 5
    batch = HeteroBatch.from_data_list(gs)
    s = get_t_schedule(2)
    m._ensure_complex(batch)                         # a batch of several complexes: the wrapper sets one group
    assert m._layout == (3,)
    nbytes = sum(int(g["ligand"].edge_mask.sum()) * g["ligand"].pos.shape[0] for g in gs)
    mask = torch.ones(nbytes, dtype=torch.uint8)

    def call(struct_size=None, ptr=(0, 1, 3), mask_t=mask, nbytes_=None):
        p = (ctypes.c_int32 * len(ptr))(*ptr)
        lay = L.BatchLayout(ctypes.sizeof(L.BatchLayout) if struct_size is None else struct_size, len(ptr) - 1,
                            ctypes.cast(p, ctypes.c_void_p), None if mask_t is None else mask_t.data_ptr(),
                            mask_t.numel() if nbytes_ is None else nbytes_)
        return m.lib.ddmi_set_batch_layout(m._h, ctypes.byref(lay), None)
    assert call() == 0
    assert call(struct_size=ctypes.sizeof(L.BatchLayout) - 8) == -1
    assert call(nbytes_=nbytes - 1) == -1
    assert call(mask_t=None, nbytes_=0) == -1
    assert call(ptr=(0, 1, 2)) == -1                 # does not span B
    assert call(ptr=(0, 2, 2, 3)) == -1              # empty group
    assert call(ptr=(1, 3)) == -1
    # ddmi_set_complex (by hand, without the layout the wrapper adds) resets the layout: a non-uniform batch returns
    # DDMI_ERR_STATE from the step loop and the conformer update until a layout is set again
    cfg = L.SampleCfg()
    sched = s.astype("float64")
    cfg.inference_steps, cfg.tr_schedule, cfg.rot_schedule, cfg.tor_schedule = 2, sched.ctypes.data, sched.ctypes.data, sched.ctypes.data
    pos = batch["ligand"].pos.clone()
    c = m._keep
    cx = L.Complex()
    cx.num_graphs, cx.n_lig, cx.n_rec = 3, batch["ligand"].pos.shape[0], batch["receptor"].pos.shape[0]
    cx.n_bond_edges, cx.n_rec_edges = batch["ligand", "ligand"].edge_index.shape[1], batch["receptor", "receptor"].edge_index.shape[1]
    cx.n_tor = int(batch["ligand"].edge_mask.sum())
    for name in ("lig_ptr", "rec_ptr", "lig_x", "bond_index", "bond_attr", "edge_mask", "rec_x", "rec_pos", "rec_edge_index"):
        setattr(cx, name, c[name].data_ptr())
    assert m.lib.ddmi_set_complex(m._h, ctypes.byref(cx), None) == 0
    assert m.lib.ddmi_sample(m._h, ctypes.c_void_p(pos.data_ptr()), ctypes.byref(cfg), None) == -2
    assert m.lib.ddmi_modify_conformer(m._h, ctypes.c_void_p(pos.data_ptr()), ctypes.c_void_p(pos.data_ptr()),
                                       ctypes.c_void_p(pos.data_ptr()), None, None) == -2
    assert call() == 0
    assert m.lib.ddmi_sample(m._h, ctypes.c_void_p(pos.data_ptr()), ctypes.byref(cfg), None) == 0


def test_different_ligands_of_equal_shape_get_their_own_masks(make):
    """Two poses of DIFFERENT ligands with equal atom and torsion counts: before the layout existed the batch passed as copies
    and every ligand was rotated with graph 0's masks.  The device loop must match each ligand sampled alone."""
    cfg = TINY.replace(fixed_center_conv=True, exec_options=(("tile_per_pose", 1),))
    gs = P.ragged_complexes()
    P.packed_run(make, place, cfg, [gs[1], gs[3]], [1, 1], noise=False, crop=None, batch_size=1, max_batch_graphs=2)
