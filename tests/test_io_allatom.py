"""diffdock_amd.io: the all-atom receptor (read_pdb_atoms, receptor_atom_features, neighbor_graph, complex_graph(all_atoms=True)) on
the reference's example complex, against tests/golden/1a0q_aa_graph.pt -- atom features, positions and relations produced by
EXECUTING the reference's new_extract_receptor_structure(all_atoms=True) and get_moad_atom_feats (tests/golden/make_1a0q_aa.py)."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from diffdock_amd.config import REC_ATOM_FEATURE_DIMS, TINY
from diffdock_amd.hetero import HeteroBatch
from diffdock_amd.io import (ATOM_ORDER, complex_graph, neighbor_graph, read_pdb_atoms, read_pdb_calpha, receptor_atom_features,
                             receptor_graph)
from diffdock_amd.model import MIScoreModel
from diffdock_amd.synth import make_pose_list
from diffdock_amd.weights import init_state_dict
from util import load_fixture, set_times, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "hipemu", "libddmi_emu.so")
REF_DATA = os.path.join(ROOT, "tests", "golden", "1a0q")      # the reference's example complex (data/1a0q), stored gzip-compressed


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("1a0q")
    for name in ("1a0q_protein_processed.pdb", "1a0q_ligand.sdf"):
        with gzip.open(os.path.join(REF_DATA, name + ".gz"), "rb") as src, open(tmp / name, "wb") as dst:
            shutil.copyfileobj(src, dst)
    return str(tmp / "1a0q_protein_processed.pdb"), str(tmp / "1a0q_ligand.sdf")


@pytest.fixture(scope="module")
def fx():
    d = load_fixture("1a0q_aa_graph")
    assert "new_extract_receptor_structure(all_atoms=True) and get_moad_atom_feats executed" in d["provenance"]
    return {k: (v.long() if torch.is_tensor(v) and v.dtype == torch.int16 else v) for k, v in d.items()}


@pytest.fixture(scope="module")
def graph(files):
    return complex_graph(*files, lm_dim=0, all_atoms=True)


def test_atom_table_follows_the_residues_of_the_calpha_reader(files, fx):
    table, names = read_pdb_atoms(files[0])
    ca = read_pdb_calpha(files[0])[0]
    assert table.shape == (416, 14, 3) and table.dtype == np.float64 and len(names) == 416
    assert np.array_equal(table[:, 1], ca)                       # column 1 is the C-alpha of the same residues
    present = ~np.isnan(table).any(-1)
    assert int(present.sum()) == 3181
    from diffdock_amd.io import _ONE_LETTER
    expected = np.asarray([len(ATOM_ORDER[_ONE_LETTER.get(n, "X")]) for n in names])
    assert not present[np.arange(14)[None] >= expected[:, None]].any()      # nothing past a residue's own atoms
    assert int((present.sum(1) < expected).sum()) == fx["n_residues_with_missing_atoms"] == 7
    # tryptophan keeps the reference's row order, which is not the file's: CE2 (row 8) before NE1 (row 10)
    assert ATOM_ORDER["W"][8:11] == ["CE2", "CE3", "NE1"]


def test_atom_features_positions_and_relation_equal_the_executed_reference(graph, fx):
    assert graph["atom"].x.shape == (3181, 4) and graph["atom"].x.dtype == torch.float32
    assert torch.equal(graph["atom"].x, fx["atom_x"].float())
    assert torch.equal(graph["atom"].pos, fx["atom_pos"])
    assert torch.equal(graph["atom", "receptor"].edge_index, fx["atom_rec_edge_index"])
    assert all(int(graph["atom"].x[:, c].max()) < d and int(graph["atom"].x[:, c].min()) >= 0 for c, d in enumerate(REC_ATOM_FEATURE_DIMS))


def test_complex_graph_all_atoms(graph, files, fx):
    assert graph["atom"].pos.shape == (3181, 3)
    ar = graph["atom", "atom_rec_contact", "receptor"].edge_index
    assert torch.equal(ar[0], torch.arange(3181)) and bool((ar[1][1:] >= ar[1][:-1]).all()) and int(ar[1].max()) == 415
    assert torch.equal(graph.original_center, fx["original_center"])
    assert torch.equal(graph["atom"].pos, fx["atom_pos_uncentred"] - graph.original_center)
    # the atom graph is the host restatement on the uncentred coordinates; the residue graph is untouched (torch.cdist path)
    aa = graph["atom", "atom_contact", "atom"].edge_index
    assert aa.dtype == torch.int64 and np.array_equal(aa.numpy(), neighbor_graph(fx["atom_pos_uncentred"].numpy(), 5.0, 8))
    plain = complex_graph(*files, lm_dim=0)
    assert "atom" not in plain.node_types
    for a, b in ((plain["receptor"].x, graph["receptor"].x), (plain["receptor"].pos, graph["receptor"].pos),
                 (plain["receptor", "receptor"].edge_index, graph["receptor", "receptor"].edge_index), (plain["ligand"].pos, graph["ligand"].pos)):
        assert torch.equal(a, b)
    assert np.array_equal(plain["receptor", "receptor"].edge_index.numpy(), receptor_graph(read_pdb_calpha(files[0])[0].astype(np.float32), 15.0, 24))


def test_host_neighbor_graph_against_the_executed_reference(fx):
    """Rows as sets: the float64 direct-difference rule and the reference's torch.cdist loop agree on every capped row of 1a0q and on
    all but a handful of uncapped ones (pairs within the recorded cdist error of the 5 A cutoff)."""
    x = fx["atom_pos_uncentred"].numpy()
    assert 1e-3 < fx["cdist_max_abs_error"] < 0.1
    for key, cap, allowed in (("atom_edge_index", 8, 0), ("atom_edge_index_uncapped", None, 4)):
        mine, ref = neighbor_graph(x, 5.0, cap), fx[key].numpy()
        cuts = lambda e: np.searchsorted(e[1], np.arange(len(x) + 1))
        rows = lambda e: [frozenset(e[0][lo:hi].tolist()) for lo, hi in zip(cuts(e)[:-1], cuts(e)[1:])]
        differing = [i for i, (a, b) in enumerate(zip(rows(mine), rows(ref))) if a != b]
        print(key, "rows differing from the executed reference:", differing)
        assert len(differing) <= allowed
        d = np.linalg.norm(x[differing][:, None].astype(np.float64) - x[None].astype(np.float64), axis=-1) if differing else np.zeros((0, 1))
        assert all((np.abs(row - 5.0) < fx["cdist_max_abs_error"]).any() for row in d)      # each has a pair at the cutoff, within the noise


def test_unknown_residue_gets_misc_features():
    table = np.full((2, 14, 3), np.nan)
    table[:, :4] = np.arange(24, dtype=np.float64).reshape(2, 4, 3)
    table[1, 4] = [1.0, 2.0, 3.0]
    feats, rel = receptor_atom_features(["XYZ", "MSE"], table)
    assert feats[:4].tolist() == [[37, 118, 22, 37]] * 4                 # the reference raises KeyError here and skips the complex
    assert feats[4:].tolist() == [[12, 6, 8, 17], [12, 5, 1, 1], [12, 5, 0, 0], [12, 7, 13, 26], [12, 5, 2, 2]]     # MSE reads as MET: N CA C O CB
    assert rel.tolist() == [list(range(9)), [0] * 4 + [1] * 5]


def test_all_atom_graph_through_the_model_on_the_emulator(graph):
    """One forward of a small all-atom score model on the graph complex_graph(all_atoms=True) built, against the float32 oracle."""
    from util import assert_scores_close, oracle_model
    r = subprocess.run(["make", "-j8", "-C", os.path.join(ROOT, "diffdock_amd", "csrc"), "emu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cfg = TINY.replace(all_atoms=True, lm_embedding_type=None, num_conv_layers=1)      # (one layer: 3597 nodes under the emulator)
    sd = init_state_dict(cfg, seed=23)
    dl = make_pose_list(graph, 1, tr_sigma_max=cfg.tr_sigma_max, seed=5, initial_noise_std_proportion=0.05)
    batch = set_times(HeteroBatch.from_data_list(dl), 0.4, 0.4, 0.4)
    m = MIScoreModel(cfg, device="cpu", lib_path=EMU)
    m.load_state_dict(sd)
    m.set_tables(*tables())
    out = m(batch)[:3]
    assert out[0].shape == (1, 3) and out[1].shape == (1, 3) and all(bool(torch.isfinite(o).all()) for o in out)
    assert_scores_close(out, oracle_model(cfg, sd)(batch)[:3], what="1a0q all-atom")
