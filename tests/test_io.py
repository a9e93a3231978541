"""diffdock_amd.io: PDB / SDF readers and graph construction on the reference's example complex."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cases
from diffdock_amd.config import TINY
from diffdock_amd.io import complex_graph, ligand_bond_arrays, read_sdf, receptor_graph, transformation_mask
from diffdock_amd.model import MIScoreModel
from diffdock_amd.synth import make_complex, receptor_contact_graph
from util import load_fixture, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "hipemu", "libddmi_emu.so")
REF_DATA = os.path.join(ROOT, "tests", "golden", "1a0q")      # the reference's example complex (data/1a0q), stored gzip-compressed


def test_fixture_has_the_documented_sizes():
    d = load_fixture("1a0q_graph")
    assert d["rec_pos"].shape == (416, 3) and d["lig_pos"].shape == (23, 3)        # 416 residues, 23 heavy atoms
    assert d["bond_index"].shape[1] == 46 and d["bond_attr"].sum(1).eq(1).all()
    assert abs(float(d["rec_pos"].mean())) < 1e-4                                   # centred on the C-alpha centroid
    deg = torch.bincount(d["rec_edge_index"][1], minlength=416)
    assert int(deg.max()) == 24 and int(deg.min()) >= 1                             # 24 nearest within 15 A
    src, dst = d["rec_edge_index"]
    assert float((d["rec_pos"][src] - d["rec_pos"][dst]).norm(dim=1).max()) < 15.0
    assert int(d["edge_mask"].sum()) == d["mask_rotate"].shape[0]


def ref_data(tmp_path):
    """the stored data/1a0q files, decompressed into tmp_path (the readers take plain file paths)"""
    for name in ("1a0q_protein_processed.pdb", "1a0q_ligand.sdf"):
        with gzip.open(os.path.join(REF_DATA, name + ".gz"), "rb") as src, open(tmp_path / name, "wb") as dst:
            shutil.copyfileobj(src, dst)
    return str(tmp_path)


def test_io_reproduces_the_reference_executed_fixture_bit_for_bit(tmp_path):
    """diffdock_amd.io against the fixture whose receptor graph / features / positions and rotatable-bond masks were produced
    by EXECUTING the reference (datasets/process_mols.py new_extract_receptor_structure, utils/torsion.py
    get_transformation_mask, the centring of datasets/pdbbind.py; tests/golden/make_1a0q.py)."""
    data = ref_data(tmp_path)
    g = complex_graph(f"{data}/1a0q_protein_processed.pdb", f"{data}/1a0q_ligand.sdf", lm_dim=0)
    d = load_fixture("1a0q_graph")
    assert "process_mols.py new_extract_receptor_structure executed" in d["provenance"]
    assert torch.equal(g["receptor"].pos, d["rec_pos"]) and torch.equal(g["receptor", "receptor"].edge_index, d["rec_edge_index"])
    assert torch.equal(g["receptor"].x, d["rec_x"]) and torch.equal(g.original_center, d["original_center"])
    assert torch.equal(g["ligand"].pos, d["lig_pos"]) and torch.equal(g["ligand", "ligand"].edge_index, d["bond_index"])
    assert torch.equal(g["ligand"].edge_mask, d["edge_mask"])
    assert np.array_equal(np.asarray(g["ligand"].mask_rotate[0]), d["mask_rotate"].numpy())
    xyz, z, bonds = read_sdf(f"{data}/1a0q_ligand.sdf", remove_hs=False)
    assert len(z) == 45 and int((z == 1).sum()) == 22 and len(bonds) == 45


def test_graph_builders_agree_with_the_synthetic_generators():
    """The networkx restatement of get_transformation_mask and the receptor graph against the independent implementations
    in diffdock_amd.synth (which the reference-executed fixtures were generated with)."""
    for seed in range(5):
        c = make_complex(seed=seed, n_res=40, n_lig=22 + seed)
        ei = c["ligand", "ligand"].edge_index.numpy()
        me, mr = transformation_mask(22 + seed, ei)
        assert np.array_equal(me, c["ligand"].edge_mask.numpy()) and np.array_equal(mr, c["ligand"].mask_rotate[0])
        rc = c["receptor"].pos.numpy()
        a, b = receptor_graph(rc, 15.0, 24), receptor_contact_graph(rc, 15.0, 24)   # torch.cdist float32 vs the generator's distances
        assert a.shape == b.shape and np.array_equal(a[1], b[1])
        sets = lambda e: [frozenset(e[0][e[1] == i]) for i in range(len(rc))]     # order inside exact ties (3.8 A chain steps) is free
        assert sum(x != y for x, y in zip(sets(a), sets(b))) <= 1
    ei, attr = ligand_bond_arrays([(0, 1, 1), (1, 2, 2), (2, 3, 4)])
    assert ei.tolist() == [[0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2]] and attr.argmax(1).tolist() == [0, 0, 1, 1, 3, 3]


def test_configs0_plumbing_on_the_cpu_emulation():
    """BASELINE configs[0] geometry (data/1a0q, 2 samples) with the small preset through the emulated kernels, 2 steps."""
    r = subprocess.run(["make", "-j8", "-C", os.path.join(ROOT, "diffdock_amd", "csrc"), "emu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def make(cfg, sd):
        m = MIScoreModel(cfg, device="cpu", lib_path=EMU)
        m.load_state_dict(sd)
        m.set_tables(*tables())
        return m
    cases.config0_case(make, lambda b: b, TINY.replace(lm_embedding_type=None, num_conv_layers=3), steps=2)   # (4 steps, full width: -m gpu)


_PHENOLATE = """phenolate
  hand-written

 12 12  0  0  0  0  0  0  0  0999 V2000
    0.0000    1.4000    0.0000 C   0  0  0  0  0  0
    1.2124    0.7000    0.0000 C   0  0  0  0  0  0
    1.2124   -0.7000    0.0000 C   0  0  0  0  0  0
    0.0000   -1.4000    0.0000 C   0  0  0  0  0  0
   -1.2124   -0.7000    0.0000 C   0  0  0  0  0  0
   -1.2124    0.7000    0.0000 C   0  0  0  0  0  0
    0.0000    2.7600    0.0000 O   0  5  0  0  0  0
    2.1500    1.2400    0.0000 H   0  0  0  0  0  0
    2.1500   -1.2400    0.0000 H   0  0  0  0  0  0
    0.0000   -2.4800    0.0000 H   0  0  0  0  0  0
   -2.1500   -1.2400    0.0000 H   0  0  0  0  0  0
   -2.1500    1.2400    0.0000 H   0  0  0  0  0  0
  1  2  4  0
  2  3  4  0
  3  4  4  0
  4  5  4  0
  5  6  4  0
  6  1  4  0
  1  7  1  0
  2  8  1  0
  3  9  1  0
  4 10  1  0
  5 11  1  0
  6 12  1  0
M  END
$$$$
"""

_SPIRO = """spiro[2.3]hexane with an ammonium substituent, charges on M  CHG
  hand-written

  7  8  0  0  0  0  0  0  0  0999 V2000
    0.0000    0.0000    0.0000 C   0  0  0  0  0  0
    1.0000    1.0000    0.0000 C   0  0  0  0  0  0
    1.0000   -1.0000    0.0000 C   0  0  0  0  0  0
   -1.0000    1.0000    0.5000 C   0  0  0  0  0  0
   -2.0000    0.0000    0.0000 C   0  0  0  0  0  0
   -1.0000   -1.0000   -0.5000 C   0  0  0  0  0  0
   -3.4000    0.0000    0.0000 N   0  3  0  0  0  0
  1  2  1  0
  2  3  1  0
  3  1  1  0
  1  4  1  0
  4  5  1  0
  5  6  1  0
  6  1  1  0
  5  7  1  0
M  CHG  1   7   1
M  END
$$$$
"""


def test_ligand_atom_features_from_the_connection_table(tmp_path):
    """The columns of lig_atom_featurizer (datasets/process_mols.py:97-120) that need no chemistry perception, on two
    hand-written molecules whose values follow from the file: phenolate (aromatic bond type 4, explicit hydrogens, charge code)
    and a spiro ring system (two rings of sizes 3 and 4 through one atom, `M  CHG`).  Chirality / implicit valence /
    hybridisation (columns 1, 4, 7) stay 0 = declared external."""
    from diffdock_amd.io import ligand_atom_features
    p = tmp_path / "phenolate.sdf"
    p.write_text(_PHENOLATE)
    f = ligand_atom_features(str(p))
    assert f.shape == (7, 16)
    assert f[:, 0].tolist() == [5] * 6 + [7]                    # C, O: atomic number - 1
    assert f[:, 2].tolist() == [3] * 6 + [1]                    # total degree: ring carbons 3 (2 C + H or O), O 1
    assert f[:, 3].tolist() == [5] * 6 + [4]                    # formal charge index: 0 -> 5, -1 -> 4
    assert f[:, 5].tolist() == [0, 1, 1, 1, 1, 1, 0]            # hydrogens written in the file
    assert f[:, 8].tolist() == [1] * 6 + [0]                    # aromatic: a bond of type 4
    assert f[:, 9].tolist() == [1] * 6 + [0]                    # one ring through every carbon
    assert f[:, 13].tolist() == [1] * 6 + [0] and not f[:, [10, 11, 12, 14, 15]].any()     # ring of size 6 only
    assert not f[:, [1, 4, 6, 7]].any()
    g = complex_graph_lig_only(str(p))
    assert np.array_equal(g, f)
    q = tmp_path / "spiro.sdf"
    q.write_text(_SPIRO)
    f = ligand_atom_features(str(q))
    assert f[:, 9].tolist() == [2, 1, 1, 1, 1, 1, 0]            # the spiro atom is in both rings
    assert f[:, 10].tolist() == [1, 1, 1, 0, 0, 0, 0] and f[:, 11].tolist() == [1, 0, 0, 1, 1, 1, 0]   # sizes 3 and 4
    assert f[:, 3].tolist() == [5] * 6 + [6]                    # M  CHG: N +1 (and it supersedes the atom-block code 3 = +1)
    assert f[:, 2].tolist() == [4, 2, 2, 2, 3, 2, 1]            # no hydrogens in the file: heavy neighbours only (documented)


def complex_graph_lig_only(sdf):
    """ligand rows of complex_graph's default atom features = ligand_atom_features (receptor side from the synthetic PDB-free path
    is not needed: the function is called directly)."""
    from diffdock_amd.io import ligand_atom_features, read_sdf
    _, z, _ = read_sdf(sdf)
    f = ligand_atom_features(sdf)
    assert f.shape[0] == len(z)
    return f
