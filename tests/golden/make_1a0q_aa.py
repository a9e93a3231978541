"""tests/golden/1a0q_aa_graph.pt: the all-atom receptor graph of the reference's example complex data/1a0q (416 residues, 3181
heavy atoms, 7 residues with missing atoms).  Data only.

    python tests/golden/make_1a0q_aa.py        (the build container: the GPU box has no /root/reference)

REFERENCE-EXECUTED (the reference's own functions, unmodified, under the stubs below):
  * datasets/process_mols.py:161-241 `new_extract_receptor_structure(..., all_atoms=True, atom_cutoff=5, atom_max_neighbors=8)` --
    atom positions, the atom neighbour graph (torch.cdist distances in float32, the 8 nearest of those within 5 A), atom features
    through `get_moad_atom_feats` (:244-276) and the atom -> residue relation -- fed with the one-letter sequence and the
    [n_res, 14, 3] coordinate table diffdock_amd.io.read_pdb_atoms parses from the stored PDB file (ProDy itself cannot run here);
  * the same call with atom_max_neighbors=None (the reference's 1000: the cap never binds): the uncapped atom graph;
  * the centring of utils/inference_utils.py:231-234 (float32 mean of the C-alpha positions).
Recorded next to them: max |torch.cdist - float64 distance| over all atom pairs, the measure of the noise in the reference's
distances that diffdock_amd's direct-difference rule does not copy (DESIGN.md "Neighbour graphs").  Edge indices are stored as
int16 (the committed-file size limit); readers widen them to int64.
The stubs: third-party modules process_mols.py imports and this path never calls are MagicMocks; rdkit's periodic table is a
five-element lookup (the only call is GetAtomicNumber on the first letter of an atom name); `get_chi_angles` (training labels) is
replaced by zeros.  tests/test_io_allatom.py and tests/neighbor_cases.py read the fixture."""
import gzip
import os
import shutil
import sys
import tempfile
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
from diffdock_amd import io as dio  # noqa: E402
from diffdock_amd.hetero import HeteroData  # noqa: E402

THREE2ONE = {'ALA': 'A', 'ARG': 'R', 'ASN': 'N', 'ASP': 'D', 'CYS': 'C', 'GLN': 'Q', 'GLU': 'E', 'GLY': 'G', 'HIS': 'H', 'ILE': 'I',
             'LEU': 'L', 'LYS': 'K', 'MET': 'M', 'MSE': 'M', 'PHE': 'F', 'PRO': 'P', 'SER': 'S', 'THR': 'T', 'TRP': 'W', 'TYR': 'Y',
             'VAL': 'V'}


def install_stubs():
    class PeriodicTable:
        numbers = {"H": 1, "C": 6, "N": 7, "O": 8, "S": 16}

        def GetAtomicNumber(self, symbol):
            return self.numbers[symbol]

    for name in ["rdkit", "rdkit.Chem", "rdkit.Chem.rdchem", "rdkit.Geometry", "rdkit.Chem.AllChem", "rdkit.Chem.rdMolTransforms",
                 "rdkit.RDLogger", "prody", "Bio", "Bio.PDB", "torch_cluster", "torch_geometric", "torch_geometric.utils",
                 "torch_geometric.data", "e3nn", "spyrmsd"]:
        sys.modules[name] = MagicMock()
    sys.modules["rdkit.Chem"].GetPeriodicTable = lambda: PeriodicTable()
    sys.path.insert(0, REF)


def main():
    install_stubs()
    import datasets.process_mols as pm
    pm.get_chi_angles = lambda coords, seq_, return_onehot=True: (np.zeros((len(seq_), 4)), None)

    with tempfile.TemporaryDirectory() as tmp:
        pdb = os.path.join(tmp, "1a0q_protein_processed.pdb")
        with gzip.open(os.path.join(HERE, "1a0q", "1a0q_protein_processed.pdb.gz"), "rb") as src, open(pdb, "wb") as dst:
            shutil.copyfileobj(src, dst)
        table, names = dio.read_pdb_atoms(pdb)
    seq = "".join(THREE2ONE.get(n, "X") for n in names)          # ProDy's pdb.ca.getSequence()
    out = {}
    for key, cap in (("", 8), ("_uncapped", None)):
        g = HeteroData()
        pm.new_extract_receptor_structure(seq, table, g, neighbor_cutoff=15.0, max_neighbors=24, lm_embeddings=None,
                                          knn_only_graph=False, all_atoms=True, atom_cutoff=5, atom_max_neighbors=cap)
        out["atom_edge_index" + key] = g["atom", "atom_contact", "atom"].edge_index.to(torch.int16)     # (3181 nodes: int16 holds them)
    center = torch.mean(g["receptor"].pos, dim=0, keepdim=True)
    out["atom_x"] = g["atom"].x
    out["atom_pos_uncentred"] = g["atom"].pos.clone()
    out["atom_pos"] = g["atom"].pos - center
    out["atom_rec_edge_index"] = g["atom", "atom_rec_contact", "receptor"].edge_index.to(torch.int16)
    out["original_center"] = center
    x = out["atom_pos_uncentred"]
    noisy = torch.cdist(x, x).double()
    worst = 0.0
    for b in range(0, len(x), 512):
        exact = (x[b:b + 512, None].double() - x[None].double()).pow(2).sum(-1).sqrt()
        worst = max(worst, float((noisy[b:b + 512] - exact).abs().max()))
    out["cdist_max_abs_error"] = worst
    out["n_residues_with_missing_atoms"] = int(sum(
        int(np.isnan(table[i, :len(dio.ATOM_ORDER[THREE2ONE.get(n, 'X')])]).any()) for i, n in enumerate(names)))
    out["provenance"] = ("atom positions / features / atom graph (5 A, 8 neighbours; and uncapped) / atom-residue relation: "
                         "datasets/process_mols.py new_extract_receptor_structure(all_atoms=True) and get_moad_atom_feats executed on "
                         "the coordinate table of diffdock_amd.io.read_pdb_atoms; centring: utils/inference_utils.py:231-234")
    path = os.path.join(HERE, "1a0q_aa_graph.pt")
    torch.save(out, path)
    print({k: (tuple(v.shape) if hasattr(v, "shape") else v) for k, v in out.items() if k != "provenance"})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
