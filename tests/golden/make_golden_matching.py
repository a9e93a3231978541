"""Writes tests/golden/conformer_matching.pt: the jobs of the quality cases of tests/matching_cases.py (start, target, torsion tables)
and the rmsd that the host route (diffdock_amd.matching.match_conformers_host: scipy.optimize.differential_evolution called as the
reference's optimize_rotatable_bonds calls it) reaches at popsize 40 and maxiter 40, with the scipy version recorded.

    python tests/golden/make_golden_matching.py
"""
import os
import sys

import scipy
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from diffdock_amd.matching import match_conformers_host   # noqa: E402
from matching_cases import synth_job                      # noqa: E402

#        (seed, n): R = 7, 5, 7 at n = 30; 7, 8 at n = 20; 11 for seed 0 at n = 30
JOBS = ((1, 30), (2, 30), (3, 30), (4, 20), (7, 20), (0, 30))


def main():
    jobs = []
    for seed, n in JOBS:
        j = synth_job(seed, n)
        res = match_conformers_host([((j["u"], j["v"], j["mask"]), j["start"], j["target"])], popsize=40, maxiter=40, seed=0)[0]
        print(f"seed {seed} n {n} R {len(j['u'])}: host rmsd {res['rmsd']:.6f} after {res['evaluations']} evaluations")
        jobs.append(dict(name=f"synth_{seed}_{n}", start=torch.from_numpy(j["start"]), target=torch.from_numpy(j["target"]),
                         rot_u=torch.from_numpy(j["u"]), rot_v=torch.from_numpy(j["v"]), mask=torch.from_numpy(j["mask"]),
                         host_rmsd=res["rmsd"], host_evaluations=res["evaluations"]))
    torch.save(dict(jobs=jobs, popsize=40, maxiter=40, scipy=scipy.__version__), os.path.join(HERE, "conformer_matching.pt"))


if __name__ == "__main__":
    main()
