#!/usr/bin/env python3
"""Energies of the reference's labeller (gco-v3.0 swap, oracle/_ref/libgco_ref.so built by oracle/Makefile) started from
argmax_k logprob -- the start of a segmentation with a saved model -- on the seeded synthetic blocks of
tests/test_gpu_segment.py::SEGMENT_GCO_CASES, under pygco's quantisation and under the finest one gco allows.

    python tests/golden/make_golden_segment_gco.py        # after __graft_entry__.build(); a few minutes

-> tests/golden/segment_gco_energies.json.  Inputs are regenerated from the seeds (oracle/synth.py, phylo_hmrf_amd/tree.py:
pure NumPy); only the energies are stored.
"""
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# (seed, N, K, diagonal): up to config 1's 652-bin diagonal block (212,878 nodes)
CASES = [(0, 150, 10, False), (1, 160, 20, True), (5, 220, 20, True), (11, 652, 20, True)]
MIN_COVAR = 2e-3          # synth.make_block's EM-time covariances: the OU covariance + 1e-3 + 1e-3


def case_inputs(seed, N, K, diagonal):
    """the inputs of one case, exactly as the GPU test builds them: block, model Gaussians, oracle logprob, argmax start"""
    from oracle import ref_numpy as R, synth
    from phylo_hmrf_amd import synthetic
    from phylo_hmrf_amd.tree import PhyloTree
    blk = synth.make_block(seed, N, N, 4, K, diagonal)
    tree = PhyloTree(synthetic.tree_for(4))
    means, covars = tree.mean_cov(blk["params"], MIN_COVAR)
    w, eid = R.edge_weights_from_distance(blk["edges"], 0.5)
    lp = R.log_multivariate_normal_density_full(blk["X"], means, covars)
    return blk, means, covars, eid, w, lp, np.argmax(lp, axis=1)


def run(case):
    from oracle import gco_ref, ref_numpy as R
    seed, N, K, diagonal = case
    blk, _, _, eid, w, lp, init = case_inputs(*case)
    V = R.potts_matrix(K, 1.0)
    out = {"seed": seed, "N": N, "K": K, "diagonal": bool(diagonal), "n": int(lp.shape[0]),
           "e_init": float(R.mrf_energy(init, lp, eid, w, 1.0)[0]), "E": int(eid.shape[0])}
    for q in ("pygco", "fine"):
        t0 = time.time()
        lab = gco_ref.cut_general_graph(eid, w, -lp, V, n_iter=5000, algorithm="swap", init_labels=init, quant=q)
        out["e_" + q] = float(R.mrf_energy(lab, lp, eid, w, 1.0)[0])
        out["s_" + q] = round(time.time() - t0, 1)
    return out


def main():
    from oracle import gco_ref
    assert gco_ref.available(), "oracle/_ref/libgco_ref.so is missing: run __graft_entry__.build() first"
    with ProcessPoolExecutor(max_workers=min(len(CASES), 8)) as ex:
        cases = list(ex.map(run, CASES))
    for c in cases:
        print(c)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "segment_gco_energies.json")
    with open(path, "w") as f:
        json.dump({"what": "gco swap from argmax_k logprob (the reference's labeller), energies by oracle.ref_numpy.mrf_energy, "
                           "beta = 1", "cases": cases}, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
