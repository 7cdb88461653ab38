"""Seeded real-valued problems for the strip DP and the label hashes they give (tests/golden/strip_dp_labels.json).

The hashes were recorded with the library as it stood BEFORE the DP of strip.hip was reworked (one recording walk for the
fusion pass, v_writelane ballots, table chunks built by both half-waves); tests/test_gpu_strip_dp.py asserts that the
library still gives them.  A strip pass has no atomics on its label path, so the pass hashes need no deterministic mode;
the two solves run under PHMRF_DETERMINISTIC=1.

Regenerate (GPU):  python -m tests.strip_dp_cases OUT.json
"""
import hashlib
import json
import os
import sys

import numpy as np

from oracle import ref_numpy as R
from oracle import synth

# (H, W, K, diagonal, beta, seed): the shapes and betas of the record
PASS_PROBLEMS = [(64, 129, 20, False, 1.0, 21), (41, 41, 6, True, 1.0, 22), (130, 7, 5, False, 1.0, 23),
                 (200, 200, 20, True, 0.5, 24), (200, 200, 20, True, 1.0, 24), (200, 200, 20, True, 2.0, 24)]
CUTS = [(0, 0), (3, 17), (5, 63)]
SOLVE_PROBLEM = dict(seed=5, N=300, S=4, K=20, beta=1.0, perturb=0.05)


def float_problem(seed, H, W, K, diagonal):
    """unaries ~ 2 |N(0, 1)| with the true label's lowered by 1.5, weights uniform in (0.05, 1): nothing is exactly
    representable, ties do not occur"""
    rng = np.random.default_rng(seed)
    n = H * (H + 1) // 2 if diagonal else H * W
    X = rng.uniform(0.5, 2, (n, 2))
    eid = np.int64(R.grid_edges(X, H, W, diagonal, 8)[:, :2])
    w = rng.uniform(0.05, 1.0, len(eid))
    img = synth.label_image(rng, H, W, K, mean_run=6)
    truth = img[np.triu_indices(H)] if diagonal else img.reshape(-1)
    un = 2.0 * np.abs(rng.standard_normal((n, K)))
    un[np.arange(n), truth] -= 1.5
    init = rng.integers(0, K, n)
    return n, eid, w, -un, init


def pass_key(H, W, K, diagonal, beta, seed):
    return "pass %dx%d%s K=%d beta=%g seed=%d" % (H, W, " tri" if diagonal else "", K, beta, seed)


def pass_sequence_hash(H, W, K, diagonal, beta, seed):
    """SHA-1 over the labellings after every pass of: per cut and orientation the fusion pass, every label's expansion in
    one launch, and one single label's expansion"""
    from phylo_hmrf_amd import Block
    n, eid, w, lp, init = float_problem(seed, H, W, K, diagonal)
    b = Block(n, 2, K)
    b.set_graph(eid, w)
    b.set_grid(H, W, diagonal, 8)
    b.set_logprob(lp)
    b.set_labels(init)
    h = hashlib.sha1()
    moved = 0
    for i, (sr, sc) in enumerate(CUTS):
        for orient in (0, 1):
            moved += b.strip_pass(beta, orient, sr, sc, -1)
            h.update(b.get_labels().astype(np.uint8).tobytes())
            moved += b.strip_multi_pass(beta, orient, sr, sc)
            h.update(b.get_labels().astype(np.uint8).tobytes())
            moved += b.strip_pass(beta, orient, sr, sc, (2 * i + orient) % K)
            h.update(b.get_labels().astype(np.uint8).tobytes())
    b.close()
    return h.hexdigest(), moved


def solve_hashes():
    """-> (cold, warm): label hashes of a cold solve_fast and of a warm one after the model moved (the caller has set
    PHMRF_DETERMINISTIC=1: it is read when the block is created)"""
    from phylo_hmrf_amd import Block
    p = SOLVE_PROBLEM
    N, S, K = p["N"], p["S"], p["K"]
    blk = synth.make_block(seed=p["seed"], H=N, W=N, S=S, K=K, diagonal=True)
    X = blk["X"]
    w, eid = R.edge_weights_from_distance(blk["edges"], 0.5)
    b = Block(X.shape[0], S, K)
    b.set_observations(X)
    b.set_graph(eid, w)
    b.set_grid(N, N, True, 8)
    b.emission(blk["means"], blk["covars"])
    b.solve_fast(p["beta"], init_mode=1)
    cold = hashlib.sha1(b.get_labels().astype(np.uint8).tobytes()).hexdigest()
    rng = np.random.default_rng(p["seed"] + 100)
    means = blk["means"] * (1 + p["perturb"] * rng.standard_normal(blk["means"].shape))
    b.emission(means, blk["covars"])
    b.solve_fast(p["beta"])
    warm = hashlib.sha1(b.get_labels().astype(np.uint8).tobytes()).hexdigest()
    b.close()
    return cold, warm


def generate():
    out = {"generator": "python -m tests.strip_dp_cases",
           "arguments": {"pass_problems (H, W, K, diagonal, beta, seed)": PASS_PROBLEMS, "cuts": CUTS,
                         "solve_problem": SOLVE_PROBLEM},
           "hashes": {}, "moved": {}}
    for case in PASS_PROBLEMS:
        hx, moved = pass_sequence_hash(*case)
        out["hashes"][pass_key(*case)] = hx
        out["moved"][pass_key(*case)] = moved
    os.environ["PHMRF_DETERMINISTIC"] = "1"
    out["hashes"]["solve cold"], out["hashes"]["solve warm"] = solve_hashes()
    return out


if __name__ == "__main__":
    res = generate()
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["hashes"], indent=1))
