"""Ancestral contact maps from a fitted model: E[z_ancestor | observed species, state] per bin pair, with its uncertainty.

Every state of the model is an Ornstein-Uhlenbeck process on the species tree, so it holds a joint Gaussian over ALL tree
nodes (tree.PhyloTree.joint_moments), the internal ones included.  Conditioning the internal nodes on the leaves, with
min_covar as the observation noise of the emission, gives per state k an affine map of the observed vector x and a
conditional variance (tree.PhyloTree.ancestral_tables):

    mu_k(x) = c_k + G_k x,   G_k = C_AL (C_LL + min_covar I)^-1,   v_k = diag(C_AA - G_k C_LA)

`reconstruct(model, weighting, want_sd)` mixes them per bin pair on the GPU (phmrf_ancestral, include/phmrf.h):
  "posterior"  with the conditional posterior p_ik given the neighbours' labels -- the posterior `conf` is taken from:
               mean = sum_k p_ik mu_k(x_i),  sd^2 = sum_k p_ik v_k + sum_k p_ik (mu_k(x_i) - mean)^2
  "called"     the called state's own map: mean = mu_{l_i}(x_i), sd^2 = v_{l_i}
on the labels the device holds: after segment(), or after the last E-step of a fit.  Per region the emission is run
first under the model's current means_ / _covars_ (after a fit the device's log-likelihoods belong to older parameters);
the tables come from the OU parameters that gave those Gaussians, the ones save_model writes.  Whole blocks run on the
model's block runner, row tiles of split blocks tile by tile from the conductor's groups; with several ranks every output
position is written by one rank and the planes are gathered with the byte all-reduce, as conf is.

The values are in the model's feature units -- the loader's normalised, log-scaled contact values -- not raw counts.
"""
import time

import numpy as np

from ._lib import PhmrfError

WEIGHTINGS = ("posterior", "called")
NPZ_KEYS = ("nodes", "parent", "species", "mean", "sd", "len_vec", "weighting")


def model_tables(model):
    """-> (affine [K, A, S+1], cond_var [K, A]) from the OU parameters behind the model's Gaussians (save_model's source)"""
    params = np.asarray(getattr(model, "params_vec", model.params_vec1), dtype=np.float64)
    return model.tree.ancestral_tables(params, float(model.min_covar))


def reconstruct(model, weighting="posterior", want_sd=True):
    """-> dict(nodes int64 [A] the tree's internal nodes, parent int64 [N] of every tree node (-1: the root),
    mean float32 [A, n] in global order, sd float32 [A, n] or None, timing {stage: ms summed over this rank's regions})"""
    if weighting not in WEIGHTINGS:
        raise ValueError("weighting must be one of %s, not %r" % (", ".join(WEIGHTINGS), weighting))
    n = int(model.n_samples)
    beta, et = float(model.beta), int(model.estimate_type)
    means, covars = model.means_, model._covars_
    affine, cond_var = model_tables(model)
    A = affine.shape[1]
    mean = np.zeros((A, n), dtype=np.float32)
    sd = np.zeros((A, n), dtype=np.float32) if want_sd else None
    timing = dict(emission=0.0, ancestral=0.0)

    def run(b, out, own_local):
        t0 = time.perf_counter()
        b.emission(means, covars)
        b.sync()
        t1 = time.perf_counter()
        try:
            mu, s = b.ancestral(beta, et, affine, cond_var, weighting, want_sd)
        except PhmrfError as e:
            if e.status != 5:
                raise
            raise RuntimeError("no labels on the device: run segment() or a fit before ancestral() (%s)" % e)
        lo = own_local.start - b.owned[0]
        sl = slice(lo, lo + (out.stop - out.start))
        mean[:, out] = mu[:, sl]
        if want_sd:
            sd[:, out] = s[:, sl]
        return t1 - t0, time.perf_counter() - t1

    def whole(r):
        s1, s2 = model.len_vec[r][1], model.len_vec[r][2]
        return run(model.blocks[r], slice(s1, s2), slice(0, s2 - s1))

    by_size = sorted(model.my_regions, key=lambda r: -int(model.len_vec[r][0]))
    pending = model.runner.start(whole, by_size)
    times = []
    for g in model.conductor.groups:
        s1 = model.len_vec[g.block_id][1]
        for t in sorted(g.local):
            tl = g.local[t]
            own = tl.owned_global_slice()
            times.append(run(tl.b, slice(s1 + own.start, s1 + own.stop), tl.owned_local_slice()))
    for te, ta in times + pending.results():
        timing["emission"] += te
        timing["ancestral"] += ta
    if model.world > 1:
        t0 = time.perf_counter()
        red = model.reducer
        mean = red.allreduce_bytes(mean.view(np.uint8).reshape(-1)).view(np.float32).reshape(A, n)
        if want_sd:
            sd = red.allreduce_bytes(sd.view(np.uint8).reshape(-1)).view(np.float32).reshape(A, n)
        timing["gather"] = time.perf_counter() - t0
    return dict(nodes=model.tree.internal_nodes.copy(), parent=model.tree.parent.copy(), mean=mean, sd=sd,
                timing={k: 1e3 * v for k, v in timing.items()})


def save_npz(path, res, weighting, len_vec, species=None):
    """the result of reconstruct() as an .npz without pickles: nodes, parent, species (leaf names, empty when unknown), mean,
    sd (empty [0, 0] when not computed), len_vec, weighting"""
    sd = res["sd"] if res["sd"] is not None else np.zeros((0, 0), dtype=np.float32)
    np.savez(path, nodes=np.asarray(res["nodes"], dtype=np.int64), parent=np.asarray(res["parent"], dtype=np.int64),
             species=np.asarray([] if species is None else [str(s) for s in species], dtype=np.str_),
             mean=np.asarray(res["mean"], dtype=np.float32), sd=np.asarray(sd, dtype=np.float32),
             len_vec=np.asarray(len_vec, dtype=np.int64), weighting=np.asarray(str(weighting)))
    return path


def load_npz(path):
    """-> dict with NPZ_KEYS; species a list of str, weighting a str, sd None when it was not computed"""
    with np.load(path, allow_pickle=False) as z:
        d = {k: z[k].copy() for k in NPZ_KEYS}
    d["species"] = [str(s) for s in d["species"].tolist()]
    d["weighting"] = str(d["weighting"])
    if d["sd"].size == 0 and d["mean"].size != 0:
        d["sd"] = None
    return d
