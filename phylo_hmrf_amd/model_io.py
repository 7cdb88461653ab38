"""A fitted Phylo-HMRF model as one self-contained file, to segment data it was not fitted on (segment.py).

The reference leaves a fit only as `estimate_ou_*.mat` (state_vec, params_vec1, params_vec2, ...): no tree, no beta, no
preprocessing, so nothing can read it back as a model.  `save_model` writes an .npz (no pickles) holding
  - format, K, S, the species tree (edge_list, branch_list) and species names;
  - the parameters the model holds when fit_accumulate_test returns: means_ / _covars_ (from params_vec, base.py:445) and
    params_vec / params_vec1;
  - the energy's and the solver's settings: min_covar, beta, beta1, estimate_type, num_neighbor, energy_tol_ppb;
  - the preprocessing that defines the features: x_max, resolution, filter_mode, filter_sigma, diagonal_type (NaN / -1
    where they do not apply, e.g. synthetic data).
Scalars and strings travel in one JSON string (`meta`), as the checkpoint's model_key does.  `load_model` recomputes the
Gaussians from the OU parameters and the tree and refuses a file whose stored ones disagree.
"""
import json
import os

import numpy as np

MODEL_FORMAT = 1
PREPROCESSING = ("x_max", "resolution", "filter_mode", "filter_sigma", "diagonal_type")
_PRE_DEFAULTS = dict(x_max=float("nan"), resolution=-1, filter_mode=-1, filter_sigma=float("nan"), diagonal_type=-1)
_REL_TOL = 1e-9


class Model(object):
    """What load_model returns: plain attributes, arrays as saved"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def fields(self):
        return dict(self.__dict__)


def save_model(model, path, species=None, **preprocessing):
    """Write `model` (a fitted phyloHMRF, or any object with its attributes) to `path` (.npz).  species: the leaves' names,
    if known; preprocessing: x_max, resolution, filter_mode, filter_sigma, diagonal_type of the run that made the features
    (missing ones: NaN / -1)."""
    unknown = sorted(set(preprocessing) - set(PREPROCESSING))
    if unknown:
        raise ValueError("unknown preprocessing settings %s (known: %s)" % (unknown, ", ".join(PREPROCESSING)))
    pre = dict(_PRE_DEFAULTS)
    pre.update({k: v for k, v in preprocessing.items() if v is not None})
    K, S = int(model.n_components), int(model.n_features)
    means, covars = np.asarray(model.means_, dtype=np.float64), np.asarray(model._covars_, dtype=np.float64)
    if means.shape != (K, S) or covars.shape != (K, S, S):
        raise ValueError("the model's means_ %s / _covars_ %s do not have K = %d states of S = %d species"
                         % (means.shape, covars.shape, K, S))
    params_vec = np.asarray(getattr(model, "params_vec", model.params_vec1), dtype=np.float64)
    branch = getattr(model, "branch_params", None)
    meta = dict(K=K, S=S, min_covar=float(model.min_covar), beta=float(model.beta), beta1=float(model.beta1),
                estimate_type=int(model.estimate_type), num_neighbor=int(model.num_neighbor),
                energy_tol_ppb=int(getattr(model, "solver_opts", {}).get("energy_tol_ppb", 10000)),
                have_branch_list=branch is not None, species=None if species is None else [str(s) for s in species],
                x_max=float(pre["x_max"]), resolution=int(pre["resolution"]), filter_mode=int(pre["filter_mode"]),
                filter_sigma=float(pre["filter_sigma"]), diagonal_type=int(pre["diagonal_type"]))
    d = dict(format=np.int64(MODEL_FORMAT), meta=json.dumps(meta, sort_keys=True),
             edge_list=np.asarray(model.edge_list, dtype=np.int64).reshape(-1, 2),
             branch_list=np.asarray([] if branch is None else branch, dtype=np.float64),
             means_=means, _covars_=covars, params_vec=params_vec,
             params_vec1=np.asarray(model.params_vec1, dtype=np.float64))
    tmp = path + ".tmp.npz"
    np.savez(tmp, **d)
    os.replace(tmp, path)
    return path


def load_model(path):
    """-> Model with K, S, edge_list, branch_list, species, means_, _covars_, params_vec, params_vec1, min_covar, beta,
    beta1, estimate_type, num_neighbor, energy_tol_ppb and the preprocessing settings.  Raises ValueError for an unknown
    format or stored Gaussians that the OU parameters and the tree do not reproduce."""
    from .tree import PhyloTree
    with np.load(path, allow_pickle=False) as z:
        if "format" not in z.files or int(z["format"]) != MODEL_FORMAT:
            raise ValueError("%s is not a Phylo-HMRF model file of format %d" % (path, MODEL_FORMAT))
        meta = json.loads(str(z["meta"]))
        arrays = {k: z[k].copy() for k in ("edge_list", "branch_list", "means_", "_covars_", "params_vec", "params_vec1")}
    K, S = int(meta["K"]), int(meta["S"])
    tree = PhyloTree([list(map(int, e)) for e in arrays["edge_list"].tolist()])
    if tree.n_features != S or arrays["params_vec"].shape != (K, tree.n_params):
        raise ValueError("%s: the tree has %d leaves and %d OU parameters per state, the file S = %d and params_vec %s"
                         % (path, tree.n_features, tree.n_params, S, arrays["params_vec"].shape))
    means, covars = tree.mean_cov(arrays["params_vec"], float(meta["min_covar"]))
    for name, want in (("means_", means), ("_covars_", covars)):
        got = arrays[name]
        if got.shape != want.shape:
            raise ValueError("%s: %s has shape %s, the tree gives %s" % (path, name, got.shape, want.shape))
        err = np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300) if want.size else 0.0
        if not err <= _REL_TOL:
            raise ValueError("%s: the stored %s disagree with the OU parameters and the tree by %.3g relative (> %g)"
                             % (path, name, err, _REL_TOL))
    kw = dict(meta)
    kw.pop("have_branch_list")
    kw.update(arrays)
    kw["branch_list"] = arrays["branch_list"] if meta["have_branch_list"] else None
    kw["tree"] = tree
    return Model(**kw)


def check_observation(model, observation, n_components=None):
    """ValueError unless the observations [n, S] have the model's S species and a requested state count is the model's K
    (called before the GPU is touched)"""
    X = np.asarray(observation)
    if X.ndim != 2 or X.shape[1] != int(model.S):
        raise ValueError("the model has S = %d species, the observations have shape %s" % (int(model.S), X.shape))
    if n_components is not None and int(n_components) != int(model.K):
        raise ValueError("the model has K = %d states, %d were asked for" % (int(model.K), int(n_components)))
