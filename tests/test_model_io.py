"""CPU: the model file of a fit (phylo_hmrf_amd/model_io.py) -- round trip, refusals -- and the command line's new options.
Nothing here touches a GPU."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from phylo_hmrf_amd import model_io, synthetic  # noqa: E402
from phylo_hmrf_amd.tree import PhyloTree  # noqa: E402


class FittedStandIn(object):
    """the attributes of a phyloHMRF after fit_accumulate_test that save_model reads"""

    def __init__(self, K=5, S=4, seed=0):
        rng = np.random.default_rng(seed)
        self.edge_list = synthetic.tree_for(S)
        self.tree = PhyloTree(self.edge_list)
        self.n_components, self.n_features = K, S
        self.params_vec = synthetic.sample_ou_params(rng, self.tree, K)
        self.params_vec1 = self.params_vec + 0.01 * rng.random(self.params_vec.shape)
        self.min_covar = 1e-3
        self.means_, self._covars_ = self.tree.mean_cov(self.params_vec, self.min_covar)
        self.branch_params = [0.5] * len(self.edge_list)
        self.beta, self.beta1, self.estimate_type, self.num_neighbor = 1.25, 0.5, 3, 8
        self.solver_opts = dict(energy_tol_ppb=1000, max_rounds=64)


def test_round_trip_returns_every_field_bit_for_bit(tmp_path):
    m = FittedStandIn()
    path = str(tmp_path / "m.npz")
    model_io.save_model(m, path, species=["hg38", "mm10", "a", "b"], x_max=12.5, resolution=50000, filter_mode=0,
                        filter_sigma=0.25, diagonal_type=0)
    assert not os.path.exists(path + ".tmp.npz")
    z = model_io.load_model(path)
    assert (z.K, z.S) == (5, 4)
    assert z.edge_list.tolist() == np.asarray(m.edge_list).tolist()
    assert z.branch_list.tolist() == m.branch_params
    assert z.species == ["hg38", "mm10", "a", "b"]
    for name in ("means_", "_covars_", "params_vec", "params_vec1"):
        want = np.asarray(getattr(m, name))
        got = getattr(z, name)
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), name
    assert (z.min_covar, z.beta, z.beta1, z.estimate_type, z.num_neighbor, z.energy_tol_ppb) == (1e-3, 1.25, 0.5, 3, 8, 1000)
    assert (z.x_max, z.resolution, z.filter_mode, z.filter_sigma, z.diagonal_type) == (12.5, 50000, 0, 0.25, 0)
    # the Gaussians the file's OU parameters and tree give agree with the stored ones
    mu, cv = z.tree.mean_cov(z.params_vec, z.min_covar)
    assert np.allclose(mu, z.means_, rtol=1e-12, atol=0) and np.allclose(cv, z._covars_, rtol=1e-12, atol=0)
    with np.load(path, allow_pickle=False) as f:              # (no pickled objects in the file)
        assert sorted(f.files) == sorted(["format", "meta", "edge_list", "branch_list", "means_", "_covars_", "params_vec",
                                          "params_vec1"])


def test_synthetic_preprocessing_is_nan_and_minus_one(tmp_path):
    m = FittedStandIn(K=3)
    m.branch_params = None
    path = str(tmp_path / "m.npz")
    model_io.save_model(m, path)
    z = model_io.load_model(path)
    assert np.isnan(z.x_max) and np.isnan(z.filter_sigma)
    assert (z.resolution, z.filter_mode, z.diagonal_type) == (-1, -1, -1)
    assert z.branch_list is None and z.species is None


def _rewrite(path, **changes):
    with np.load(path, allow_pickle=False) as f:
        d = {k: f[k] for k in f.files}
    d.update(changes)
    np.savez(path, **d)


def test_unknown_format_is_refused(tmp_path):
    path = str(tmp_path / "m.npz")
    model_io.save_model(FittedStandIn(), path)
    _rewrite(path, format=np.int64(2))
    with pytest.raises(ValueError, match="format"):
        model_io.load_model(path)


def test_tampered_means_are_refused(tmp_path):
    m = FittedStandIn()
    path = str(tmp_path / "m.npz")
    model_io.save_model(m, path)
    bad = np.array(m.means_, copy=True)
    bad[1, 2] *= 1.0 + 1e-6
    _rewrite(path, means_=bad)
    with pytest.raises(ValueError, match="means_"):
        model_io.load_model(path)
    model_io.save_model(m, path)
    cv = np.array(m._covars_, copy=True)
    cv[0, 0, 1] += 1e-3
    _rewrite(path, _covars_=cv)
    with pytest.raises(ValueError, match="_covars_"):
        model_io.load_model(path)


def test_mismatched_species_or_states_are_refused(tmp_path):
    path = str(tmp_path / "m.npz")
    model_io.save_model(FittedStandIn(K=5, S=4), path)
    z = model_io.load_model(path)
    model_io.check_observation(z, np.zeros((10, 4)))
    with pytest.raises(ValueError, match="S = 4"):
        model_io.check_observation(z, np.zeros((10, 3)))
    with pytest.raises(ValueError):
        model_io.check_observation(z, np.zeros((10, 4)), n_components=6)
    # a file whose K does not match its own parameters
    with np.load(path, allow_pickle=False) as f:
        meta = json.loads(str(f["meta"]))
    meta["K"] = 6
    _rewrite(path, meta=json.dumps(meta))
    with pytest.raises(ValueError):
        model_io.load_model(path)


def test_from_model_refuses_other_species_before_any_gpu_work(tmp_path):
    from phylo_hmrf_amd.hmrf import phyloHMRF
    path = str(tmp_path / "m.npz")
    model_io.save_model(FittedStandIn(S=4), path)
    X = np.zeros((6, 3))
    with pytest.raises(ValueError, match="species"):
        phyloHMRF.from_model(path, X, [[6, 0, 6, 3, 3, 0, 0, 0, 1, 1]], [np.zeros((0, 3))])


def test_cli_options_default_empty_and_segment_settings():
    import phylo_hmrf
    opts = phylo_hmrf.parse_args([])
    assert opts.save_model == "" and opts.segment == ""
    m = model_io.Model(K=5, resolution=50000, num_neighbor=8, filter_mode=1, filter_sigma=0.5, diagonal_type=0)
    d = phylo_hmrf.PARSER_DEFAULTS
    got = phylo_hmrf.segment_settings(m, d["num_states"], d["resolution"], d["num_neighbor"], d["filter_mode"],
                                      d["filter_sigma"], d["dtype"])
    assert [float(v) for v in got] == [5, 50000, 8, 1, 0.5, 0]
    assert phylo_hmrf.segment_settings(m, "5", "50000", "8", "1", "0.5", "0") == got
    with pytest.raises(ValueError, match="filter_mode"):
        phylo_hmrf.segment_settings(m, "5", "50000", "8", "2", "0.25", "0")
    with pytest.raises(ValueError, match="num_states"):
        phylo_hmrf.segment_settings(m, "7", "50000", "8", "0", "0.25", "0")
