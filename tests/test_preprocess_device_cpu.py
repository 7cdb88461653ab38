"""CPU side of the GPU filters of the raw loader (csrc/preprocess.hip, preprocess.*_device): the float64 yardstick the GPU
tests measure the diffusion against, the refusal to fall back to the host, the unchanged default and the header's text."""
import os
import re

import numpy as np
import pytest

from phylo_hmrf_amd import preprocess
from tests.diffusion_f64 import DIFFUSION_CASES, DIFFUSION_SHAPES, contact_like, diffusion_f64
from tests.test_preprocess import RES, SPECIES, _perona_malik_by_the_book, _write_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "phylo_hmrf_amd", "libphmrf.so")


@pytest.mark.parametrize("shape", DIFFUSION_SHAPES)
@pytest.mark.parametrize("niter,kappa,option", DIFFUSION_CASES + [(3, 0.05, 2)])
def test_f64_yardstick_bounds_the_host_filters_rounding(shape, niter, kappa, option):
    """e_ref = max |anisotropic_diffusion - float64 recurrence| is the float32 restatement's own rounding error: above 0 (the
    two are not the same computation) and below 1e-6 (a few float32 ulps of values below 2: a wrong stencil, border or sign in
    either would show at 1e-3 and above)."""
    img = contact_like(np.random.default_rng(11), shape)
    ref = diffusion_f64(img, niter, kappa, 0.1, option)
    host = preprocess.anisotropic_diffusion(img, niter=niter, kappa=kappa, gamma=0.1, option=option)
    assert host.dtype == np.float32 and ref.dtype == np.float64 and ref.shape == host.shape
    e_ref = float(np.abs(host.astype(np.float64) - ref).max())
    assert 0.0 < e_ref < 1e-6, e_ref


@pytest.mark.parametrize("shape,niter,kappa", [((3, 3), 1, 50.0), ((5, 5), 5, 50.0), ((4, 7), 5, 0.5), ((1, 8), 3, 0.05),
                                               ((8, 1), 10, 50.0)])
def test_f64_yardstick_is_the_published_update_rule(shape, niter, kappa):
    """The yardstick against the per-pixel rule of Perona & Malik written out in tests/test_preprocess.py, both in float64:
    they differ by the order of a handful of float64 operations only."""
    img = contact_like(np.random.default_rng(12), shape)
    want = _perona_malik_by_the_book(np.asarray(img, dtype=np.float32), niter, kappa, 0.1)
    got = diffusion_f64(img, niter, kappa, 0.1, 1)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)


def _no_gpu():
    if not os.path.exists(LIB):
        pytest.skip("libphmrf.so not built")
    from phylo_hmrf_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")


def test_device_filters_fail_loudly_without_a_gpu():
    _no_gpu()
    img = contact_like(np.random.default_rng(1), (9, 7))
    with pytest.raises(RuntimeError):
        preprocess.anisotropic_diffusion_device(img, niter=5, kappa=50, gamma=0.1, option=1)
    with pytest.raises(RuntimeError):
        preprocess.denoise_bilateral_device(img, sigma_color=0.5, sigma_spatial=1)
    with pytest.raises(RuntimeError):
        preprocess.gaussian_filter_device(img, 0.25)


@pytest.fixture(scope="module")
def window(tmp_path_factory):
    g = np.load(os.path.join(ROOT, "tests", "golden", "example_loader.npz"))
    d, flist = _write_dir(tmp_path_factory.mktemp("win"), g, "22", int(g["first_bin"]), 120, 0, g["a_synteny"])
    sizes = os.path.join(d, "hg38.chrom.sizes")
    mv = preprocess.quantile_contact_vec([22], RES, sizes, flist, SPECIES)
    return g, d, flist, sizes, float(np.median(mv[:, 6]))


@pytest.mark.parametrize("fm,sigma", [(2, 0.25), (0, 0.25), (1, 0.25)])
def test_loader_does_not_fall_back_to_the_host(window, fm, sigma):
    _no_gpu()
    g, d, flist, sizes, x_max = window
    with pytest.raises(RuntimeError):
        preprocess.load_data_chromosome2([22], x_max, 0, RES, 8, fm, sigma, 0, sizes, flist, SPECIES, d, "t",
                                         filter_device=True)


def test_loader_default_is_unchanged(window):
    """filter_device=False through the new keyword: the golden window, bit for bit (tests/test_preprocess.py's assertion)."""
    g, d, flist, sizes, x_max = window
    for tag, fm, sigma in (("none", 2, 0.0), ("gauss", 2, 0.25), ("diffusion", 0, 0.25)):
        samples, len_vec, elv = preprocess.load_data_chromosome2([22], x_max, 0, RES, 8, fm, sigma, 0, sizes, flist, SPECIES,
                                                                 d, "t", filter_device=False)
        assert np.array_equal(np.asarray(len_vec), g["a_%s_lenvec" % tag]), tag
        assert np.array_equal(samples, g["a_%s_samples" % tag]), tag
        if tag == "none":
            assert np.array_equal(elv[0], g["a_none_edges"])


def test_cli_refuses_the_flag_where_nothing_is_filtered():
    import phylo_hmrf as cli
    o = cli.parse_args([])
    assert o.filter_device == "0"
    args = [o.num_states, o.chromvec, o.root_path, o.multiple, o.species_name, o.sort_states, o.run_id, o.cons_param,
            o.method_mode, o.initial_mode, o.initial_weight, o.initial_weight1, o.initial_magnitude, o.position1, o.position2,
            o.filter_sigma, o.beta, o.beta1, o.num_neighbor, o.filter_mode, o.threshold, o.estimate_type, o.simu_version,
            o.annotation, "1", o.dtype, o.miter, o.resolution, o.quantile, o.ref_species, o.output]
    with pytest.raises(SystemExit, match="--reload 1"):
        cli.run(*args, filter_device="1")
    args[24] = "0"
    with pytest.raises(SystemExit, match="--synthetic"):
        cli.run(*args, filter_device="1", synthetic="32")
    with pytest.raises(SystemExit, match="--postprocess"):
        cli.run(*args, filter_device="1", postprocess="x.mat")


def test_header_documents_the_three_filters():
    txt = open(os.path.join(ROOT, "include", "phmrf.h")).read()
    assert re.search(r"#define\s+PHMRF_VERSION\s+127\b", txt)
    m = re.search(r"/\* ABI 127:(.*?)\*/\s*PHMRF_API int phmrf_filter_diffusion\(", txt, re.S)
    assert m, "phmrf_filter_diffusion has no ABI 127 comment"
    general = m.group(1)
    for name in ("phmrf_filter_diffusion", "phmrf_filter_bilateral", "phmrf_filter_gaussian"):
        c = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*PHMRF_API int %s\(" % name, txt, re.S)
        assert c, name
        text = c.group(1) + (general if name != "phmrf_filter_diffusion" else "")
        assert name in text
        assert re.search(r"float(32|64) \[H W\]", text), (name, "dtypes")
        assert "pixel" in text, (name, "units")
        assert "PHMRF_ERR_INVALID" in text and "PHMRF_ERR_UNSUPPORTED" in text, (name, "error codes")
    from phylo_hmrf_amd import _lib
    assert _lib.ABI_VERSION == 127
    for name in ("phmrf_filter_diffusion", "phmrf_filter_bilateral", "phmrf_filter_gaussian"):
        assert name in _lib.SIGNATURES
