"""CPU: the image of a state map -- the full-matrix restatement of tests/render_reference.py on cases worked out by hand, the
host helpers of phylo_hmrf_amd.render (factor, palettes, the PNG writer) and the command line's --render refusals."""
import os

import numpy as np
import pytest

from phylo_hmrf_amd import render
from tests import render_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LV = np.array([[6, 0, 6, 3, 3, 0, 0, 0, 1, 1]], dtype=np.int64)
PAL = np.array([[10, 20, 30], [200, 100, 0], [0, 0, 255], [90, 90, 90]], dtype=np.uint8)


# ---- the definition, by hand ------------------------------------------------------------------------------------------------
def test_diagonal_3x3_at_factor_2_counts_the_corner_pixels_off_diagonal_cells_twice():
    # stored (0,0) (0,1) (0,2) (1,1) (1,2) (2,2); M = [[0,1,2],[1,2,2],[2,2,0]]
    labels = [0, 1, 2, 2, 2, 0]
    conf = np.array([1.0, 0.5, 0.25, 0.0, 0.75, 1.0], dtype=np.float32)
    mark = [0, 0, 7, 0, 0, 0]
    assert R.full(labels, 3, 3, True).tolist() == [[0, 1, 2], [1, 2, 2], [2, 2, 0]]
    state, conf8, mark8 = R.planes(labels, 3, 3, True, 3, 2, conf, mark)
    # pixel (0, 0) holds {0, 1, 1, 2}: state 1 wins because (0, 1) stands for (1, 0) too -- counted once, all three would tie
    assert state.tolist() == [[1, 2], [2, 0]]
    # (0,0): 0.5 + 0.5 over 2 cells; (0,1) and (1,0): 0.25 + 0.75 over 2 cells; (1,1): 1.0 -> floor(255 / 2) = 127
    assert conf8.tolist() == [[127, 127], [127, 255]]
    assert mark8.tolist() == [[0, 1], [1, 0]]
    s0, c0, m0 = R.planes(labels, 3, 3, True, 3, 2)
    assert s0.tolist() == state.tolist() and c0.tolist() == [[255, 255], [255, 255]] and m0.tolist() == [[0, 0], [0, 0]]


def test_offdiagonal_2x5_at_factor_2_has_a_ragged_last_column():
    labels = [0, 0, 1, 1, 2,
              0, 1, 1, 1, 0]
    state, conf8, mark8 = R.planes(labels, 2, 5, False, 3, 2, mark=[0] * 9 + [1])
    assert state.shape == (1, 3)
    assert state.tolist() == [[0, 1, 0]]                     # {0,0,0,1}, {1,1,1,1}, and the last column alone {2, 0}: a tie
    assert mark8.tolist() == [[0, 0, 1]] and conf8.tolist() == [[255, 255, 255]]


def test_a_tie_goes_to_the_lowest_state():
    state, _, _ = R.planes([3, 1, 1, 3], 2, 2, False, 4, 2)
    assert state.tolist() == [[1]]
    state, _, _ = R.planes([2, 0, 1, 2, 0, 1], 1, 6, False, 3, 6)
    assert state.tolist() == [[0]]


def test_colour_by_hand():
    state = np.array([[0, 0, 1], [0, 1, 1]], dtype=np.uint8)
    conf8 = np.array([[255, 127, 0], [255, 255, 255]], dtype=np.uint8)
    mark8 = np.array([[0, 0, 0], [0, 0, 1]], dtype=np.uint8)
    rgb = R.colour(state, conf8, mark8, PAL, (255, 0, 255), (0, 0, 0), False)
    assert rgb[0, 0].tolist() == [10, 20, 30]                # full confidence: the palette colour itself
    assert rgb[0, 1].tolist() == [103, 109, 115]             # t = 64 + 191 * 127 // 255 = 159; 255 - 245 * 159 // 255 = 103
    assert rgb[0, 2].tolist() == [242, 217, 191]             # t = 64; 255 - 55 * 64 // 255 = 242, 255 - 155 * 64 // 255 = 217
    assert rgb[1, 2].tolist() == [255, 0, 255]
    lined = R.colour(state, conf8, mark8, PAL, (255, 0, 255), (1, 2, 3), True)
    # (0,0): right equal, below equal; (0,1): right differs; (0,2): below equal, no right; (1,0): right differs; (1,1): marked right
    assert lined[0, 0].tolist() == [10, 20, 30] and lined[0, 1].tolist() == [1, 2, 3] and lined[1, 0].tolist() == [1, 2, 3]
    assert lined[0, 2].tolist() == rgb[0, 2].tolist()
    assert lined[1, 1].tolist() == [200, 100, 0]             # the mark colours a pixel, it does not change its state
    assert lined[1, 2].tolist() == [255, 0, 255]


# ---- host helpers -----------------------------------------------------------------------------------------------------------
def test_choose_factor_at_the_edges():
    assert render.choose_factor(1, 1, 1) == 1
    assert render.choose_factor(2048, 2048, 2048) == 1
    assert render.choose_factor(2049, 5, 2048) == 2
    assert render.choose_factor(5, 4096, 2048) == 2
    assert render.choose_factor(5, 4097, 2048) == 3
    assert render.choose_factor(24895, 24895, 2048) == 13
    assert render.choose_factor(70, 3, 1) == 70
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        with pytest.raises(ValueError):
            render.choose_factor(*bad)


@pytest.mark.parametrize("K", range(1, 65))
def test_default_palette_is_distinct_and_avoids_the_reserved_colours(K):
    p = render.default_palette(K)
    assert p.shape == (K, 3) and p.dtype == np.uint8
    rows = [tuple(int(x) for x in r) for r in p]
    assert len(set(rows)) == K
    for reserved in ((255, 255, 255), render.HIGHLIGHT, render.OUTLINE):
        assert tuple(reserved) not in rows
    assert np.array_equal(p, render.default_palette(64)[:K])     # state k has one colour whatever K is


def test_default_palette_is_not_the_reference_table_and_refuses_other_K():
    with pytest.raises(ValueError):
        render.default_palette(0)
    with pytest.raises(ValueError):
        render.default_palette(65)
    assert render.default_palette(3).tolist() == [[225, 30, 30], [30, 165, 68], [123, 30, 195]]


def test_load_palette(tmp_path):
    path = str(tmp_path / "colours.txt")
    with open(path, "w") as fh:
        fh.write("0\t60\t48\n1 102   94\n\n255\t0\t7\r\n")
    assert render.load_palette(path, 3).tolist() == [[0, 60, 48], [1, 102, 94], [255, 0, 7]]
    assert render.load_palette(path, 2).tolist() == [[0, 60, 48], [1, 102, 94]]
    with pytest.raises(ValueError, match="3 colours for 4 states"):
        render.load_palette(path, 4)
    for text in ("0 0 256\n", "0 0\n", "0 0 0 0\n", "0 -1 0\n", "0 0.5 0\n", "r g b\n"):
        with open(path, "w") as fh:
            fh.write("1 2 3\n" + text)
        with pytest.raises(ValueError, match="line 2"):
            render.load_palette(path, 1)
    with pytest.raises(ValueError):
        render.load_palette(path, 0)


# ---- PNG --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (5, 3), (7, 1), (40, 33)])
def test_write_png_round_trips(tmp_path, h, w):
    rgb = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w, 3)).astype(np.uint8)
    rgb[0, 0] = (0, 128, 255)
    path = str(tmp_path / "a.png")
    render.write_png(path, rgb)
    assert np.array_equal(R.decode_png(path), rgb)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as img:
        assert img.mode == "RGB" and img.size == (w, h)
        assert np.array_equal(np.asarray(img), rgb)


def test_write_png_refuses_what_is_not_an_rgb_image(tmp_path):
    path = str(tmp_path / "a.png")
    for bad in (np.zeros((2, 2), np.uint8), np.zeros((2, 2, 4), np.uint8), np.zeros((2, 2, 3), np.int32),
                np.zeros((0, 2, 3), np.uint8)):
        with pytest.raises(ValueError):
            render.write_png(path, bad)
    assert not os.path.exists(path)


# ---- arguments refused before the library -----------------------------------------------------------------------------------
def test_render_states_refuses_bad_arguments_before_the_library():
    z = np.zeros(6, dtype=np.int64)
    with pytest.raises(ValueError):
        render.render_states(z[:5], LV)
    with pytest.raises(ValueError):
        render.render_states(z, LV, conf=np.ones(5))
    with pytest.raises(ValueError):
        render.render_states(z, LV, mark=np.ones(7))
    with pytest.raises(ValueError):
        render.render_states(z, LV, factor=0)
    with pytest.raises(ValueError):
        render.render_states(z, LV, max_side=0)
    with pytest.raises(ValueError):
        render.render_states(z + 3, LV, palette=PAL[:3])
    with pytest.raises(ValueError):
        render.render_states(z, LV, palette=np.full((1, 3), 256))
    with pytest.raises(ValueError):
        render.render_states(z, LV, highlight=(1, 2))
    with pytest.raises(ValueError):
        render.render_states(z, LV, outline_colour=(1, 2, 300))
    with pytest.raises(ValueError):
        render.render_states(z + 64, LV)


def test_no_host_fallback():
    from phylo_hmrf_amd import _lib
    if _lib.device_count() == 0:                            # (tests/test_gpu_render.py runs the call where there is one)
        with pytest.raises(RuntimeError):
            render.render_states(np.zeros(6, dtype=np.int64), LV)


def test_render_files_refuses_before_it_draws(tmp_path):
    import scipy.io
    path, other = str(tmp_path / "a.mat"), str(tmp_path / "compare_b.mat")
    scipy.io.savemat(path, dict(state_vec=np.zeros((1, 6), dtype=np.int64), len_vec=LV))
    with pytest.raises(ValueError, match="state_vec_smooth"):
        render.render_files(path, str(tmp_path), field="state_vec_smooth")
    with pytest.raises(ValueError, match="max_side"):
        render.render_files(path, str(tmp_path), max_side=0)
    with pytest.raises(ValueError, match="conf"):
        render.render_files(path, str(tmp_path), use_conf=True)
    with pytest.raises(ValueError, match="diff_vec"):
        render.render_files(path, str(tmp_path), mark_path=path)
    lv2 = LV.copy()
    lv2[0, 5] = 9
    scipy.io.savemat(other, dict(diff_vec=np.zeros((1, 6), dtype=np.uint8), len_vec=lv2))
    with pytest.raises(ValueError, match="regions"):
        render.render_files(path, str(tmp_path), mark_path=other)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("render_")]


# ---- the command line -------------------------------------------------------------------------------------------------------
def _cli(**extra):
    import phylo_hmrf as cli
    return cli.run("5", "1", ".", "true", "human", "false", "0", "1", "1", "0", "0.3", "0.1", "1", "0", "50000", "0.25", "1",
                   "0.5", "8", "0", "0.001", "0", "1", "test", "0", "0", "3", "50000", "1", "hg38", "unused", quiet="1", **extra)


@pytest.mark.parametrize("extra", [
    dict(segment="m.npz"),
    dict(postprocess="x.mat"),
    dict(compare="a.mat", compare_with="b.mat"),
    dict(compare="a.mat"),
    dict(domains="a.mat"),
    dict(segment="m.npz", ancestral="posterior"),
    dict(ancestral="posterior"),
    dict(save_model="m.npz"),
    dict(profile="1"),
    dict(filter_device="1"),
    dict(render_field="top"),
    dict(render_side="0"),
    dict(render_side="-3"),
    dict(render_side="wide"),
    dict(render_outline="2"),
    dict(render_conf="yes"),
])
def test_cli_refusals(extra):
    with pytest.raises(SystemExit) as e:
        _cli(render="a.mat", **extra)
    assert "--render" in str(e.value)
    assert not os.path.exists("unused")


def test_cli_parses_the_options_with_their_defaults():
    import phylo_hmrf as cli
    o = cli.parse_args(["--render", "a.mat"])
    assert (o.render, o.render_field, o.render_side, o.render_colors, o.render_outline, o.render_conf, o.render_mark) == \
        ("a.mat", "state_vec", "2048", "", "0", "0", "")
    o = cli.parse_args(["--render", "a.mat", "--render_field", "state_vec_smooth", "--render_side", "512", "--render_colors",
                        "c.txt", "--render_outline", "1", "--render_conf", "1", "--render_mark", "compare_a__b.mat"])
    assert (o.render_field, o.render_side, o.render_colors, o.render_outline, o.render_conf, o.render_mark) == \
        ("state_vec_smooth", "512", "c.txt", "1", "1", "compare_a__b.mat")
    assert cli.parse_args([]).render == ""
    assert cli.check_render("", "top", "0", "2", "2", "m.npz", "", "", "", "", "", "0", "0") is None      # off: nothing to refuse
    assert cli.check_render("a.mat", "state_vec", "7", "0", "1", "", "", "", "", "", "", "0", "0") == 7


def test_constants_are_the_headers_and_the_sources():
    from phylo_hmrf_amd import _lib
    txt = open(os.path.join(ROOT, "include", "phmrf.h")).read()
    assert "#define PHMRF_VERSION 127\n" in txt and _lib.ABI_VERSION == 127          # no ABI bump: an entry point only
    assert "PHMRF_API int phmrf_render_states(" in txt and txt.count("phmrf_render_states") >= 2
    assert len(_lib.SIGNATURES["phmrf_render_states"]) == 14
    src = open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "render.hip")).read()
    assert "RENDER_GRID_CAP = %d;" % render.GRID_CAP in src
    assert "RENDER_TILE = %d;" % render.TILE in src
    assert "RENDER_MAX_FACTOR = %d;" % render.MAX_FACTOR in src
    assert "render.hip" in open(os.path.join(ROOT, "phylo_hmrf_amd", "csrc", "Makefile")).read()
