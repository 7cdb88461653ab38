"""phylo_hmrf_amd/maps.py: what the post-processing modules share.  Host only."""
import glob
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the names other code takes from the modules that held them before maps.py
OLD_NAMES = {
    "smooth": ("MAX_STATES", "check_len_vec", "check_state_vec", "default_max_area"),
    "compare": ("MAX_STATES", "FIRST_CAPACITY", "CONF_ONE", "check_len_vec", "check_state_vec", "default_max_area"),
    "domains": ("FIRST_CAPACITY", "CONF_ONE", "load_map", "check_len_vec", "check_state_vec", "default_max_area"),
    "tracks": ("MAX_STATES", "check_len_vec", "check_state_vec"),
    "render": ("MAX_STATES", "check_len_vec", "check_state_vec"),
    "enrich": ("MAX_STATES", "check_len_vec", "check_state_vec"),
}


def test_the_old_names_are_still_there_and_are_the_shared_ones():
    import importlib
    from phylo_hmrf_amd import maps
    for module, names in OLD_NAMES.items():
        mod = importlib.import_module("phylo_hmrf_amd." + module)
        for name in names:
            assert getattr(mod, name) is getattr(maps, name), (module, name)


# the one private name a sibling takes: the EM driver's base class keeps the reference's name (base.py), and the benchmark
# imports it under that name too
KNOWN_PRIVATE = {("hmrf.py", "base", "_BaseGraph")}


def test_no_module_imports_a_private_name_of_a_sibling():
    files = sorted(glob.glob(os.path.join(ROOT, "phylo_hmrf_amd", "*.py")))
    assert len(files) > 20
    for path in files:
        src = open(path).read()
        # `from .mod import a, b [as c]` and the parenthesised form over several lines
        for mod, names in re.findall(r"^\s*from \.(\w+) import (\([^)]*\)|[^\n]*)", src, flags=re.M):
            for name in re.findall(r"\w+", re.sub(r"\bas\s+\w+", "", names.split("#")[0])):
                private = name.startswith("_") and mod != "_lib" and (os.path.basename(path), mod, name) not in KNOWN_PRIVATE
                assert not private, "%s imports %s from .%s" % (os.path.basename(path), name, mod)
        assert not re.search(r"^\s*from \.domains import load_map", src, flags=re.M), path


def test_regions_walks_a_len_vec():
    from phylo_hmrf_amd import maps
    lv = maps.check_len_vec([[6, 0, 6, 3, 3, 10, 10, 0, 1, 1], [12, 6, 18, 3, 4, 10, 25, 1, 0, 1]], 18)
    assert list(maps.regions(lv)) == [(0, 0, 6, 3, 3, 1, 0), (1, 6, 18, 3, 4, 0, 15)]


def test_list_rows_calls_twice_only_when_the_first_table_is_too_small():
    from phylo_hmrf_amd import maps
    for have, calls in ((0, [4]), (4, [4]), (9, [4, 9])):
        seen = []

        def call(capacity, table, found):
            assert table.shape == (max(capacity, 1), 3) and table.dtype == np.int64
            seen.append(capacity)
            table[:min(have, capacity)] = np.arange(min(have, capacity))[:, None]
            found.value = have

        rows = maps.list_rows(call, 3, 4)
        assert seen == calls and rows.shape == (have, 3) and np.array_equal(rows[:, 0], np.arange(have))
