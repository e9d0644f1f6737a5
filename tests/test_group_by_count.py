"""group_by_count (csrc/rt_progressive_plan.hpp): the ordered grouping of a reduction's pixels by sample count that
the per-pixel-count calls of a progressive session build their finish launches from.  tests/group_by_count_check.cpp
compares it with a naive grouping (distinct non-zero counts ascending, pixels appended in pixel order) on the
smallest shapes at which it can go wrong: its one-entry cache of the previous pixel's class must survive strictly
alternating counts, inserts at the front, zeros in between and the second pass that fills the list, and the 257th
distinct count is refused wherever it first appears.  CPU only.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (0, 1, 2, 5, 64)
SHAPES = ("all_zero", "one_class", "alternating", "descending", "zeros_interleaved", "zeros_descending")
CASES = [f"{s}_n{n}" for n in SIZES for s in SHAPES] + \
        ["distinct_256", "distinct_257_at_last_pixel", "distinct_257_at_last_pixel_front", "random_400"]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """One build and one run of the program: {case: the rest of its line}."""
    exe = str(tmp_path_factory.mktemp("group") / "group_by_count_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(HERE, "group_by_count_check.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    lines = dict(line.split(" ", 1) for line in r.stdout.splitlines() if not line.startswith("random map"))
    lines["_exit"] = str(r.returncode)
    lines["_stdout"] = r.stdout
    return lines


def test_every_case_ran_and_the_program_passed(results):
    assert set(CASES) == set(results) - {"_exit", "_stdout"}
    assert results["_exit"] == "0", results["_stdout"]


@pytest.mark.parametrize("case", CASES)
def test_group_by_count_matches_the_naive_grouping(results, case):
    assert results[case] == "ok", results["_stdout"]
