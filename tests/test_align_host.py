"""vdf_align_windows_host - the definition of the align calls in plain C++ (include/vdf.h) - against the numpy twin of
tests/aligngen.py: every problem the GPU test gives the kernel, plus 200 random small ones.  Records are compared for equality."""
import numpy as np
import pytest

import aligngen


def host(p, capacity=4096):
    from vid_dup_finder_lib_amd import align_windows_host

    rec, found = align_windows_host(p.a_hashes, p.a_first, p.b_hashes, p.b_first, tol_int=p.tol, min_run=p.min_run, a_skip=p.a_skip, b_skip=p.b_skip,
                                    capacity=capacity)
    return aligngen.records(rec), found


@pytest.mark.parametrize("name", sorted(aligngen.CASES))
def test_host_form_matches_the_twin(name):
    got, found = host(aligngen.case(name))
    want = list(aligngen.expected(name))
    assert found == len(want)
    assert got == want


def test_the_cases_say_what_they_are_meant_to():
    """the problems' builders against their own intent: a case that has drifted from what its name says would test nothing"""
    e = {k: list(aligngen.expected(k)) for k in aligngen.CASES}
    assert e["first_diagonal"] == [(0, 0, -69, 69, 1, 3), (1, 1, 0, 0, 1, 0), (2, 2, 0, 0, 1, 1), (3, 3, -39, 39, 1, 2)]
    assert e["last_diagonal"] == [(0, 0, 49, 0, 1, 3), (1, 1, 129, 0, 1, 0), (2, 2, 1, 0, 1, 9)]
    assert [(r[2], r[3], r[4]) for r in e["edges"]] == [(17, 0, 9), (-23, 23, 9), (-41, 71, 9), (69, 12, 9)]
    assert [(r[2], r[3], r[4]) for r in e["reload_wrap"]] == [(5, 60, 70), (-59, 60, 70)]
    assert e["band_neighbours_first"] == [(0, 0, -36, 40, 10, 0)] and e["band_neighbours_second"] == [(0, 0, -35, 60, 10, 0)]
    assert e["two_runs_one_diagonal"] == [(0, 0, 5, 50, 12, 48)]
    assert e["tie_two_diagonals"] == [(0, 0, -7, 10, 8, 0), (1, 1, -7, 10, 8, 48)]
    assert e["tie_one_diagonal"] == [(0, 0, 7, 8, 6, 12)]
    for t in (0, 1, 350):
        assert e[f"tolerance_{t}"] == [(0, 0, -1, 2, 1, t)]
    for t in (1024, 5000):  # every cell matches: three full-length runs per pair
        assert [r[:5] for r in e[f"tolerance_{t}"]] == [(a, b, 0, 0, 3) for a in range(3) for b in range(3)]
    assert e["min_run_1"] == [(0, 0, 38, 2, 1, 0)] and e["min_run_2"] == [(0, 0, 10, 10, 2, 400)] and e["min_run_16"] == [(0, 0, -27, 30, 16, 16 * 335)]
    assert [(r[0], r[3], r[4]) for r in e["skip_cuts"]] == [(0, 10, 10), (1, 8, 7)] and [r[:2] for r in e["skip_silences"]] == [(1, 1)]
    assert e["static_equal"] == [(0, 0, 0, 0, 70, 0)]
    assert e["static_a_shorter"] == [(0, 0, 0, 0, 40, 0), (0, 1, 0, 0, 40, 0), (1, 0, 0, 0, 3, 0), (1, 1, 0, 0, 3, 0)]
    assert e["static_a_longer"] == [(0, 0, -64, 64, 65, 0)]
    assert [r[:2] for r in e["static_self"]] == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    pairs = {r[:2] for r in e["self_mode"]}  # the planted copies (and the copies of copies); (6, 10) is one cell: under min_run = 2
    assert all(a < b for a, b in pairs) and {(0, 1), (1, 3), (2, 5), (3, 7), (4, 9), (0, 10), (7, 11), (5, 11)} <= pairs and (6, 10) not in pairs
    assert len(e["mixed_counts"]) >= 12 and all(r[1] != 1 for r in e["mixed_counts"])  # video 1 of B has no windows


def test_self_mode_is_a_against_a_without_the_lower_triangle():
    p = aligngen.case("self_mode")
    both, _ = host(p._replace(b_hashes=p.a_hashes, b_first=p.a_first))
    assert [r for r in both if r[0] < r[1]] == list(aligngen.expected("self_mode"))
    assert any(r[0] == r[1] for r in both)  # against itself a video matches on offset 0: self mode leaves it out


def test_capacity_smaller_than_the_result():
    want = list(aligngen.expected("self_mode"))
    got, found = host(aligngen.case("self_mode"), capacity=3)
    assert found == len(want) and got == want[:3]
    got, found = host(aligngen.case("self_mode"), capacity=0)
    assert found == len(want) and got == []


def test_random_small_problems():
    rng = np.random.default_rng(2024)
    seen = 0
    for _ in range(200):
        p = aligngen.random_problem(rng)
        got, found = host(p)
        want = aligngen.align_twin(p)
        assert got == want and found == len(want)
        seen += len(want)
    assert seen > 300  # the problems are not empty
