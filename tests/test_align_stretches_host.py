"""vdf_align_windows_stretches_host - the definition of the align-stretches calls in plain C++ (include/vdf.h) - against the numpy
twin of tests/stretchgen.py: every problem the GPU test gives the masked kernel, plus 300 random small ones at several max_stretches and guards.
Records are compared for equality."""
import ctypes as C

import numpy as np
import pytest

import aligngen
import stretchgen


def host(p, max_stretches, guard, capacity=8192):
    from vid_dup_finder_lib_amd import align_windows_stretches_host

    rec, found = align_windows_stretches_host(p.a_hashes, p.a_first, p.b_hashes, p.b_first, tol_int=p.tol, min_run=p.min_run, max_stretches=max_stretches,
                                              guard=guard, a_skip=p.a_skip, b_skip=p.b_skip, capacity=capacity)
    return stretchgen.records(rec), found


@pytest.mark.parametrize("name,guard", stretchgen.CASES)
def test_host_form_matches_the_twin(name, guard):
    p = stretchgen.case(name)
    for max_stretches in (8, 2, 1):
        want = list(stretchgen.expected(name, guard, max_stretches))
        got, found = host(p, max_stretches, guard)
        assert found == len(want)
        assert got == want


def test_the_cases_say_what_they_are_meant_to():
    """the problems' builders against their own intent, on the twin alone"""
    e = lambda name, guard: [r[2:5] for r in stretchgen.expected(name, guard)]
    assert e("ad_removed", 0) == [(0, 0, 100), (-30, 130, 70)]
    assert e("repeat_in_b", 0) == [(-15, 20, 30), (75, 25, 30)]  # the rows 25 ... 49 of A are in both: masked against one part of B only
    assert e("two_runs_one_diagonal", 0) == [(5, 50, 12), (5, 5, 12)]
    assert e("static_tiles", 0) == [(0, 0, 40), (40, 0, 40), (60, 20, 20), (80, 0, 20)]
    across = e("rect_across_bands", 0)
    assert across[0] == (5, 60, 70) and (-130, 140, 30) in across
    assert (40, 48, 12) in across and (40, 95, 12) in across      # ONE run of 59 cells on diagonal 40, cut in two by the rectangle of rank 0
    p = stretchgen.case("rect_across_bands")
    d = aligngen.hashgen.all_distances(p.a_hashes, p.b_hashes)
    assert all(d[ka, ka + 40] == 0 for ka in range(48, 107)) and d[47, 87] > 350 and d[107, 147] > 350
    across2 = e("rect_across_bands", 2)
    assert (40, 48, 10) in across2 and (40, 97, 10) in across2
    assert e("guard_clipped", 5) == [(50, 0, 30), (-23, 33, 17)]
    assert stretchgen.rect_of(50, 0, 30, 5, 60, 80) == (0, 35, 45, 80)  # both clamps act: row 0 of A, the last row of B
    # min_run_after_mask: diagonal 30 holds a run of 26 >= min_run = 8 cells, of which the rectangle of rank 0 leaves 6
    assert e("min_run_after_mask", 0) == [(10, 20, 40)]
    loose = stretchgen._min_run_after_mask(6)
    assert [r[2:5] for r in stretchgen.stretches_twin(loose, 8, 0)][:2] == [(10, 20, 40), (30, 14, 6)]
    d = aligngen.hashgen.all_distances(loose.a_hashes, loose.b_hashes)
    assert all(d[ka, ka + 30] == 0 for ka in range(14, 40)) and d[13, 43] > 350
    # every cell matches.  3 x 3: the rectangle of the main diagonal is the whole matrix - one record per pair, found in a second round that
    # every pair runs; the larger static videos are tiled until the eighth rank
    assert [r[:2] + r[6:] for r in stretchgen.expected("tolerance_5000", 2)] == [(a, b, 0) for a in range(3) for b in range(3)]
    assert max(r[6] for r in stretchgen.expected("static_self", 0)) == 7
    assert max(r[6] for r in stretchgen.expected("mixed_counts", 2)) >= 1


def test_slow_content_needs_the_guard():
    """slowly changing content: the diagonals beside the true one match too, and what the rectangle of rank 0 leaves of them at its two ends is
    reported at guard 0; the pinned guard is the smallest that leaves the true stretch alone (searched for here, on the twin)"""
    p = stretchgen.case("slow_content_echo")
    counts = [len(stretchgen.stretches_twin(p, 8, g)) for g in range(stretchgen.SLOW_GUARD + 1)]
    print("records per guard:", counts)
    assert counts[0] > 1
    assert counts[stretchgen.SLOW_GUARD] == 1 and all(c > 1 for c in counts[:stretchgen.SLOW_GUARD])
    assert stretchgen.expected("slow_content_echo", stretchgen.SLOW_GUARD) == ((0, 0, 10, 20, 30, 0, 0),)


def test_random_small_problems():
    rng = np.random.default_rng(2025)
    seen = later = 0
    for i in range(300):
        p = aligngen.random_problem(rng)
        max_stretches, guard = (1, 2, 3, 8)[i % 4], (0, 1, 3)[(i // 4) % 3]
        got, found = host(p, max_stretches, guard)
        want = stretchgen.stretches_twin(p, max_stretches, guard)
        assert got == want and found == len(want), (i, max_stretches, guard)
        seen += len(want)
        later += sum(1 for r in want if r[6] > 0)
    assert seen > 400 and later > 100  # the problems are not empty, and not all of rank 0


def test_one_stretch_is_align_windows():
    rng = np.random.default_rng(7)
    for name in sorted(aligngen.CASES):
        got, found = host(aligngen.case(name), 1, 3)
        assert got == [r + (0,) for r in aligngen.expected(name)] and found == len(got)
    for _ in range(50):
        p = aligngen.random_problem(rng)
        assert host(p, 1, 0)[0] == [r + (0,) for r in aligngen.align_twin(p)]


def test_rank_zero_is_align_windows_host():
    from vid_dup_finder_lib_amd import align_windows_host

    for name, guard in stretchgen.CASES:
        p = stretchgen.case(name)
        rec, _ = align_windows_host(p.a_hashes, p.a_first, p.b_hashes, p.b_first, tol_int=p.tol, min_run=p.min_run, a_skip=p.a_skip, b_skip=p.b_skip, capacity=8192)
        got, _ = host(p, 8, guard)
        assert [r[:6] for r in got if r[6] == 0] == aligngen.records(rec)


def test_capacity_smaller_than_the_result():
    p, want = stretchgen.case("self_mode"), list(stretchgen.expected("self_mode", 0))
    assert len(want) > 5
    for capacity in (0, 5, len(want)):
        got, found = host(p, 8, 0, capacity=capacity)
        assert found == len(want) and got == want[:capacity]


def test_argument_checks():
    import vid_dup_finder_lib_amd as vdf

    lib = vdf._capi.load()
    rng = np.random.default_rng(3)
    h = np.ascontiguousarray(aligngen.hashgen.random_hashes(rng, 8))
    first = lambda *v: np.array(v, np.uint32)
    f = first(0, 3, 8)
    out = np.zeros(64, vdf.ALIGN_STRETCH_DTYPE)
    n = C.c_size_t(99)

    def call(ah, af, n_a, min_run, max_stretches, guard, o=out.ctypes.data, n_out=True):
        p = lambda x: None if x is None else x.ctypes.data
        return lib.vdf_align_windows_stretches_host(p(ah), p(af), n_a, None, None, None, 0, None, 350, min_run, max_stretches, guard, o, 64,
                                                    C.byref(n) if n_out else None)

    # every refusal is VDF_E_INVAL; the host form has no context to leave a message in, so which check spoke is seen on the context forms
    # (test_gpu_align_stretches.py reads the messages in their order)
    assert call(None, f, 2, 0, 0, 2**21) == -5
    assert call(h, f, 2, 1, 0, 2**21, n_out=False) == -5
    big = first(0, 2**20 + 1, 2**20 - 5)
    assert call(h, big, 2, 0, 0, 2**21) == -5
    assert call(h, big, 2, 1, 0, 2**21) == -5
    assert call(h, first(0, 5, 3), 2, 1, 0, 2**21) == -5
    for bad in (0, 9, 2**32 - 1):
        assert call(h, f, 2, 1, bad, 2**21) == -5
    assert call(h, f, 2, 1, 8, 2**20 + 1) == -5
    assert call(h, f, 2, 1, 8, 2**20) == 0 and n.value == 0
    assert call(h, f, 2, 1, 1, 0) == 0 and n.value == 0
    n.value = 99
    assert call(h, f, 1, 1, 4, 0) == 0 and n.value == 0  # self mode with one video: nothing to do
    with pytest.raises(vdf.VdfError) as ei:
        vdf.align_windows_stretches_host(h, f, max_stretches=9)
    assert ei.value.code == -5
