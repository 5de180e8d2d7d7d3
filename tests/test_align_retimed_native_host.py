"""vdf_align_windows_retimed_host / _pairs_host (csrc/api.cpp: the definition of DESIGN.md 4.17 in plain C++, no GPU) against the numpy twin of
tests/retimedaligngen.py, records equal field for field, on every problem tests/test_gpu_align_retimed_native.py gives the kernel: band boundaries
and the reload wrap at 3 / 2, planted lines at every matrix edge, across a band boundary and split by one miss, tolerances on and one over, min_run
on and one above a run's length, the tie trap of the two-level reduction, the rates up to num = 32, skip bytes, dense matches.  The twin itself is
held against the brute-force twin of the composition (tests/retimedgen.py) where no skip bytes are set; api.align_retimed(native=True) against
native=False; rate 1 / 1 against vdf_align_windows_host; and the argument checks return their codes."""
import ctypes as C

import numpy as np
import pytest

import aligngen
import retimedaligngen as rg
import retimedgen
from test_align_retimed_host import SEED, hashed


def host_form(p, capacity=4096, pairs=None):
    import vid_dup_finder_lib_amd as vdf

    kw = dict(tol_int=p.tol, min_run=p.min_run, a_skip=p.a_skip, b_skip=p.b_skip, capacity=capacity)
    if pairs is not None:
        rec, found = vdf.align_windows_retimed_pairs_host(p.a_hashes, p.a_first, pairs, p.b_hashes, p.b_first, p.rate, **kw)
    else:
        rec, found = vdf.align_windows_retimed_host(p.a_hashes, p.a_first, p.b_hashes, p.b_first, p.rate, **kw)
    assert rec.dtype == vdf.ALIGN_RETIMED_DTYPE and rec.dtype.itemsize == 24
    return rg.records(rec), found


@pytest.mark.parametrize("name", sorted(rg.CASES))
def test_host_definition_matches_the_twin(name):
    p, want = rg.case(name), list(rg.expected(name))
    got, found = host_form(p)
    print(f"{name}: {len(want)} records")
    assert found == len(want) and got == want


@pytest.mark.parametrize("name", [n for n in sorted(rg.CASES) if not n.startswith("skip")])
def test_the_twin_is_the_composition_s_brute_force_twin_where_nothing_is_skipped(name):
    p = rg.case(name)
    split = lambda h, f: [h[int(f[v]):int(f[v + 1])] for v in range(len(f) - 1)]
    want = retimedgen.align_retimed_twin(split(p.a_hashes, p.a_first), split(p.b_hashes, p.b_first), p.rate, p.tol, p.min_run)
    assert [(a, b, fa, fb, n, round(mean * n)) for a, b, _, _, fa, fb, _, _, n, mean in want] == list(rg.expected(name))


def test_the_tie_trap_needs_both_levels():
    """on this input ONE comparator on (score, first_a, first_b) over all runs of all phases picks another run than the two-level rule"""
    p = rg.case("tie_trap")
    two, one = rg.align_retimed_twin(p), rg.align_retimed_twin(p, reduce=rg.one_level)
    assert two == [(0, 0, 46, 0, 4, 0), (1, 1, 27, 45, 4, 0), (2, 2, 36, 5, 4, 0)]
    assert one[0] == (0, 0, 26, 55, 4, 0) and one[1:] == two[1:]
    assert host_form(p)[0] == two


def test_planted_lines_are_found_where_they_were_planted():
    want = {m: {r[:2]: r[2:] for r in rg.expected(f"planted_min_run_{m}")} for m in (1, 5, 6)}
    assert sorted(want[1]) == [(i, i) for i in range(8)] and sorted(want[5]) == [(i, i) for i in (0, 1, 2, 3, 4, 6, 7)] and sorted(want[6]) == [(i, i) for i in (1, 2, 3, 7)]
    assert want[1][(2, 2)][:3] == (0 + 3 * 45, 2 * 43, 7) and want[1][(3, 3)][:3] == (1 + 3 * 30, 2 * 27, 7)   # the better of two runs on the two sides of a band boundary
    assert want[1][(4, 4)][:3] == (2 + 3 * 10, 2 * 20, 5)                                                    # the first of two equal runs on one line
    assert want[1][(5, 5)] == (0 + 3 * 8, 2 * 9, 1, 350)                                                      # exactly on the tolerance; the cell one over is no run
    assert want[1][(7, 7)][:3] == (0, 0, 65)


def test_pair_lists_and_capacity():
    p, want = rg.case("band_boundaries"), list(rg.expected("band_boundaries"))
    assert len(want) > 5
    for cap in (0, 5, len(want)):
        got, found = host_form(p, capacity=cap)
        assert found == len(want) and got == want[:cap]
    pairs = [(0, 3), (1, 1), (3, 0), (3, 4), (4, 3), (5, 4)]  # (0, 3) and (3, 0) name a video of 0 windows
    got, found = host_form(p, pairs=pairs)
    assert got == rg.align_retimed_twin(p, pairs=pairs) == [r for r in want if r[:2] in pairs] and found == len(got) >= 3
    assert host_form(p, pairs=np.zeros((0, 2), np.int64)) == ([], 0)


def test_rate_one_is_the_plain_alignment():
    import vid_dup_finder_lib_amd as vdf

    for name in ("mixed_counts", "reload_wrap", "tie_two_diagonals", "skip_cuts", "static_a_shorter"):
        q = aligngen.case(name)
        plain, n_plain = vdf.align_windows_host(q.a_hashes, q.a_first, q.b_hashes, q.b_first, tol_int=q.tol, min_run=q.min_run, a_skip=q.a_skip, b_skip=q.b_skip,
                                                capacity=4096)
        got, found = host_form(rg.Problem(q.a_hashes, q.a_first, q.b_hashes, q.b_first, (1, 1), q.tol, q.min_run, q.a_skip, q.b_skip))
        assert found == n_plain > 0
        assert got == [(int(r["a"]), int(r["b"]), int(r["start_a"]), int(r["start_a"]) + int(r["offset"]), int(r["n_windows"]), int(r["dist_sum"])) for r in plain]


def _video_hashes(hashes, first, tag):
    import vid_dup_finder_lib_amd as vdf

    return [[vdf.VideoHash(w, f"{tag}{v}", 10 + v) for w in hashes[int(first[v]):int(first[v + 1])]] for v in range(len(first) - 1)]


def _static(skip, first):
    return None if skip is None else [skip[int(first[v]):int(first[v + 1])] for v in range(len(first) - 1)]


@pytest.mark.parametrize("name", ["band_boundaries", "planted_min_run_5", "tie_trap", "rate_32_17", "rate_31_16_noise", "skip_cuts", "skip_noise", "dense_6_5"])
def test_api_native_equals_the_composition_on_the_cases(name, monkeypatch):
    import vid_dup_finder_lib_amd as vdf

    monkeypatch.setattr(vdf.api, "ALIGN_HOST_CELLS", 1 << 40)  # the host forms, whatever the size
    p = rg.case(name)
    va, vb = _video_hashes(p.a_hashes, p.a_first, "a"), _video_hashes(p.b_hashes, p.b_first, "b")
    kw = dict(tolerance=p.tol / 1000.0, min_run=p.min_run, static_a=_static(p.a_skip, p.a_first), static_b=_static(p.b_skip, p.b_first))
    assert vdf.engine.tolerance_int(kw["tolerance"]) == p.tol
    want = vdf.align_retimed(va, vb, p.rate, **kw)
    assert [(r.a, r.b, r.first_frame_a, r.first_frame_b, r.n_windows, round(r.mean_distance * r.n_windows)) for r in want] == list(rg.expected(name))
    assert vdf.align_retimed(va, vb, p.rate, native=True, **kw) == want
    assert vdf.align_retimed(va, vb, p.rate, native=True, seed=True, **kw) == want
    some = [(r.a, r.b) for r in want][::2]
    assert vdf.align_retimed(va, vb, p.rate, native=True, pairs=some, **kw) == [r for r in want if (r.a, r.b) in some] == vdf.align_retimed(va, vb, p.rate, pairs=some, **kw)


@pytest.mark.parametrize("rate", sorted(SEED))
def test_api_native_equals_the_composition_on_the_corpus(rate):
    import vid_dup_finder_lib_amd as vdf

    va, vb, _, _, _ = hashed(rate)
    sa = [np.zeros(len(w), np.uint8) for w in va]
    sb = [np.zeros(len(w), np.uint8) for w in vb]
    sb[0][4] = 1
    sa[1][9] = 1
    for tolerance, min_run in ((0.35, 1), (0.35, 2), (0.0, 2)):
        for static in (dict(), dict(static_a=sa, static_b=sb)):
            want = vdf.align_retimed(va, vb, rate, tolerance, min_run=min_run, **static)
            assert want and vdf.align_retimed(va, vb, rate, tolerance, min_run=min_run, native=True, **static) == want
            assert vdf.align_retimed(va, vb, rate, tolerance, min_run=min_run, native=True, seed=True, **static) == want
    assert vdf.align_retimed(va, vb, (2 * rate[0], 2 * rate[1]), 0.35, native=True) == vdf.align_retimed(va, vb, rate, 0.35)
    assert vdf.align_retimed([], vb, rate, 0.35, native=True) == [] and vdf.align_retimed(va, [], rate, 0.35, native=True) == []


def test_argument_checks_return_their_codes():
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    p = rg.case("rate_6_5")
    out = np.zeros(16, vdf.ALIGN_RETIMED_DTYPE)
    n = C.c_size_t(99)
    pairs = vdf.engine.video_pairs([(0, 0), (0, 1)])

    def call(num, den, min_run=1, a_first=p.a_first, listed=False, n_out=True):
        sides = [p.a_hashes.ctypes.data, a_first.ctypes.data, len(a_first) - 1, None, p.b_hashes.ctypes.data, p.b_first.ctypes.data, len(p.b_first) - 1, None]
        tail = [350, min_run, num, den, out.ctypes.data, out.size, C.byref(n) if n_out else None]
        if listed:
            return lib.vdf_align_windows_retimed_pairs_host(*sides, pairs.ctypes.data, pairs.size, *tail)
        return lib.vdf_align_windows_retimed_host(*sides, *tail)

    assert _capi.ALIGN_RETIMED_MAX_NUM == vdf.api.ALIGN_RETIMED_MAX_NUM == 32
    for listed in (False, True):
        assert call(6, 5, listed=listed) == _capi.VDF_OK and n.value == len(rg.expected("rate_6_5"))
        for num, den in ((6, 0), (0, 0), (4, 5), (11, 5), (33, 32), (33, 17), (2**32 - 1, 2**31)):  # den = 0; num < den; num > 2 den; reduced num = 33 (and above)
            assert call(num, den, listed=listed) == _capi.VDF_E_INVAL, (num, den)
        n.value = 99
        assert call(64, 34, listed=listed) == _capi.VDF_OK  # reduces to 32 / 17
        assert call(12, 10, listed=listed) == _capi.VDF_OK and n.value == len(rg.expected("rate_6_5"))
        # vdf_align_windows' own checks come first and keep their codes
        assert call(0, 0, min_run=0, listed=listed) == _capi.VDF_E_INVAL and call(6, 5, n_out=False, listed=listed) == _capi.VDF_E_INVAL
        assert call(6, 5, a_first=np.array([0, 70, 60], np.uint32), listed=listed) == _capi.VDF_E_INVAL
    # no self mode: B missing is a null pointer
    assert lib.vdf_align_windows_retimed_host(p.a_hashes.ctypes.data, p.a_first.ctypes.data, 2, None, None, p.b_first.ctypes.data, 2, None, 350, 1, 6, 5,
                                              out.ctypes.data, out.size, C.byref(n)) == _capi.VDF_E_INVAL
    bad = vdf.engine.video_pairs([(0, 1), (0, 0)])
    assert lib.vdf_align_windows_retimed_pairs_host(p.a_hashes.ctypes.data, p.a_first.ctypes.data, 2, None, p.b_hashes.ctypes.data, p.b_first.ctypes.data, 2, None,
                                                    bad.ctypes.data, 2, 350, 1, 6, 5, out.ctypes.data, out.size, C.byref(n)) == _capi.VDF_E_INVAL
    with pytest.raises(vdf.VdfError) as ei:
        vdf.align_windows_retimed_pairs_host(p.a_hashes, p.a_first, [(0, 1), (0, 0)], p.b_hashes, p.b_first, (6, 5))
    assert ei.value.code == _capi.VDF_E_INVAL and "strictly increasing" in str(ei.value)
    with pytest.raises(ValueError):
        vdf.align_windows_retimed_host(p.a_hashes, p.a_first, None, None, (6, 5))
    for badrate in ((33, 32), (1, 2), (3, 0)):
        with pytest.raises(ValueError):
            vdf.align_retimed([], [], badrate, 0.35, native=True)
