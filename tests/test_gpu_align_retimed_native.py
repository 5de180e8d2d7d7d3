"""vdf_align_windows_retimed[_device] and their _pairs forms (csrc/align.hip: align_bands_kernel<AlignPairUnits<true>, false> and the two-level reduction)
against the numpy twin of tests/retimedaligngen.py, records equal field for field and `found` equal: the device form on device arrays of exactly their
size and the host-array form, on every problem tests/test_align_retimed_native_host.py gives the plain C++ definition - sub-matrices of 67 x 65 cells
in three bands with the reload wrap, phases with p >= Na and empty videos, planted lines at the four matrix edges, on the two sides of a band
boundary and split by one miss, distances on the tolerance and one over, min_run on and one above a run's length, the tie trap of the two-level
reduction, the rates 1/1 ... 32/17, skip bytes behind first values that are no multiples of 4, dense matches - then the buffer protocol, pair lists,
and hash_frame_windows(rate=) -> align_retimed(native=True) end to end."""
import numpy as np
import pytest

import retimedaligngen as rg
import retimedgen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import vid_dup_finder_lib_amd as vdf

    e = vdf.Engine(0)
    yield e
    e.close()


def _dev(x, dtype):
    import torch

    return None if x is None else torch.from_numpy(np.ascontiguousarray(x).view(dtype).copy()).cuda()


def device_form(eng, p, capacity=4096, pairs=None):
    """the problem's arrays as device arrays of exactly their size -> (records, found)"""
    import torch

    ah, af, ak = _dev(p.a_hashes, np.int64), _dev(p.a_first, np.int32), _dev(p.a_skip, np.uint8)
    bh, bf, bk = _dev(p.b_hashes, np.int64), _dev(p.b_first, np.int32), _dev(p.b_skip, np.uint8)
    torch.cuda.synchronize()
    ptr = lambda t: 0 if t is None else t.data_ptr()
    kw = dict(tol_int=p.tol, min_run=p.min_run, d_a_skip=ptr(ak), d_b_skip=ptr(bk), capacity=capacity)
    if pairs is not None:
        rec, found = eng.align_windows_retimed_pairs_device(ptr(ah), ptr(af), len(p.a_first) - 1, pairs, ptr(bh), ptr(bf), len(p.b_first) - 1, p.rate, **kw)
    else:
        rec, found = eng.align_windows_retimed_device(ptr(ah), ptr(af), len(p.a_first) - 1, ptr(bh), ptr(bf), len(p.b_first) - 1, p.rate, **kw)
    return rg.records(rec), found


def host_array_form(eng, p, capacity=4096, pairs=None):
    kw = dict(tol_int=p.tol, min_run=p.min_run, a_skip=p.a_skip, b_skip=p.b_skip, capacity=capacity)
    if pairs is not None:
        rec, found = eng.align_windows_retimed_pairs(p.a_hashes, p.a_first, pairs, p.b_hashes, p.b_first, p.rate, **kw)
    else:
        rec, found = eng.align_windows_retimed(p.a_hashes, p.a_first, p.b_hashes, p.b_first, p.rate, **kw)
    return rg.records(rec), found


@pytest.mark.parametrize("name", sorted(rg.CASES))
def test_kernel_matches_the_twin(eng, name):
    p, want = rg.case(name), list(rg.expected(name))
    got, found = device_form(eng, p)
    print(f"{name}: {len(want)} records, device form found {found}")
    assert found == len(want)
    assert got == want
    got, found = host_array_form(eng, p)
    assert found == len(want) and got == want


def test_the_tie_trap_needs_both_levels(eng):
    """on this input ONE comparator on (score, first_a, first_b) over all runs of all phases would pick another run than the two-level rule"""
    p = rg.case("tie_trap")
    two, one = rg.align_retimed_twin(p), rg.align_retimed_twin(p, reduce=rg.one_level)
    assert two[0] == (0, 0, 46, 0, 4, 0) and one[0] == (0, 0, 26, 55, 4, 0) and one != two
    assert device_form(eng, p) == (two, 3)


def test_dense_matches_give_one_record_per_pair(eng):
    """every cell of every phase matches: 4 x 3 pairs of up to 200 x 129 windows, and still 12 records.  200 x 129 windows at 3 / 2: 67, 67 and 66
    rows against 65 columns, so every phase has a run of 65 - level 1 keeps the smallest offset (-2, -2, -1: i0 2, 2, 1), level 2 the smallest
    first_a: 6, 7, 5 - phase 2's.  200 x 200: only phases 0 and 1 have 67 rows, both from the corner: phase 0's."""
    p, want = rg.case("dense_3_2"), list(rg.expected("dense_3_2"))
    assert len(want) == 12 and want[0] == (0, 0, 5, 0, 65, 0) and want[1] == (0, 1, 0, 0, 67, 0) and want[11] == (3, 2, 0, 0, 1, 0)
    assert device_form(eng, p) == (want, 12)


def test_capacity_smaller_than_the_result(eng):
    p, want = rg.case("band_boundaries"), list(rg.expected("band_boundaries"))
    assert len(want) > 5
    for form in (device_form, host_array_form):
        got, found = form(eng, p, capacity=5)
        assert found == len(want) and got == want[:5]  # the count is right and the prefix is valid
        got, found = form(eng, p, capacity=0)
        assert found == len(want) and got == []
        got, found = form(eng, p, capacity=found)      # the second call is complete
        assert found == len(want) and got == want


def test_pair_lists(eng):
    p, want = rg.case("band_boundaries"), list(rg.expected("band_boundaries"))
    pairs = [(0, 3), (1, 1), (3, 0), (3, 4), (4, 3), (5, 4)]  # (0, 3) and (3, 0) name a video of 0 windows
    listed = rg.align_retimed_twin(p, pairs=pairs)
    assert listed == [r for r in want if r[:2] in pairs] and len(listed) >= 3
    for form in (device_form, host_array_form):
        assert form(eng, p, pairs=pairs) == (listed, len(listed))
        assert form(eng, p, pairs=pairs, capacity=1) == (listed[:1], len(listed))
        assert form(eng, p, pairs=[(0, 3), (3, 0)]) == ([], 0)          # only pairs with an empty video: nothing is launched
        assert form(eng, p, pairs=np.zeros((0, 2), np.int64)) == ([], 0)
    q = rg.case("skip_cuts")
    assert device_form(eng, q, pairs=[(1, 2)]) == ([r for r in rg.expected("skip_cuts") if r[:2] == (1, 2)], 1)


@pytest.mark.parametrize("rate,seed", [((6, 5), 65), ((2, 1), 21)])
def test_end_to_end_retimed_windows_to_native_alignment(eng, rate, seed):
    import vid_dup_finder_lib_amd as vdf

    A, B = retimedgen.corpus(rate, seed)
    va = vdf.hash_frame_windows(A, [f"a{i}" for i in range(len(A))], [len(v) for v in A], stride=1, rate=rate, engine=eng)
    vb = vdf.hash_frame_windows(B, [f"b{i}" for i in range(len(B))], [len(v) for v in B], stride=1, engine=eng)
    for min_run in (1, 2):
        want = vdf.align_retimed(va, vb, rate, 0.35, min_run=min_run, engine=eng)
        assert vdf.align_retimed(va, vb, rate, 0.35, min_run=min_run, engine=eng, native=True) == want
        assert vdf.align_retimed(va, vb, rate, 0.35, min_run=min_run, engine=eng, native=True, seed=True) == want
    exact = {(r.a, r.b): r for r in vdf.align_retimed(va, vb, rate, 0.0, min_run=2, engine=eng, native=True)}
    assert sorted(exact) == sorted(retimedgen.EXCERPTS)
    for (a, b), (c, fb0, nb) in retimedgen.EXCERPTS.items():
        r = exact[(a, b)]
        assert r.mean_distance == 0 and (r.first_frame_a, r.first_frame_b, r.n_windows) == (c, fb0, (nb - 16) // rate[1] + 1), (rate, a, b, r)
        assert (r.num, r.den, r.path_a, r.path_b) == (rate[0], rate[1], f"a{a}", f"b{b}")


def test_argument_checks_and_a_multi_gpu_context(eng):
    import vid_dup_finder_lib_amd as vdf

    p = rg.case("rate_6_5")
    for bad in ((6, 0), (4, 5), (11, 5), (33, 32)):
        with pytest.raises(vdf.VdfError) as ei:
            eng.align_windows_retimed(p.a_hashes, p.a_first, p.b_hashes, p.b_first, bad)
        assert ei.value.code == -5 and ("den <= num" in str(ei.value) or "above 32" in str(ei.value))
    assert host_array_form(eng, p._replace(rate=(64, 34)))[1] == len(rg.align_retimed_twin(p._replace(rate=(32, 17))))
    with pytest.raises(vdf.VdfError) as ei:
        eng.align_windows_retimed(p.a_hashes, p.a_first, p.b_hashes, p.b_first, (6, 5), min_run=0)
    assert "min_run" in str(ei.value)                                   # the align checks come first
    with pytest.raises(vdf.VdfError) as ei:
        eng.align_windows_retimed_pairs(p.a_hashes, p.a_first, [(0, 1), (0, 0)], p.b_hashes, p.b_first, (6, 0))
    assert "den <= num" in str(ei.value)                                # the rate before the list
    with pytest.raises(vdf.VdfError) as ei:
        eng.align_windows_retimed_pairs(p.a_hashes, p.a_first, [(0, 1), (0, 0)], p.b_hashes, p.b_first, (6, 5))
    assert "strictly increasing" in str(ei.value)
    multi = vdf.Engine(devices=[0, 0])
    try:
        with pytest.raises(vdf.VdfError) as ei:
            multi.align_windows_retimed(p.a_hashes, p.a_first, p.b_hashes, p.b_first, (6, 0))
        assert "den <= num" in str(ei.value)                            # a multi-GPU context: the last check
        with pytest.raises(vdf.VdfError) as ei:
            multi.align_windows_retimed(p.a_hashes, p.a_first, p.b_hashes, p.b_first, (6, 5))
        assert ei.value.code == -5 and "single-device" in str(ei.value)
    finally:
        multi.close()
