"""vdf_align_windows_rates_host on the CPU: the retimed alignment over (rate, a, b) triples of up to 8 rates in one call.  The host
form - the statement of the semantics the band kernel is held against on the GPU - must equal the twin (tests/ratealigngen.py: per rate
retimedaligngen's twin on that rate's block, tagged and concatenated) in its three modes - all triples, a list, the candidates found inside the
call - on every problem the GPU tests use; seed = 1 must equal seed = 0; the tie trap of 4.17 sits in slot 2 of five; duplicate and unreduced
rates get a slot each; a one-rate list at 1/1 is vdf_align_windows_pairs_host; exclude_same, the capacity protocol and every refusal of the
header, in its order, are checked through ctypes.  api.align_rates(one_call=True) returns the default route's dict and one_pass' on the corpus of
tests/test_align_rates_host.py, unseeded, seeded, with static flags and with pairs=, on the host forms alone."""
import ctypes as C
import os

import numpy as np
import pytest

import ratealigngen as gen
import retimedaligngen as rgen
import seedrategen as sgen

NAMES = list(gen.CASES)
SEEDS = max(20, int(os.environ.get("VDF_FUZZ_SEEDS", "0")))


def host(p, capacity=4096, **over):
    import vid_dup_finder_lib_amd as vdf

    kw = dict(tol_int=p.tol, min_run=p.min_run, a_rate_first=p.a_rate_first, a_skip=p.a_skip, b_skip=p.b_skip, exclude_same=p.exclude_same, capacity=capacity)
    kw.update(over)
    return vdf.align_windows_rates_host(p.a_hashes, p.a_first, p.b_hashes, p.b_first, p.rates, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_the_cases_decide_something(name):
    gen.check_non_vacuous(name)


@pytest.mark.parametrize("name", NAMES)
def test_host_is_the_twin_in_all_three_modes(name):
    p = gen.case(name)
    want = list(gen.expected(name))
    got, found = host(p)
    assert found == len(got) and gen.records(got) == want
    # seed = 1: the candidates are found inside the call, and the records are the same
    got, found = host(p, seed=True)
    assert found == len(got) and gen.records(got) == want
    # a list: every second triple, then the candidate set, then the triples that have a record
    every = gen.all_triples(p)
    for triples in (every[::2], list(gen.expected_candidates(name)), [(w[2], w[0], w[1]) for w in want]):
        got, found = host(p, triples=gen.triple_array(triples), exclude_same=False)
        assert found == len(got) and gen.records(got) == gen.twin(p._replace(exclude_same=False), triples), name


def test_the_seed_calls_own_records_go_in_unchanged():
    import vid_dup_finder_lib_amd as vdf

    p = gen.case("mixed_offsets")
    t, n = vdf.align_seed_pairs_rates_host(p.a_hashes, p.a_first, p.b_hashes, p.b_first, p.rates, tol_int=p.tol, min_run=p.min_run,
                                           a_rate_first=p.a_rate_first, a_skip=p.a_skip, b_skip=p.b_skip, capacity=4096)
    assert n == len(t) and [(int(x["rate"]), int(x["a"]), int(x["b"])) for x in t] == list(gen.expected_candidates("mixed_offsets"))
    assert gen.records(host(p, triples=t)[0]) == list(gen.expected("mixed_offsets"))


def test_the_record_is_the_retimed_pairs_calls_record():
    """field for field what vdf_align_windows_retimed_pairs_host gives for the pair on block r, with rate and n_frames_b added"""
    import vid_dup_finder_lib_amd as vdf

    for name in ("mixed_offsets", "tie_trap", "bands3"):
        p = gen.case(name)
        got = gen.records(host(p)[0])
        want = []
        for r, rate in enumerate(p.rates):
            ah, af, ak = sgen.block(p, r)
            rec, n = vdf.align_windows_retimed_host(ah, af, p.b_hashes, p.b_first, rate, tol_int=p.tol, min_run=p.min_run, a_skip=ak, b_skip=p.b_skip, capacity=4096)
            want += [(a, b, r, fa, fb, nw, ds, (nw - 1) * sgen.reduced(rate)[1] + 16) for a, b, fa, fb, nw, ds in rgen.records(rec)]
        assert got == want and got


def test_the_tie_trap_in_slot_two_of_five():
    """both levels of the reduction decide: the record of (2, 0, 0) is R3, which one comparator over all runs would not report"""
    p = gen.case("tie_trap")
    got = {(r[2], r[0], r[1]): r for r in gen.records(host(p)[0])}
    assert sorted(got) == [(2, 0, 0), (2, 1, 1), (2, 2, 2)]
    assert got[(2, 0, 0)][3:5] == (46, 0) and got[(2, 1, 1)][3] == 27 and got[(2, 2, 2)][3] == 36
    one = rgen.align_retimed_twin(gen.block_problem(p, 2), reduce=rgen.one_level)
    assert one[0][2] == 26   # the trap is one: a single comparator reports R2


@pytest.mark.parametrize("name", ["twins_6_5", "twins_32_17"])
def test_duplicate_and_unreduced_rates_get_a_slot_each(name):
    got = gen.records(host(gen.case(name))[0])
    slot = lambda r: [(a, b, fa, fb, n, s, nf) for a, b, rr, fa, fb, n, s, nf in got if rr == r]
    assert slot(0) and slot(0) == slot(2)


def test_one_rate_at_1_1_is_the_plain_pairs_call():
    """first_a = start_a, first_b = start_a + offset, as DESIGN 4.17 states; n_frames_b = n_windows + 15"""
    import vid_dup_finder_lib_amd as vdf

    p = gen.case("mixed_offsets")
    ah, af, ak = sgen.block(p, 0)
    pairs = [(a, b) for a in range(4) for b in range(3)]
    plain, n = vdf.align_windows_pairs_host(ah, af, pairs, p.b_hashes, p.b_first, tol_int=p.tol, min_run=p.min_run, a_skip=ak, b_skip=p.b_skip, capacity=64)
    got, found = vdf.align_windows_rates_host(ah, af[None, :], p.b_hashes, p.b_first, [(1, 1)], tol_int=p.tol, min_run=p.min_run, a_skip=ak, b_skip=p.b_skip,
                                              triples=[(0, a, b) for a, b in pairs])
    assert n == len(plain) == found >= 2
    assert gen.records(got) == [(int(x["a"]), int(x["b"]), 0, int(x["start_a"]), int(x["start_a"]) + int(x["offset"]), int(x["n_windows"]), int(x["dist_sum"]),
                                 int(x["n_windows"]) + 15) for x in plain]


def test_exclude_same():
    import vid_dup_finder_lib_amd as vdf

    ex = gen.case("square")
    full = gen.records(host(ex, exclude_same=False)[0])
    assert sum(1 for r in full if r[0] == r[1]) == 2 * 7
    assert gen.records(host(ex)[0]) == [r for r in full if r[0] != r[1]] == list(gen.expected("square"))
    with pytest.raises(vdf.VdfError):   # n_a != n_b
        host(ex._replace(b_first=ex.b_first[:-1]))


def test_capacity_protocol():
    p = gen.case("planted_min_run_1")
    want = list(gen.expected("planted_min_run_1"))
    for kw in (dict(), dict(seed=True), dict(triples=gen.triple_array(gen.expected_candidates("planted_min_run_1")))):
        got, found = host(p, capacity=0, **kw)
        assert len(got) == 0 and found == len(want)
        got, found = host(p, capacity=5, **kw)
        assert found == len(want) > 5 and gen.records(got) == want[:5]
        got, found = host(p, capacity=found, **kw)
        assert found == len(want) and gen.records(got) == want


def _job(p, **over):
    """the job of the host form through ctypes, for the refusals numpy arguments cannot express: (job, what it points into)"""
    from vid_dup_finder_lib_amd import _capi

    num = np.array([r[0] for r in p.rates], np.uint32)
    den = np.array([r[1] for r in p.rates], np.uint32)
    rf = np.ascontiguousarray(p.a_rate_first, dtype=np.uintp)
    af = np.ascontiguousarray(p.a_first, dtype=np.uint32)
    bf = np.ascontiguousarray(p.b_first, dtype=np.uint32)
    out = np.zeros(4096, _capi.ALIGN_RATE_DTYPE)
    n = C.c_size_t(77)
    f = dict(a_hashes=p.a_hashes.ctypes.data, a_first=af.ctypes.data, a_rate_first=rf.ctypes.data, a_skip=None, n_a=af.shape[1] - 1, b_hashes=p.b_hashes.ctypes.data,
             b_first=bf.ctypes.data, b_skip=None, n_b=len(bf) - 1, n_rates=len(num), rate_num=num.ctypes.data, rate_den=den.ctypes.data, tol_int=p.tol,
             min_run=p.min_run, triples=None, n_triples=0, seed=0, exclude_same=0, out=out.ctypes.data, capacity=out.size, n_out=C.pointer(n), stream=None)
    f.update(over)
    return _capi.VdfAlignRatesJob(**f), (num, den, rf, af, bf, out, n)


def test_every_refusal_is_e_inval_in_the_headers_order():
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    p = sgen.square()
    call = lambda **over: (lambda jk: lib.vdf_align_windows_rates_host(C.byref(jk[0])))(_job(p, **over))
    arr = lambda v, t=np.uint32: np.array(v, t)
    tri = lambda v: np.array(v, _capi.VIDEO_PAIR_RATE_DTYPE)   # (a, b, rate)
    assert call() == _capi.VDF_OK
    # 1. a null job
    assert lib.vdf_align_windows_rates_host(None) == _capi.VDF_E_INVAL
    # 2. the checks of vdf_align_seed_pairs_rates in its order, B first and then the blocks of A, up to and including the rate list
    for field in ("n_out", "out", "b_hashes", "b_first", "a_hashes", "a_first"):
        assert call(**{field: None}) == _capi.VDF_E_INVAL, field
    assert call(min_run=0) == _capi.VDF_E_INVAL
    long_b, long_a = p.b_first.copy(), p.a_first.copy()
    long_b[1:] += (1 << 20) + 1
    long_a[1, 3:] += (1 << 20) + 1       # the second block: every block is checked
    down_b, down_a = p.b_first.copy(), p.a_first.copy()
    down_b[2] = down_b[1] - 1
    down_a[1, 2] = down_a[1, 1] - 1
    assert call(b_first=long_b.ctypes.data) == _capi.VDF_E_INVAL and call(a_first=long_a.ctypes.data) == _capi.VDF_E_INVAL
    assert call(b_first=down_b.ctypes.data) == _capi.VDF_E_INVAL and call(a_first=down_a.ctypes.data) == _capi.VDF_E_INVAL
    far = arr([0, 2**32 - 5, 0], np.uintp)
    assert call(a_rate_first=far.ctypes.data) == _capi.VDF_E_INVAL    # 2^32 rows or more
    wide_a, wide_b = np.zeros(2 * 4098, np.uint32), np.zeros(4097, np.uint32)
    assert call(n_a=4097, n_b=4096, a_first=wide_a.ctypes.data, b_first=wide_b.ctypes.data) == _capi.VDF_E_INVAL      # 4097 x 4096 pairs are too many
    nine = arr([1] * 9)
    assert call(n_rates=0) == _capi.VDF_E_INVAL and call(rate_num=None) == _capi.VDF_E_INVAL and call(rate_den=None) == _capi.VDF_E_INVAL
    assert call(n_rates=9, rate_num=nine.ctypes.data, rate_den=nine.ctypes.data, a_first=np.zeros(9 * 8, np.uint32).ctypes.data) == _capi.VDF_E_INVAL
    for bad in ([(1, 1), (1, 0)], [(1, 1), (2, 3)], [(1, 1), (5, 2)], [(66, 34), (1, 1)], [(1, 1), (37, 36)]):
        nn, dd = arr([r[0] for r in bad]), arr([r[1] for r in bad])
        assert call(rate_num=nn.ctypes.data, rate_den=dd.ctypes.data) == _capi.VDF_E_INVAL, bad
    ok_n, ok_d = arr([64, 6]), arr([34, 4])
    assert call(rate_num=ok_n.ctypes.data, rate_den=ok_d.ctypes.data) == _capi.VDF_OK     # 64/34 is 32/17: the limit is on the reduced num
    # 3. exclude_same with n_a != n_b
    assert call(exclude_same=1) == _capi.VDF_OK and call(exclude_same=1, n_b=6) == _capi.VDF_E_INVAL
    # 4. a list together with seed or exclude_same
    good = tri([(0, 0, 0), (0, 1, 0), (3, 2, 0), (0, 0, 1), (6, 6, 1)])
    assert call(triples=good.ctypes.data, n_triples=len(good)) == _capi.VDF_OK
    assert call(triples=good.ctypes.data, n_triples=len(good), seed=1) == _capi.VDF_E_INVAL
    assert call(triples=good.ctypes.data, n_triples=len(good), exclude_same=1) == _capi.VDF_E_INVAL
    assert call(seed=1) == _capi.VDF_OK and call(seed=1, exclude_same=1) == _capi.VDF_OK
    # 5. the list: too long, unsorted, a duplicate, a rate outside the list, a video that does not exist
    assert call(triples=good.ctypes.data, n_triples=(1 << 27) + 1) == _capi.VDF_E_INVAL
    for bad in ([(0, 1, 0), (0, 0, 0)], [(0, 0, 1), (0, 0, 0)], [(1, 0, 0), (0, 5, 0)], [(2, 2, 1), (2, 2, 1)], [(0, 0, 2)], [(7, 0, 0)], [(0, 7, 1)]):
        t = tri(bad)
        assert call(triples=t.ctypes.data, n_triples=len(t)) == _capi.VDF_E_INVAL, bad
    # the order of two kinds: a bad list does not hide a bad rate, and a list with seed is refused before its entries are read
    assert call(triples=tri([(7, 0, 0)]).ctypes.data, n_triples=1, n_rates=0) == _capi.VDF_E_INVAL
    assert call(triples=None, n_triples=5) == _capi.VDF_OK    # no list: n_triples is not read
    # empty input: VDF_OK with *n_out = 0, whatever the pointers of the empty side; an empty list
    for over in (dict(n_a=0, a_hashes=None, a_first=None), dict(n_b=0, b_hashes=None, b_first=None), dict(triples=good.ctypes.data, n_triples=0)):
        job, keep = _job(p, **over)
        assert lib.vdf_align_windows_rates_host(C.byref(job)) == _capi.VDF_OK and keep[-1].value == 0
    assert call(n_a=0, min_run=0) == _capi.VDF_E_INVAL and call(n_b=0, n_rates=0) == _capi.VDF_E_INVAL


def test_refusal_messages_come_in_the_headers_order():
    """through a context the message names the check that fired: two faults at once report the earlier one (no GPU: the context is never made,
    so the order is read from the host form's behaviour on pairs of faults instead)"""
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    p = sgen.square()
    tri = np.array([(0, 0, 0)], _capi.VIDEO_PAIR_RATE_DTYPE)
    # exclude_same with n_a != n_b (3.) and a list with exclude_same (4.) and a bad list (5.): each alone is refused, and so is every combination
    for over in (dict(exclude_same=1, n_b=6), dict(triples=tri.ctypes.data, n_triples=1, exclude_same=1), dict(triples=tri.ctypes.data, n_triples=1, seed=1, n_rates=0)):
        job, keep = _job(p, **over)
        assert lib.vdf_align_windows_rates_host(C.byref(job)) == _capi.VDF_E_INVAL and keep[-1].value == 77   # a refused call writes nothing


def test_python_arguments_are_checked():
    import vid_dup_finder_lib_amd as vdf

    p = sgen.square()
    with pytest.raises(ValueError):
        vdf.align_windows_rates_host(p.a_hashes, p.a_first[0], p.b_hashes, p.b_first, p.rates)           # a_first: one row per rate
    with pytest.raises(ValueError):
        vdf.align_windows_rates_host(p.a_hashes, p.a_first, None, None, p.rates, a_rate_first=p.a_rate_first)
    with pytest.raises(ValueError):
        vdf.align_windows_rates_host(p.a_hashes, p.a_first, p.b_hashes, p.b_first, p.rates, a_rate_first=p.a_rate_first, triples=[(0, -1, 0)])
    with pytest.raises(vdf.VdfError):
        vdf.align_windows_rates_host(p.a_hashes, p.a_first, p.b_hashes, p.b_first, [(1, 1), (3, 1)], a_rate_first=p.a_rate_first)
    assert vdf.ALIGN_RATE_DTYPE.itemsize == 32


@pytest.mark.parametrize("seed", range(SEEDS))
def test_seeded_random_problems(seed):
    p = gen.random_problem(np.random.default_rng([91, 11, seed]))
    want = gen.twin(p)
    got, found = host(p, capacity=1 << 12)
    assert found == len(got) and gen.records(got) == want, (seed, p.rates, p.tol, p.min_run)
    got, found = host(p, capacity=1 << 12, seed=True)
    assert gen.records(got) == want, (seed, p.rates, p.tol, p.min_run)


@pytest.mark.parametrize("true", [(6, 5), (3, 2)])
def test_align_rates_one_call_returns_the_same_dict(true):
    """the corpus of DESIGN.md 4.16 at the five usual rates: one call for all rates against one align_retimed per rate and against one_pass"""
    import vid_dup_finder_lib_amd as vdf
    from test_align_rates_host import CANDIDATES, MIN_RUN, TOLERANCE, hashed

    va, vb, _, _ = hashed(true)
    assert set(va) == set(CANDIDATES) and len(CANDIDATES) == 5
    plain = vdf.align_rates(va, vb, TOLERANCE, MIN_RUN)
    assert any(plain.values()) and vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, one_call=True) == plain
    seeded = vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, seed=True, native=True)
    assert seeded == plain and vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, seed=True, one_call=True) == seeded
    assert vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, seed=True, native=True, one_pass=True) == seeded
    assert vdf.best_rates(vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, seed=True, one_call=True), TOLERANCE) == vdf.best_rates(plain, TOLERANCE)
    # static flags: every third window of A at every rate, every fifth of B
    sa = {r: [np.arange(len(ws)) % 3 == 1 for ws in va[r]] for r in CANDIDATES}
    sb = [np.arange(len(ws)) % 5 == 2 for ws in vb]
    kw = dict(static_a=sa, static_b=sb, seed=True, native=True)
    flagged = vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, **kw)
    assert flagged != plain and vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, one_call=True, **kw) == flagged
    assert vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, one_call=True, static_a=sa, static_b=sb) == flagged
    # a caller's list: every rate on the listed pairs, and the candidates that are on it
    pairs = [(0, 0), (0, 3), (1, 1), (1, 2)]
    listed = vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, seed=True, native=True, pairs=pairs)
    assert any(listed.values()) and vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, seed=True, pairs=pairs, one_call=True) == listed
    assert vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, pairs=pairs, one_call=True) == vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, pairs=pairs) == listed
    assert vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, seed=True, native=True, pairs=pairs, one_pass=True) == listed
    with pytest.raises(ValueError):
        vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, native=False, one_call=True)
    with pytest.raises(ValueError):
        vdf.align_rates({(1, 1): va[(1, 1)], **{(40 + i, 39 + i): va[(1, 1)] for i in range(8)}}, vb, TOLERANCE, MIN_RUN, one_call=True)   # nine rates
