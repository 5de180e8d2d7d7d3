"""vdf_align_seed_pairs_rates_host on the CPU: the candidates of the retimed alignment, every phase of up to 8 rates from one call.
The host form - the statement of the semantics the seed kernel is held against on the GPU - must equal the numpy twin of the definition
(tests/seedrategen.py: brute-force distances on the strided sets) AND the composition it replaces (vdf_align_seed_pairs_host on the sub-sampled
sets, united over the phases) on every problem the GPU tests use; it must hold every pair vdf_align_windows_retimed_host has a record for; at 1/1 it
is vdf_align_seed_pairs_host's set; duplicate and unreduced rates get a slot each; exclude_same drops the diagonal; the capacity protocol and
every refusal of the header are checked through ctypes.  api.align_rates(one_pass=True) returns align_rates' dict on the corpus of
tests/test_align_rates_host.py, with static flags and with pairs=, on the host forms alone."""
import ctypes as C
import os

import numpy as np
import pytest

import seedrategen as gen

NAMES = list(gen.CASES) + ["dense"]
SEEDS = max(20, int(os.environ.get("VDF_FUZZ_SEEDS", "0")))


def host(p, capacity=4096, **over):
    import vid_dup_finder_lib_amd as vdf

    kw = dict(tol_int=p.tol, min_run=p.min_run, a_rate_first=p.a_rate_first, a_skip=p.a_skip, b_skip=p.b_skip, exclude_same=p.exclude_same, capacity=capacity)
    kw.update(over)
    return vdf.align_seed_pairs_rates_host(p.a_hashes, p.a_first, p.b_hashes, p.b_first, p.rates, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_host_is_the_twin_and_the_composition(name):
    import vid_dup_finder_lib_amd as vdf

    p = gen.case(name)
    got, found = host(p)
    assert found == len(got) and gen.triples_of(got) == list(gen.expected(name))
    assert gen.composition(p, vdf.align_seed_pairs_host) == list(gen.expected(name))


@pytest.mark.parametrize("name", gen.SPARSE)
def test_the_cases_decide_something(name):
    """the non-vacuity condition of the GPU cases, on the twin: between 2 % and 50 % of all (rate, a, b) are candidates, and every rate has at least
    one candidate and one non-candidate"""
    p = gen.case(name)
    want = gen.expected(name)
    pairs = (p.a_first.shape[1] - 1) * (len(p.b_first) - 1)
    assert 0.02 * pairs * len(p.rates) <= len(want) <= 0.5 * pairs * len(p.rates), (name, len(want))
    for r in range(len(p.rates)):
        n = sum(1 for t in want if t[2] == r)
        assert 1 <= n < pairs, (name, r, n)
    assert pairs % 32, "slot boundaries fall inside bitmap words"


def test_the_dense_case_is_dense():
    p = gen.case("dense")
    assert len(gen.expected("dense")) > 0.4 * len(p.rates) * (p.a_first.shape[1] - 1) * (len(p.b_first) - 1)


@pytest.mark.parametrize("name", ["tol250_run2", "tol350_run3", "big_num"])
def test_every_pair_with_a_record_is_a_candidate(name):
    import vid_dup_finder_lib_amd as vdf

    p = gen.case(name)
    want = set(gen.expected(name))
    records = 0
    for r, rate in enumerate(p.rates):
        ah, af, ak = gen.block(p, r)
        rec, n = vdf.align_windows_retimed_host(ah, af, p.b_hashes, p.b_first, rate, tol_int=p.tol, min_run=p.min_run, a_skip=ak, b_skip=p.b_skip, capacity=4096)
        assert n == len(rec)
        records += n
        assert {(int(x["a"]), int(x["b"]), r) for x in rec} <= want, (name, r)
    # single planted cells are runs of one window: at min_run 1 they are records, above it they are candidates without one - both sides are exercised
    assert records > 0 or p.min_run > 1


def test_runs_along_the_slope_are_found_and_seeded():
    """stretches of min_run and more cells along each rate's slope, at every phase: each has a record, and each is among the candidates"""
    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng([83, 9])
    rates = gen.USUAL_RATES
    a_hashes, a_first, a_rate_first, b_hashes, b_first = gen._layout(rng, rates, [40, 90, 64], [120, 77], 2, 1)
    for r, (num, den) in enumerate(rates):
        for a, b, ka, kb in [(0, 0, num - 1, 0), (1, 1, 7, 3 * den), (2, 0, 5 + r, 10 * den)]:
            for m in range(3):
                a_hashes[int(a_rate_first[r]) + int(a_first[r, a]) + ka + num * m] = b_hashes[int(b_first[b]) + kb + den * m]
    p = gen.Problem(a_hashes, a_first, a_rate_first, b_hashes, b_first, rates, 350, 3)
    got, _ = host(p)
    assert gen.triples_of(got) == gen.seed_rates_twin(p) == [(a, b, r) for r in range(5) for a, b in [(0, 0), (1, 1), (2, 0)]]
    for r, rate in enumerate(rates):
        ah, af, _ = gen.block(p, r)
        rec, n = vdf.align_windows_retimed_host(ah, af, b_hashes, b_first, rate, tol_int=350, min_run=3)
        assert [(int(x["a"]), int(x["b"]), int(x["n_windows"])) for x in rec] == [(0, 0, 3), (1, 1, 3), (2, 0, 3)]


def test_rate_one_is_the_plain_seed_call():
    import vid_dup_finder_lib_amd as vdf

    for name in ["tol150_run1", "tol350_run3", "dense"]:
        p = gen.case(name)
        r = list(p.rates).index((1, 1))
        ah, af, ak = gen.block(p, r)
        plain, n = vdf.align_seed_pairs_host(ah, af, p.b_hashes, p.b_first, tol_int=p.tol, min_run=p.min_run, a_skip=ak, b_skip=p.b_skip, capacity=4096)
        assert n == len(plain) and n > 0
        assert [(int(x["a"]), int(x["b"])) for x in plain] == [(a, b) for a, b, s in gen.expected(name) if s == r]


def test_duplicate_and_unreduced_rates_get_a_slot_each():
    """64/34 is 32/17 and 6/4 is 3/2: the same rate on the same block gives the same pairs, slot by slot"""
    p = gen.case("duplicates")
    n_rates = len(p.rates)
    per_block = int(p.a_rate_first[1])
    same = p._replace(a_hashes=np.tile(p.a_hashes[:per_block], (n_rates, 1)), a_skip=np.tile(p.a_skip[:per_block], n_rates), rates=((64, 34), (32, 17), (64, 34), (3, 2), (6, 4)))
    got = gen.triples_of(host(same)[0])
    assert got == gen.seed_rates_twin(same)
    by_slot = [[(a, b) for a, b, s in got if s == r] for r in range(n_rates)]
    assert by_slot[0] == by_slot[1] == by_slot[2] and by_slot[0] and by_slot[3] == by_slot[4]
    # and the blocks may lie on top of each other: a null a_rate_first is zeros
    one = same._replace(a_hashes=same.a_hashes[:per_block], a_skip=same.a_skip[:per_block], a_rate_first=np.zeros(n_rates + 1, np.int64))
    assert gen.triples_of(host(one, a_rate_first=None)[0]) == got


def test_exclude_same():
    p = gen.square()
    full = gen.triples_of(host(p)[0])
    assert full == gen.seed_rates_twin(p) and sum(1 for a, b, _ in full if a == b) == 2 * 7 and any(a != b for a, b, _ in full)
    ex = p._replace(exclude_same=True)
    got = gen.triples_of(host(ex)[0])
    assert got == gen.seed_rates_twin(ex) == [t for t in full if t[0] != t[1]]
    import vid_dup_finder_lib_amd as vdf

    with pytest.raises(vdf.VdfError):   # n_a != n_b
        host(ex._replace(b_first=ex.b_first[:-1]))


def test_capacity_protocol():
    p = gen.case("tol250_run2")
    want = list(gen.expected("tol250_run2"))
    got, found = host(p, capacity=0)
    assert len(got) == 0 and found == len(want)
    got, found = host(p, capacity=5)
    assert found == len(want) > 5 and gen.triples_of(got) == want[:5]
    got, found = host(p, capacity=found)
    assert found == len(want) and gen.triples_of(got) == want


def _job(p, **over):
    """the job of the host form through ctypes, for the refusals numpy arguments cannot express: (job, what it points into)"""
    from vid_dup_finder_lib_amd import _capi

    num = np.array([r[0] for r in p.rates], np.uint32)
    den = np.array([r[1] for r in p.rates], np.uint32)
    rf = np.ascontiguousarray(p.a_rate_first, dtype=np.uintp)
    af = np.ascontiguousarray(p.a_first, dtype=np.uint32)
    bf = np.ascontiguousarray(p.b_first, dtype=np.uint32)
    out = np.zeros(4096, _capi.VIDEO_PAIR_RATE_DTYPE)
    n = C.c_size_t(77)
    f = dict(a_hashes=p.a_hashes.ctypes.data, a_first=af.ctypes.data, a_rate_first=rf.ctypes.data, a_skip=None, n_a=af.shape[1] - 1, b_hashes=p.b_hashes.ctypes.data,
             b_first=bf.ctypes.data, b_skip=None, n_b=len(bf) - 1, n_rates=len(num), rate_num=num.ctypes.data, rate_den=den.ctypes.data, tol_int=p.tol,
             min_run=p.min_run, exclude_same=0, out=out.ctypes.data, capacity=out.size, n_out=C.pointer(n), stream=None)
    f.update(over)
    return _capi.VdfAlignSeedRatesJob(**f), (num, den, rf, af, bf, out, n)


def test_every_refusal_is_e_inval():
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    p = gen.square()
    call = lambda **over: (lambda jk: lib.vdf_align_seed_pairs_rates_host(C.byref(jk[0])))(_job(p, **over))
    arr = lambda v, t=np.uint32: np.array(v, t)
    assert call() == _capi.VDF_OK
    assert lib.vdf_align_seed_pairs_rates_host(None) == _capi.VDF_E_INVAL
    # the checks of vdf_align_seed_pairs: null pointers, min_run, 2^20 windows, a first array that decreases, on B and on every block of A; rows; pairs
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
    assert call(n_a=4097, n_b=4096, a_first=None, b_first=None, a_hashes=None, b_hashes=None) == _capi.VDF_E_INVAL    # null pointers come first ...
    wide_a, wide_b = np.zeros(2 * 4098, np.uint32), np.zeros(4097, np.uint32)
    assert call(n_a=4097, n_b=4096, a_first=wide_a.ctypes.data, b_first=wide_b.ctypes.data) == _capi.VDF_E_INVAL      # ... 4097 x 4096 pairs are too many
    # the rate list
    nine = arr([1] * 9)
    assert call(n_rates=0) == _capi.VDF_E_INVAL and call(rate_num=None) == _capi.VDF_E_INVAL and call(rate_den=None) == _capi.VDF_E_INVAL
    assert call(n_rates=9, rate_num=nine.ctypes.data, rate_den=nine.ctypes.data, a_first=np.zeros(9 * 8, np.uint32).ctypes.data) == _capi.VDF_E_INVAL
    for bad in ([(1, 1), (1, 0)], [(1, 1), (2, 3)], [(1, 1), (5, 2)], [(66, 34), (1, 1)], [(1, 1), (37, 36)]):
        nn, dd = arr([r[0] for r in bad]), arr([r[1] for r in bad])
        assert call(rate_num=nn.ctypes.data, rate_den=dd.ctypes.data) == _capi.VDF_E_INVAL, bad
    ok_n, ok_d = arr([64, 6]), arr([34, 4])
    assert call(rate_num=ok_n.ctypes.data, rate_den=ok_d.ctypes.data) == _capi.VDF_OK     # 64/34 is 32/17: the limit is on the reduced num
    # exclude_same
    assert call(exclude_same=1) == _capi.VDF_OK and call(exclude_same=1, n_b=6) == _capi.VDF_E_INVAL
    # empty input: VDF_OK with *n_out = 0, whatever the pointers of the empty side
    for over in (dict(n_a=0, a_hashes=None, a_first=None), dict(n_b=0, b_hashes=None, b_first=None)):
        job, keep = _job(p, **over)
        assert lib.vdf_align_seed_pairs_rates_host(C.byref(job)) == _capi.VDF_OK and keep[-1].value == 0
    # the order of two kinds: an empty side does not excuse min_run == 0 or a bad rate
    assert call(n_a=0, min_run=0) == _capi.VDF_E_INVAL and call(n_b=0, n_rates=0) == _capi.VDF_E_INVAL


def test_python_arguments_are_checked():
    import vid_dup_finder_lib_amd as vdf

    p = gen.square()
    with pytest.raises(ValueError):
        vdf.align_seed_pairs_rates_host(p.a_hashes, p.a_first[0], p.b_hashes, p.b_first, p.rates)           # a_first: one row per rate
    with pytest.raises(ValueError):
        vdf.align_seed_pairs_rates_host(p.a_hashes, p.a_first, p.b_hashes, p.b_first, p.rates, a_rate_first=[0, len(p.a_hashes)])   # behind the hashes
    with pytest.raises(ValueError):
        vdf.align_seed_pairs_rates_host(p.a_hashes, p.a_first, None, None, p.rates, a_rate_first=p.a_rate_first)
    with pytest.raises(vdf.VdfError):
        vdf.align_seed_pairs_rates_host(p.a_hashes, p.a_first, p.b_hashes, p.b_first, [(1, 1), (3, 1)], a_rate_first=p.a_rate_first)


@pytest.mark.parametrize("seed", range(SEEDS))
def test_seeded_random_problems(seed):
    p = gen.random_problem(np.random.default_rng([83, 11, seed]))
    got, found = host(p, capacity=1 << 12)
    assert found == len(got) and gen.triples_of(got) == gen.seed_rates_twin(p), (seed, p.rates, p.tol, p.min_run)


def _videos(p):
    """a generator problem as api.align_rates takes it: ({rate: windows of A}, windows of B, {rate: static flags}, static flags of B)"""
    import vid_dup_finder_lib_amd as vdf

    mk = lambda words, first, tag: [[vdf.VideoHash(w, f"{tag}{i}", 10 + i) for w in words[int(first[i]):int(first[i + 1])]] for i in range(len(first) - 1)]
    flags = lambda skip, first: [np.asarray(skip[int(first[i]):int(first[i + 1])]) for i in range(len(first) - 1)]
    wa = {rate: mk(gen.block(p, r)[0], p.a_first[r], "a") for r, rate in enumerate(p.rates)}
    sa = {rate: flags(gen.block(p, r)[2], p.a_first[r]) for r, rate in enumerate(p.rates)}
    return wa, mk(p.b_hashes, p.b_first, "b"), sa, flags(p.b_skip, p.b_first)


def test_candidate_pairs_rates_is_the_call_per_rate():
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd.api import ALIGN_HOST_CELLS

    p = gen.planted(rates=((1, 1), (3, 2), (6, 5)), tol=350, min_run=2, seed=12, ca=(0, 3, 31, 40), cb=(0, 1, 50, 9))   # 0.35 -> tol_int 350
    assert sum(p.a_first[0, -1:] - p.a_first[0, :1]) * 60 <= ALIGN_HOST_CELLS    # small enough for the host forms: no engine is looked for
    wa, wb, sa, sb = _videos(p)
    assert vdf.engine.tolerance_int(0.35) == p.tol
    got = vdf.candidate_pairs_rates(wa, wb, 0.35, min_run=2, static_a=sa, static_b=sb)
    want = gen.seed_rates_twin(p)
    assert want and got == {rate: [(a, b) for a, b, s in want if s == r] for r, rate in enumerate(p.rates)}
    with pytest.raises(ValueError):
        vdf.candidate_pairs_rates({(3, 1): wa[(1, 1)]}, wb)


@pytest.mark.parametrize("true", [(6, 5), (3, 2)])
def test_align_rates_one_pass_returns_the_same_dict(true):
    """the corpus of DESIGN.md 4.16 / 4.19: one seed call for all rates and one list call per rate, against one align_retimed per rate"""
    import vid_dup_finder_lib_amd as vdf
    from test_align_rates_host import CANDIDATES, MIN_RUN, TOLERANCE, hashed

    va, vb, _, _ = hashed(true)
    today = vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, seed=True, native=True)
    assert any(today.values()) and today == vdf.align_rates(va, vb, TOLERANCE, MIN_RUN)
    assert vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, seed=True, native=True, one_pass=True) == today
    # static flags: every third window of A at every rate, every fifth of B
    sa = {r: [np.arange(len(ws)) % 3 == 1 for ws in va[r]] for r in CANDIDATES}
    sb = [np.arange(len(ws)) % 5 == 2 for ws in vb]
    kw = dict(static_a=sa, static_b=sb, seed=True, native=True)
    flagged = vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, **kw)
    assert flagged != today and vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, one_pass=True, **kw) == flagged
    # a caller's list: the candidates that are on it
    pairs = [(0, 0), (0, 3), (1, 1), (1, 2)]
    listed = vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, seed=True, native=True, pairs=pairs)
    assert any(listed.values()) and vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, seed=True, native=True, pairs=pairs, one_pass=True) == listed
    with pytest.raises(ValueError):
        vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, one_pass=True)
    with pytest.raises(ValueError):
        vdf.align_rates(va, vb, TOLERANCE, MIN_RUN, seed=True, native=False, one_pass=True)
