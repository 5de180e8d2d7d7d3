"""vdf_align_windows_rates_stretches_host on the CPU: every stretch of a retimed pair, ranked, over (rate, a, b) triples of up to 8
rates in one call.  The host form - the statement of the semantics the masked rates kernel is held against on the GPU - must equal the numpy twin of
tests/ratestretchgen.py in its three triple modes on the planted cases (a 6/5 copy with a cut, a source used twice, a replaced scene, exactly
max_stretches stretches and more, an unrelated library) and on every problem the GPU tests use.  The phase trap shows that the rectangle of a
stretch must mask EVERY phase, and that a masking of its own phase alone would be caught.  max_stretches = 1 is vdf_align_windows_rates_host with
rank 0; a one-rate list at 1/1 is vdf_align_windows_stretches_pairs_host; 6/5 beside 12/10 gives equal records in two slots; seed = 1 equals seed =
0; exclude_same, the capacity protocol, guard 0 and a guard larger than the videos, every refusal of the header in its order through ctypes, seeded
random problems, and api.align_rates_all / best_rates_all on the host route."""
import ctypes as C
import os

import numpy as np
import pytest

import ratealigngen as gen
import ratestretchgen as sg
import seedrategen as sgen

NAMES = list(sg.CASES)
SEEDS = max(20, int(os.environ.get("VDF_FUZZ_SEEDS", "0")))


def host(p, max_stretches, guard, capacity=4096, **over):
    import vid_dup_finder_lib_amd as vdf

    kw = dict(tol_int=p.tol, min_run=p.min_run, max_stretches=max_stretches, guard=guard, a_rate_first=p.a_rate_first, a_skip=p.a_skip, b_skip=p.b_skip,
              exclude_same=p.exclude_same, capacity=capacity)
    kw.update(over)
    return vdf.align_windows_rates_stretches_host(p.a_hashes, p.a_first, p.b_hashes, p.b_first, p.rates, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_the_cases_hold_a_rank_one_record(name):
    sg.check_non_vacuous(name)


@pytest.mark.parametrize("name", NAMES)
def test_host_is_the_twin_in_all_three_modes(name):
    sg.check_non_vacuous(name)   # on the twin's output, before any comparison
    p, most, guard = sg.case(name)
    want = list(sg.expected(name))
    got, found = host(p, most, guard)
    assert found == len(got) and sg.records(got) == want
    got, found = host(p, most, guard, seed=True)
    assert found == len(got) and sg.records(got) == want
    every = gen.all_triples(p)
    for triples in (every[::2], gen.candidates(p), sorted({(w[2], w[0], w[1]) for w in want})):
        got, found = host(p, most, guard, triples=gen.triple_array(triples), exclude_same=False)
        assert found == len(got) and sg.records(got) == sg.twin(p._replace(exclude_same=False), most, guard, triples), name


def test_the_phase_trap():
    """6/5, min_run 1, one planted stretch in slowly changing content.  Every later record must lie outside the rank-0 rectangle - in b's rows
    outside it, or in other rows of a - and a masking of rank 0 in its own phase only reports the same stretch again from the phases beside it."""
    p, most, guard = sg.slow_content()
    want = sg.twin(p, most, guard)
    got = sg.records(host(p, most, guard)[0])
    assert got == want and [w[8] for w in got] == [0, 1, 2, 3]
    r0 = got[0]
    assert r0[3:6] == (23, 10, 7) and r0[6] == 0                    # the planted stretch, phase 5
    a_lo, a_hi, b_lo, b_hi = sg.rect_of(r0[3], r0[4], r0[5], (6, 5), guard, 100, 60)
    for w in got[1:]:
        for ra, rb in sg.cells_of(w, (6, 5)):
            assert not (a_lo <= ra < a_hi and b_lo <= rb < b_hi), w
    wrong = sg.twin(p, most, guard, own_phase_only=True)
    assert wrong != want and wrong[1][8] == 1 and wrong[1][3] % 6 in (4, 0) and wrong[1][5] == 7       # phase 5 - 1 or 5 + 1: the same seven cells
    assert all(a_lo <= ra < a_hi and b_lo <= rb < b_hi for ra, rb in sg.cells_of(wrong[1], (6, 5)))
    # without a guard the rectangle is the stretch's own rows: still every phase of them
    got0 = sg.records(host(p, most, 0)[0])
    assert got0 == sg.twin(p, most, 0) and len(got0) > 1
    lo_a, hi_a, lo_b, hi_b = sg.rect_of(r0[3], r0[4], r0[5], (6, 5), 0, 100, 60)
    assert all(not (lo_a <= ra < hi_a and lo_b <= rb < hi_b) for w in got0[1:] for ra, rb in sg.cells_of(w, (6, 5)))


@pytest.mark.parametrize("name", ["cut_6_5_offsets", "exactly_max", "dense", "four_rates"])
def test_max_stretches_one_is_the_rates_call_with_rank_zero(name):
    import vid_dup_finder_lib_amd as vdf

    p, _, guard = sg.case(name)
    plain, n = vdf.align_windows_rates_host(p.a_hashes, p.a_first, p.b_hashes, p.b_first, p.rates, tol_int=p.tol, min_run=p.min_run, a_rate_first=p.a_rate_first,
                                            a_skip=p.a_skip, b_skip=p.b_skip, capacity=4096)
    got, found = host(p, 1, guard)
    assert n == found == len(got) >= 1 and sg.records(got) == [r + (0,) for r in gen.records(plain)]
    # and rank 0 of any max_stretches is that record, field for field
    assert [w[:8] for w in sg.expected(name) if w[8] == 0] == gen.records(plain)


def test_one_rate_at_1_1_is_the_plain_stretches_pairs_call():
    """at 1/1 the rectangle is DESIGN 4.12's: first_a = start_a, first_b = start_a + offset, n_frames_b = n_windows + 15"""
    import vid_dup_finder_lib_amd as vdf

    for name, guard in (("dense", 1), ("dense", 0), ("four_rates_offsets", 2), ("bands3", 6)):
        p = sg.case(name)[0]
        ah, af, ak = sgen.block(p, 0)
        assert gen.reduced(p.rates[0]) == (1, 1)
        pairs = [(a, b) for a in range(len(af) - 1) for b in range(len(p.b_first) - 1)]
        plain, n = vdf.align_windows_stretches_pairs_host(ah, af, pairs, p.b_hashes, p.b_first, tol_int=p.tol, min_run=p.min_run, max_stretches=5, guard=guard,
                                                          a_skip=ak, b_skip=p.b_skip, capacity=4096)
        got, found = vdf.align_windows_rates_stretches_host(ah, af[None, :], p.b_hashes, p.b_first, [(1, 1)], tol_int=p.tol, min_run=p.min_run, max_stretches=5,
                                                            guard=guard, a_skip=ak, b_skip=p.b_skip, triples=[(0, a, b) for a, b in pairs], capacity=4096)
        assert n == len(plain) == found >= 1
        assert sg.records(got) == [(int(x["a"]), int(x["b"]), 0, int(x["start_a"]), int(x["start_a"]) + int(x["offset"]), int(x["n_windows"]),
                                    int(x["dist_sum"]), int(x["n_windows"]) + 15, int(x["rank"])) for x in plain]
    assert any(int(x["rank"]) >= 1 for x in plain)


def test_a_rate_beside_its_unreduced_spelling_gives_equal_records_in_two_slots():
    p, most, guard = sg.case("cut_6_5")
    lo, hi = int(p.a_rate_first[1]), int(p.a_rate_first[2])
    a_hashes = np.concatenate([p.a_hashes, p.a_hashes[lo:hi]])
    q = p._replace(a_hashes=a_hashes, a_first=np.concatenate([p.a_first, p.a_first[1:2]]), a_rate_first=np.concatenate([p.a_rate_first, [len(a_hashes)]]),
                   rates=p.rates + ((12, 10),))
    got = sg.records(host(q, most, guard)[0])
    assert got == sg.twin(q, most, guard)
    slot = lambda r: [w[:2] + w[3:] for w in got if w[2] == r]
    assert len(slot(1)) == 2 and slot(1) == slot(3)


@pytest.mark.parametrize("name", sg.SEEDED)
def test_seed_one_equals_seed_zero(name):
    p, most, guard = sg.case(name)
    assert sg.records(host(p, most, guard, seed=True)[0]) == sg.records(host(p, most, guard)[0]) == list(sg.expected(name))


def test_exclude_same():
    import vid_dup_finder_lib_amd as vdf

    ex = sg.case("square")[0]
    full = sg.records(host(ex, 3, 1, exclude_same=False)[0])
    assert ex.exclude_same and sum(1 for r in full if r[0] == r[1]) == 2 * 3 * 2 and any(r[8] >= 1 and r[0] != r[1] for r in full)
    assert sg.records(host(ex, 3, 1)[0]) == [r for r in full if r[0] != r[1]] == sg.twin(ex, 3, 1)
    assert sg.records(host(ex, 3, 1, seed=True)[0]) == sg.twin(ex, 3, 1)
    with pytest.raises(vdf.VdfError):   # n_a != n_b
        host(ex._replace(b_first=ex.b_first[:-1]), 3, 1)


def test_capacity_protocol():
    p, most, guard = sg.case("dense")
    want = list(sg.expected("dense"))
    triples = gen.triple_array(sorted({(w[2], w[0], w[1]) for w in want}))
    for kw in (dict(), dict(seed=True), dict(triples=triples)):
        for m in (most, 1):
            w = [x for x in want if x[8] < m]
            got, found = host(p, m, guard, capacity=0, **kw)
            assert len(got) == 0 and found == len(w)
            got, found = host(p, m, guard, capacity=5, **kw)
            assert found == len(w) > 5 and sg.records(got) == w[:5]
            got, found = host(p, m, guard, capacity=found, **kw)
            assert found == len(w) and sg.records(got) == w


def test_guard_zero_and_a_guard_larger_than_the_videos():
    for name in ("cut_6_5", "replaced_scene", "seven_rects", "dense"):
        p, most, _ = sg.case(name)
        g0 = sg.records(host(p, most, 0)[0])
        assert g0 == sg.twin(p, most, 0) and any(w[8] >= 1 for w in g0)
        big = sg.records(host(p, most, 1 << 20)[0])
        assert big == sg.twin(p, most, 1 << 20) and big and all(w[8] == 0 for w in big)     # the whole matrix is one rectangle: rank 0 alone
        assert big == [w for w in g0 if w[8] == 0]


def _job(p, **over):
    """the job of the host form through ctypes, for the refusals numpy arguments cannot express: (job, what it points into)"""
    from vid_dup_finder_lib_amd import _capi

    num = np.array([r[0] for r in p.rates], np.uint32)
    den = np.array([r[1] for r in p.rates], np.uint32)
    rf = np.ascontiguousarray(p.a_rate_first, dtype=np.uintp)
    af = np.ascontiguousarray(p.a_first, dtype=np.uint32)
    bf = np.ascontiguousarray(p.b_first, dtype=np.uint32)
    out = np.zeros(4096, _capi.ALIGN_RATE_STRETCH_DTYPE)
    n = C.c_size_t(77)
    f = dict(a_hashes=p.a_hashes.ctypes.data, a_first=af.ctypes.data, a_rate_first=rf.ctypes.data, a_skip=None, n_a=af.shape[1] - 1, b_hashes=p.b_hashes.ctypes.data,
             b_first=bf.ctypes.data, b_skip=None, n_b=len(bf) - 1, n_rates=len(num), rate_num=num.ctypes.data, rate_den=den.ctypes.data, tol_int=p.tol,
             min_run=p.min_run, triples=None, n_triples=0, seed=0, exclude_same=0, max_stretches=4, guard=15, out=out.ctypes.data, capacity=out.size,
             n_out=C.pointer(n), stream=None)
    f.update(over)
    return _capi.VdfAlignRatesStretchesJob(**f), (num, den, rf, af, bf, out, n)


def test_every_refusal_is_e_inval_in_the_headers_order():
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    p = sgen.square()
    call = lambda **over: (lambda jk: lib.vdf_align_windows_rates_stretches_host(C.byref(jk[0])))(_job(p, **over))
    arr = lambda v, t=np.uint32: np.array(v, t)
    tri = lambda v: np.array(v, _capi.VIDEO_PAIR_RATE_DTYPE)   # (a, b, rate)
    assert _capi.ALIGN_RATE_STRETCH_DTYPE.itemsize == 36 and _capi.ALIGN_RATE_STRETCH_DTYPE.names[:8] == _capi.ALIGN_RATE_DTYPE.names
    assert call() == _capi.VDF_OK
    # 1. those of vdf_align_windows_rates*, in their order: a null job; the seed call's checks, B first and then the blocks of A; the rate list
    assert lib.vdf_align_windows_rates_stretches_host(None) == _capi.VDF_E_INVAL
    for field in ("n_out", "out", "b_hashes", "b_first", "a_hashes", "a_first"):
        assert call(**{field: None}) == _capi.VDF_E_INVAL, field
    assert call(min_run=0) == _capi.VDF_E_INVAL
    long_b, long_a = p.b_first.copy(), p.a_first.copy()
    long_b[1:] += (1 << 20) + 1
    long_a[1, 3:] += (1 << 20) + 1
    down_b, down_a = p.b_first.copy(), p.a_first.copy()
    down_b[2] = down_b[1] - 1
    down_a[1, 2] = down_a[1, 1] - 1
    assert call(b_first=long_b.ctypes.data) == _capi.VDF_E_INVAL and call(a_first=long_a.ctypes.data) == _capi.VDF_E_INVAL
    assert call(b_first=down_b.ctypes.data) == _capi.VDF_E_INVAL and call(a_first=down_a.ctypes.data) == _capi.VDF_E_INVAL
    far = arr([0, 2**32 - 5, 0], np.uintp)
    assert call(a_rate_first=far.ctypes.data) == _capi.VDF_E_INVAL
    wide_a, wide_b = np.zeros(2 * 4098, np.uint32), np.zeros(4097, np.uint32)
    assert call(n_a=4097, n_b=4096, a_first=wide_a.ctypes.data, b_first=wide_b.ctypes.data) == _capi.VDF_E_INVAL
    nine = arr([1] * 9)
    assert call(n_rates=0) == _capi.VDF_E_INVAL and call(rate_num=None) == _capi.VDF_E_INVAL and call(rate_den=None) == _capi.VDF_E_INVAL
    assert call(n_rates=9, rate_num=nine.ctypes.data, rate_den=nine.ctypes.data, a_first=np.zeros(9 * 8, np.uint32).ctypes.data) == _capi.VDF_E_INVAL
    for bad in ([(1, 1), (1, 0)], [(1, 1), (2, 3)], [(1, 1), (5, 2)], [(66, 34), (1, 1)], [(1, 1), (37, 36)]):
        nn, dd = arr([r[0] for r in bad]), arr([r[1] for r in bad])
        assert call(rate_num=nn.ctypes.data, rate_den=dd.ctypes.data) == _capi.VDF_E_INVAL, bad
    assert call(exclude_same=1) == _capi.VDF_OK and call(exclude_same=1, n_b=6) == _capi.VDF_E_INVAL
    good = tri([(0, 0, 0), (0, 1, 0), (3, 2, 0), (0, 0, 1), (6, 6, 1)])
    assert call(triples=good.ctypes.data, n_triples=len(good)) == _capi.VDF_OK
    assert call(triples=good.ctypes.data, n_triples=len(good), seed=1) == _capi.VDF_E_INVAL
    assert call(triples=good.ctypes.data, n_triples=len(good), exclude_same=1) == _capi.VDF_E_INVAL
    assert call(seed=1) == _capi.VDF_OK and call(seed=1, exclude_same=1) == _capi.VDF_OK
    assert call(triples=good.ctypes.data, n_triples=(1 << 27) + 1) == _capi.VDF_E_INVAL
    for bad in ([(0, 1, 0), (0, 0, 0)], [(0, 0, 1), (0, 0, 0)], [(2, 2, 1), (2, 2, 1)], [(0, 0, 2)], [(7, 0, 0)], [(0, 7, 1)]):
        t = tri(bad)
        assert call(triples=t.ctypes.data, n_triples=len(t)) == _capi.VDF_E_INVAL, bad
    # 2. max_stretches outside 1 ... 8
    assert call(max_stretches=0) == _capi.VDF_E_INVAL and call(max_stretches=9) == _capi.VDF_E_INVAL
    assert call(max_stretches=1) == _capi.VDF_OK and call(max_stretches=8) == _capi.VDF_OK
    # 3. guard above 2^20
    assert call(guard=(1 << 20) + 1) == _capi.VDF_E_INVAL and call(guard=1 << 20) == _capi.VDF_OK and call(guard=0) == _capi.VDF_OK
    # (4. a multi-GPU context: the GPU test.)  A refused call writes nothing, whatever else is wrong with it
    for over in (dict(max_stretches=0, guard=1 << 21), dict(max_stretches=9, n_rates=0), dict(guard=1 << 21, triples=tri([(7, 0, 0)]).ctypes.data, n_triples=1)):
        job, keep = _job(p, **over)
        assert lib.vdf_align_windows_rates_stretches_host(C.byref(job)) == _capi.VDF_E_INVAL and keep[-1].value == 77
    # empty input: VDF_OK with *n_out = 0 - but a bad max_stretches or guard is refused before that
    for over in (dict(n_a=0, a_hashes=None, a_first=None), dict(n_b=0, b_hashes=None, b_first=None), dict(triples=good.ctypes.data, n_triples=0)):
        job, keep = _job(p, **over)
        assert lib.vdf_align_windows_rates_stretches_host(C.byref(job)) == _capi.VDF_OK and keep[-1].value == 0
        assert call(max_stretches=0, **over) == _capi.VDF_E_INVAL and call(guard=1 << 21, **over) == _capi.VDF_E_INVAL


def test_refusals_come_in_the_headers_order_through_the_python_wrapper():
    """the wrapper names nothing, so the order is read from pairs of faults: a fault of the rates call beside a bad max_stretches is still refused,
    and python checks its own arguments first"""
    import vid_dup_finder_lib_amd as vdf

    p = sgen.square()
    with pytest.raises(vdf.VdfError):
        host(p, 0, 15)
    with pytest.raises(vdf.VdfError):
        host(p, 4, (1 << 20) + 1)
    with pytest.raises(ValueError):
        host(p, 4, -1)
    with pytest.raises(ValueError):
        vdf.align_windows_rates_stretches_host(p.a_hashes, p.a_first[0], p.b_hashes, p.b_first, p.rates)           # a_first: one row per rate
    assert vdf.ALIGN_RATE_STRETCH_DTYPE.itemsize == 36


_RANKS = {}


@pytest.mark.parametrize("seed", range(SEEDS))
def test_seeded_random_problems(seed):
    p, most, guard = sg.random_problem(np.random.default_rng([92, 11, seed]))
    want = sg.twin(p, most, guard)
    _RANKS[seed] = max([0] + [w[8] for w in want])
    got, found = host(p, most, guard, capacity=1 << 12)
    assert found == len(got) and sg.records(got) == want, (seed, p.rates, p.tol, p.min_run, most, guard)
    got, found = host(p, most, guard, capacity=1 << 12, seed=True)
    assert sg.records(got) == want, (seed, p.rates, p.tol, p.min_run, most, guard)


def test_the_random_problems_hold_ranks_up_to_two():
    """on the twin's output: comparing empty lists shows nothing"""
    for seed in range(20):
        if seed not in _RANKS:
            p, most, guard = sg.random_problem(np.random.default_rng([92, 11, seed]))
            _RANKS[seed] = max([0] + [w[8] for w in sg.twin(p, most, guard)])
    assert max(_RANKS[s] for s in range(20)) >= 2, _RANKS


# ---- the Python route ---------------------------------------------------------------------------------------------------------------------
def _as_windows(p, static=False):
    """a generator problem as align_rates_all takes it: ({rate: windows of A}, windows of B, static flags of A, of B)"""
    import vid_dup_finder_lib_amd as vdf

    def side(words, first, tag):
        return [[vdf.VideoHash(words[k], f"/{tag}/{v}.mp4", 10 + v) for k in range(int(first[v]), int(first[v + 1]))] for v in range(len(first) - 1)]
    wa = {rate: side(*sgen.block(p, r)[:2], f"a{r}") for r, rate in enumerate(p.rates)}
    wb = side(p.b_hashes, p.b_first, "b")
    sa = sb = None
    if static:
        sa = {rate: [np.asarray(sgen.block(p, r)[2][int(f0):int(f1)]) != 0 for f0, f1 in zip(sgen.block(p, r)[1][:-1], sgen.block(p, r)[1][1:])]
              for r, rate in enumerate(p.rates)}
        sb = [np.asarray(p.b_skip[int(f0):int(f1)]) != 0 for f0, f1 in zip(p.b_first[:-1], p.b_first[1:])]
    return wa, wb, sa, sb


def _as_stretches(p, want):
    out = {rate: [] for rate in p.rates}
    for a, b, r, fa, fb, n, s, nfb, rank in want:
        num, den = gen.reduced(p.rates[r])
        out[p.rates[r]].append((a, b, num, den, fa, fb, (n - 1) * num + (15 * num) // den + 1, nfb, n, s / n, f"/a{r}/{a}.mp4", f"/b/{b}.mp4", rank))
    return out


@pytest.mark.parametrize("name", ["cut_6_5", "cut_6_5_offsets", "four_rates_offsets", "replaced_scene", "unrelated"])   # small enough for the host route
def test_align_rates_all_on_the_host_route_is_the_twin(name):
    import vid_dup_finder_lib_amd as vdf

    p, most, guard = sg.case(name)
    static = p.a_skip is not None
    wa, wb, sa, sb = _as_windows(p, static)
    tolerance = p.tol / 1000.0
    kw = dict(tolerance=tolerance, min_run=p.min_run, max_stretches=most, guard=guard, static_a=sa, static_b=sb)
    want = _as_stretches(p, sg.expected(name))
    got = vdf.align_rates_all(wa, wb, **kw)
    assert list(got) == list(p.rates) and {r: [tuple(x) for x in v] for r, v in got.items()} == want
    assert all(isinstance(x, vdf.RetimedAlignmentStretch) for v in got.values() for x in v)
    assert vdf.align_rates_all(wa, wb, seed=True, **kw) == got
    n_a, n_b = p.a_first.shape[1] - 1, len(p.b_first) - 1
    pairs = [(a, b) for a in range(n_a) for b in range(n_b) if (a + b) % 2 == 1]
    listed = _as_stretches(p, sg.twin(p, most, guard, [(r, a, b) for r in range(len(p.rates)) for a, b in pairs]))
    assert {r: [tuple(x) for x in v] for r, v in vdf.align_rates_all(wa, wb, pairs=pairs, **kw).items()} == listed
    assert {r: [tuple(x) for x in v] for r, v in vdf.align_rates_all(wa, wb, pairs=pairs, seed=True, **kw).items()} == listed
    if name == "cut_6_5":
        assert listed[(6, 5)] and vdf.align_rates_all(wa, wb, tolerance, p.min_run) == vdf.align_rates_all(wa, wb, tolerance, p.min_run, 4, 15)   # guard None: 15
        # rank 0 is align_rates' record, and best_rates_all names 6/5 for the copy with both of its stretches
        plain = vdf.align_rates(wa, wb, tolerance, p.min_run, one_call=True)
        assert {r: [tuple(x)[:12] for x in v if x.rank == 0] for r, v in got.items()} == {r: [tuple(x) for x in v] for r, v in plain.items()}
        best = vdf.best_rates_all(got, tolerance)
        assert list(best) == [(2, 1)] and [(x.num, x.den, x.rank) for x in best[(2, 1)]] == [(6, 5, 0), (6, 5, 1)]


def test_best_rates_all_on_a_hand_made_dict():
    import vid_dup_finder_lib_amd as vdf

    R = vdf.RetimedAlignmentStretch
    # pair (0, 1): 1/1 has ONE stretch of 40 frames of b at distance 0 (40 * 351 = 14040); 6/5 has two of 26 and 21 frames at distance 10
    # (47 * 341 = 16027): together they cover more - best_rates, which sees rank 0 alone, would name 1/1 (26 * 341 = 8866)
    a0 = R(0, 1, 1, 1, 0, 0, 40, 40, 25, 0.0, None, None, 0)
    b0 = R(0, 1, 6, 5, 0, 0, 31, 26, 3, 10.0, None, None, 0)
    b1 = R(0, 1, 6, 5, 60, 70, 25, 21, 2, 10.0, None, None, 1)
    c0 = R(2, 0, 6, 5, 0, 0, 19, 16, 1, 0.0, None, None, 0)
    result = {(1, 1): [a0], (6, 5): [b0, b1, c0]}
    assert vdf.best_rates_all(result, 0.35) == {(0, 1): [b0, b1], (2, 0): [c0]}
    assert list(vdf.best_rates_all(result, 0.35)) == [(0, 1), (2, 0)]
    assert [(r.num, r.den) for r in vdf.best_rates({k: [x for x in v if x.rank == 0] for k, v in result.items()}, 0.35)] == [(1, 1), (6, 5)]
    # a tie goes to the rate that comes first in the caller's dict; the stretches come by rank whatever their order in the list
    t1, t2 = R(0, 0, 1, 1, 0, 0, 16, 16, 1, 0.0, None, None, 0), R(0, 0, 6, 5, 3, 0, 19, 16, 1, 0.0, None, None, 0)
    assert vdf.best_rates_all({(1, 1): [t1], (6, 5): [t2]}, 0.35) == {(0, 0): [t1]} and vdf.best_rates_all({(6, 5): [t2], (1, 1): [t1]}, 0.35) == {(0, 0): [t2]}
    assert vdf.best_rates_all({(6, 5): [b1, b0]}, 0.35) == {(0, 1): [b0, b1]}
    assert vdf.best_rates_all({}, 0.35) == {} and vdf.best_rates_all({(1, 1): []}, 0.35) == {}
