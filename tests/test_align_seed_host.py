"""The seed calls and the align calls on a list of pairs without a GPU (include/vdf.h): vdf_align_seed_pairs_host,
vdf_align_windows_pairs_host and vdf_align_windows_stretches_pairs_host - the definitions in plain C++ - against the numpy twin of
tests/seedgen.py, on every named problem of aligngen.CASES and of stretchgen.CASES (each at its guards), on those of seedgen (which the GPU
test gives the seed kernel) and on 300 random small ones; the superset property itself; the python mirrors align(seed=True),
align_all(seed=True), candidate_pairs and the `pairs` keyword; what a pair list is refused for, with the message.  Pairs and records are
compared for equality."""
import ctypes as C

import numpy as np
import pytest

import aligngen
import hashgen
import seedgen
import stretchgen
import vid_dup_finder_lib_amd as vdf
from vid_dup_finder_lib_amd import api


def sides(p):
    return dict(b_hashes=p.b_hashes, b_first=p.b_first, tol_int=p.tol, a_skip=p.a_skip, b_skip=p.b_skip)


def seed_host(p, min_run=None, capacity=1 << 16):
    got, found = vdf.align_seed_pairs_host(p.a_hashes, p.a_first, min_run=p.min_run if min_run is None else min_run, capacity=capacity, **sides(p))
    return seedgen.pairs_of(got), found


def pairs_host(p, pairs, capacity=1 << 16):
    rec, found = vdf.align_windows_pairs_host(p.a_hashes, p.a_first, pairs, min_run=p.min_run, capacity=capacity, **sides(p))
    return aligngen.records(rec), found


def stretches_pairs_host(p, pairs, max_stretches, guard, capacity=1 << 16):
    rec, found = vdf.align_windows_stretches_pairs_host(p.a_hashes, p.a_first, pairs, min_run=p.min_run, max_stretches=max_stretches, guard=guard,
                                                        capacity=capacity, **sides(p))
    return stretchgen.records(rec), found


def test_the_pair_is_the_header_s():
    from vid_dup_finder_lib_amd import _capi

    assert vdf.VIDEO_PAIR_DTYPE.itemsize == 8 == C.sizeof(_capi.VdfVideoPair) and vdf.VIDEO_PAIR_DTYPE.names == ("a", "b")


@pytest.mark.parametrize("name", sorted(aligngen.CASES))
def test_seed_host_matches_the_twin_on_the_align_cases(name):
    p = aligngen.case(name)
    for min_run in sorted({p.min_run, 1, 3}):
        want = seedgen.seed_twin(p, min_run)
        got, found = seed_host(p, min_run)
        assert found == len(want) and got == want, min_run
    recs = {(r[0], r[1]) for r in aligngen.expected(name)}
    assert recs <= set(seed_host(p)[0])


@pytest.mark.parametrize("name", sorted(seedgen.BUILDERS))
def test_seed_host_matches_the_twin_on_the_seed_cases(name):
    p = seedgen.case(name)
    want = list(seedgen.expected(name))
    got, found = seed_host(p)
    assert found == len(want) and got == want


def test_the_seed_cases_say_what_they_are_meant_to():
    """the problems' builders against their own intent, on the twin alone"""
    for m in (2, 3, 4, 5, 6):
        p = seedgen.case(f"phases_{m}")
        recs = seedgen.expected_records(f"phases_{m}")
        # one run of exactly min_run windows per residue of its start, and the videos that hold them start off the array's grid
        assert [(r[0], r[1], r[3] % m, r[4]) for r in recs] == [(2 * r, 2 * r + 1, r, m) for r in range(m)]
        assert all(int(p.a_first[2 * r]) % m for r in range(1, m))
        # the single cells at window 0 of those videos: candidates without a record
        assert set(seedgen.expected(f"phases_{m}")) == {(2 * r, 2 * r + 1) for r in range(m)} | {(2 * r, 2 * r) for r in range(m)}
    assert seedgen.expected("skipped_seeds") == ((3, 4),)
    assert seedgen.expected("early_exit") == ((0, 0), (1, 1)) == seedgen.expected("early_exit_tol_100")
    for name, tol in (("early_exit", 350), ("early_exit_tol_100", 100)):
        p = seedgen.case(name)
        d = hashgen.all_distances(p.a_hashes, p.b_hashes)
        assert [int(d[i, i]) for i in range(3)] == [tol, tol, tol + 1]
        assert (p.a_hashes[0, :10] == p.b_hashes[0, :10]).all()                                          # all of it behind word 10
        assert sum(hashgen.hamming(p.a_hashes[1, w:w + 1], p.b_hashes[1, w:w + 1]) for w in range(7)) == min(tol, 448)  # all of it in front
    p = seedgen.case("early_exit_tol_100")
    assert (p.a_hashes[2, :13] == p.b_hashes[2, :13]).all()
    # tolerance 1024: every pair with a live seed and a live row
    p = seedgen.case("tile_edges_all")
    ca, cb = np.diff(p.a_first.astype(np.int64)), np.diff(p.b_first.astype(np.int64))
    assert list(seedgen.expected("tile_edges_all")) == [(a, b) for a in range(len(ca)) for b in range(len(cb)) if ca[a] and cb[b]]
    assert len(seedgen.expected("tile_edges")) > len(seedgen.expected_records("tile_edges")) >= 10
    assert seedgen.expected_records("tile_edges_min_run_above") == () and len(seedgen.expected("tile_edges_min_run_above")) >= 1


def test_every_pair_with_a_record_is_a_candidate():
    """the superset property, asserted directly on the host forms for min_run 1 ... 6"""
    names = [n for n in sorted(aligngen.CASES) if not n.startswith("static")] + ["static_self"]
    problems = [aligngen.case(n) for n in names] + [seedgen.case(n) for n in ("tile_edges", "tile_edges_self", "skipped_seeds")]
    rng = np.random.default_rng(31)
    problems += [aligngen.random_problem(rng) for _ in range(60)]
    seen = 0
    for p in problems:
        for min_run in range(1, 7):
            q = p._replace(min_run=min_run)
            rec, found = vdf.align_windows_host(q.a_hashes, q.a_first, min_run=min_run, capacity=1 << 16, **sides(q))
            assert found == len(rec)
            cand = set(seed_host(q)[0])
            with_record = {(int(r["a"]), int(r["b"])) for r in rec}
            assert with_record <= cand, (min_run, sorted(with_record - cand))
            seen += len(with_record)
    assert seen > 1000


def test_300_random_problems():
    rng = np.random.default_rng(32)
    n_pairs = n_cand = 0
    for i in range(300):
        p = aligngen.random_problem(rng)
        want = seedgen.seed_twin(p)
        got, found = seed_host(p)
        assert found == len(want) and got == want, i
        n_cand += len(want)
        # the align calls on the candidates are the all-pairs calls; on a sublist, the matching subset
        whole = aligngen.align_twin(p)
        assert pairs_host(p, want) == (whole, len(whole)), i
        sub = seedgen.sublist(p, i)
        assert pairs_host(p, sub)[0] == [r for r in whole if (r[0], r[1]) in set(sub)], i
        if i % 3 == 0:
            guard, ms = int(rng.integers(0, 3)), int(rng.integers(1, 9))
            whole_st = stretchgen.stretches_twin(p, ms, guard)
            assert stretches_pairs_host(p, want, ms, guard) == (whole_st, len(whole_st)), i
            assert stretches_pairs_host(p, sub, ms, guard)[0] == seedgen.stretches_pairs_twin(p, sub, ms, guard), i
        n_pairs += len(whole)
    assert n_pairs > 300 and n_cand > n_pairs


@pytest.mark.parametrize("name", sorted(aligngen.CASES))
def test_pairs_host_on_the_align_cases(name):
    """vdf_align_windows_pairs_host on every named case of aligngen: the seed call's candidates and the list of all pairs give the all-pairs
    twin's records, a sublist its part"""
    p = aligngen.case(name)
    whole = list(aligngen.expected(name))
    cand = seed_host(p)[0]
    assert cand == seedgen.seed_twin(p)
    assert pairs_host(p, cand) == (whole, len(whole))
    assert pairs_host(p, seedgen.all_pairs(p)) == (whole, len(whole))
    sub = seedgen.sublist(p, 1)
    assert pairs_host(p, sub)[0] == [r for r in whole if (r[0], r[1]) in set(sub)]
    assert pairs_host(p, []) == ([], 0)


@pytest.mark.parametrize("name,guard", stretchgen.CASES)
def test_seed_and_stretches_pairs_host_on_the_stretch_cases(name, guard):
    """every named case of stretchgen at each of its guards, eight ranks: the candidates are the twin's and hold every pair with a stretch;
    vdf_align_windows_stretches_pairs_host on the candidates and on all pairs gives stretchgen.expected, on a sublist its part; and
    vdf_align_windows_pairs_host on the candidates gives the rank-0 records"""
    p = stretchgen.case(name)
    want = list(stretchgen.expected(name, guard))
    cand, found = seed_host(p)
    assert found == len(cand) and cand == seedgen.seed_twin(p)
    assert {(r[0], r[1]) for r in want} <= set(cand)
    assert stretches_pairs_host(p, cand, 8, guard) == (want, len(want))
    assert stretches_pairs_host(p, seedgen.all_pairs(p), 8, guard) == (want, len(want))
    sub = seedgen.sublist(p, 2)
    assert stretches_pairs_host(p, sub, 8, guard)[0] == [r for r in want if (r[0], r[1]) in set(sub)]
    for max_stretches in (2, 1):
        part = list(stretchgen.expected(name, guard, max_stretches))
        assert stretches_pairs_host(p, cand, max_stretches, guard) == (part, len(part))
    assert pairs_host(p, cand)[0] == [r[:6] for r in want if r[6] == 0]
    if len(seedgen.all_pairs(p)) == 1:  # a one-pair problem: the empty sublist and the pair itself, whatever the draw above was
        assert stretches_pairs_host(p, [], 8, guard) == ([], 0)
        assert stretches_pairs_host(p, seedgen.all_pairs(p), 8, guard)[0] == want


def test_capacity_protocol():
    p = seedgen.case("tile_edges")
    want = list(seedgen.expected("tile_edges"))
    for cap in (0, 1, len(want) - 1, len(want)):
        got, found = seed_host(p, capacity=cap)
        assert found == len(want) and got == want[:cap]
    recs = list(seedgen.expected_records("tile_edges"))
    for cap in (0, 3, len(recs)):
        got, found = pairs_host(p, want, capacity=cap)
        assert found == len(recs) and got == recs[:cap]
        got, found = stretches_pairs_host(p, want, 1, 0, capacity=cap)
        assert found == len(recs) and [r[:6] for r in got] == recs[:cap]


def test_a_pair_list_is_refused_with_its_message():
    p = aligngen.case("self_mode")      # 12 videos, self mode
    q = aligngen.case("mixed_counts")   # 9 x 10 videos
    bad = [
        (p, [(0, 3), (0, 2)], "not strictly increasing in (a, b) at entry 1"),   # unsorted
        (p, [(1, 2), (0, 5)], "not strictly increasing in (a, b) at entry 1"),
        (p, [(0, 2), (0, 2)], "not strictly increasing in (a, b) at entry 1"),   # a duplicate
        (p, [(0, 2), (3, 12)], "pair 1 of the list names a video that does not exist"),
        (q, [(9, 0)], "pair 0 of the list names a video that does not exist"),
        (q, [(0, 0), (8, 10)], "pair 1 of the list names a video that does not exist"),
        (p, [(0, 1), (4, 4)], "pair 1 of the list has a >= b in self mode"),
        (p, [(5, 2)], "pair 0 of the list has a >= b in self mode"),
    ]
    for prob, pairs, message in bad:
        for call in (lambda: pairs_host(prob, pairs), lambda: stretches_pairs_host(prob, pairs, 2, 0), lambda: align_lists(prob, pairs=pairs)):
            with pytest.raises((vdf.VdfError, ValueError)) as ei:
                call()
            assert message in str(ei.value), (pairs, str(ei.value))
    assert pairs_host(q, [(8, 9)])[1] in (0, 1) and pairs_host(q, [(0, 0), (0, 1), (1, 0)])[1] >= 0  # a >= b is fine between two sets
    # the order of the checks, on the C ABI itself: a null list before everything, the align checks before the list, the listed-pairs limit
    from vid_dup_finder_lib_amd import _capi
    lib = _capi.load()
    h, f = p.a_hashes, p.a_first
    n, out = C.c_size_t(7), np.zeros(4, vdf.ALIGN_DTYPE)
    unsorted = np.array([(0, 3), (0, 2)], vdf.VIDEO_PAIR_DTYPE)
    call = lambda pairs, n_pairs, min_run=1, n_out=n: lib.vdf_align_windows_pairs_host(
        h.ctypes.data, f.ctypes.data, len(f) - 1, None, None, None, 0, None, pairs, n_pairs, 350, min_run, out.ctypes.data, 4, C.byref(n_out) if n_out is not None else None)
    assert call(None, 2, min_run=0) == _capi.VDF_E_INVAL
    assert call(unsorted.ctypes.data, 2, min_run=0) == _capi.VDF_E_INVAL and call(unsorted.ctypes.data, 2) == _capi.VDF_E_INVAL
    assert call(unsorted.ctypes.data, (1 << 24) + 1) == _capi.VDF_E_INVAL   # the limit is read before the list is
    assert call(unsorted.ctypes.data, 1) == _capi.VDF_OK and n.value == len(seedgen.pairs_twin(p, [(0, 3)]))
    assert call(None, 0) == _capi.VDF_OK and n.value == 0
    # stretches: max_stretches and guard where they are today
    with pytest.raises(vdf.VdfError):
        stretches_pairs_host(p, [(0, 1)], 9, 0)
    with pytest.raises(vdf.VdfError):
        stretches_pairs_host(p, [(0, 1)], 1, 2**20 + 1)
    with pytest.raises(ValueError):
        vdf.align_windows_pairs_host(h, f, [(0, -1)])
    with pytest.raises(ValueError):
        vdf.align_windows_pairs_host(h, f, [(0, 1, 2)])


def test_the_listed_pairs_limit_replaces_the_pairs_of_videos_limit():
    """5000 x 5000 videos of one window are 2.5e7 pairs of videos - above what the all-pairs and the seed calls take - and fine with a list"""
    rng = np.random.default_rng(33)
    h = hashgen.random_hashes(rng, 5000)
    f = np.arange(5001, dtype=np.uint32)
    g = h.copy()
    g[4999] = h[17]
    with pytest.raises(vdf.VdfError):
        vdf.align_windows_host(h, f, b_hashes=g, b_first=f)
    with pytest.raises(vdf.VdfError):
        vdf.align_seed_pairs_host(h, f, b_hashes=g, b_first=f)
    rec, found = vdf.align_windows_pairs_host(h, f, [(0, 0), (17, 4999), (4999, 17)], b_hashes=g, b_first=f)
    assert found == 2 and aligngen.records(rec) == [(0, 0, 0, 0, 1, 0), (17, 4999, 0, 0, 1, 0)]


# ---- the python mirrors ---------------------------------------------------------------------------------------------------------------------
def lists(hashes, first, tag):
    return [[vdf.VideoHash(hashes[k], f"/{tag}/{v}.mp4", 1) for k in range(int(first[v]), int(first[v + 1]))] for v in range(len(first) - 1)]


def static(skip, first):
    return None if skip is None else [skip[int(first[v]):int(first[v + 1])] for v in range(len(first) - 1)]


def align_lists(p, fn=None, **kw):
    fn = fn or api.align
    a = lists(p.a_hashes, p.a_first, "a")
    b = None if p.b_hashes is None else lists(p.b_hashes, p.b_first, "b")
    return fn(a, b, tolerance=min(p.tol, 1000) / 1000.0, min_run=p.min_run, static_a=static(p.a_skip, p.a_first),
              static_b=None if p.b_hashes is None else static(p.b_skip, p.b_first), **kw)


SMALL = ["first_diagonal", "two_runs_one_diagonal", "tie_two_diagonals", "min_run_2", "min_run_16", "skip_cuts", "skip_silences", "static_a_shorter",
         "static_self", "tolerance_350"]


def corpora():
    rng = np.random.default_rng(34)
    return [aligngen.case(n) for n in SMALL] + [seedgen.case(n) for n in ("phases_3", "phases_self_3", "skipped_seeds")] + \
        [aligngen.random_problem(rng) for _ in range(40)]


def test_seeded_equals_plain(monkeypatch):
    monkeypatch.setattr(api, "ALIGN_HOST_CELLS", 1 << 40)  # everything here is walked on the CPU
    seeded = 0
    for i, p in enumerate(corpora()):
        plain = align_lists(p)
        assert align_lists(p, seed=True) == plain, i
        plain_all = align_lists(p, api.align_all, guard=1)
        assert align_lists(p, api.align_all, guard=1, seed=True) == plain_all, i
        cand = align_lists(p, api.candidate_pairs)
        assert cand == seedgen.seed_twin(p) and {(g.a, g.b) for g in plain} <= set(cand), i
        # pairs: the candidates give the whole list, a sublist its part; with seed=True, the candidates on the list
        assert align_lists(p, pairs=cand) == plain and align_lists(p, api.align_all, guard=1, pairs=cand) == plain_all, i
        sub = seedgen.sublist(p, i)
        part = [g for g in plain if (g.a, g.b) in set(sub)]
        assert align_lists(p, pairs=sub) == part and align_lists(p, pairs=sub, seed=True) == part, i
        assert align_lists(p, pairs=np.array(sub, np.int64).reshape(-1, 2)) == part, i
        assert align_lists(p, api.align_all, guard=1, pairs=sub, seed=True) == [g for g in plain_all if (g.a, g.b) in set(sub)], i
        seeded += len(plain)
    assert seeded > 60


def test_seeded_align_aligns_only_the_candidates(monkeypatch):
    monkeypatch.setattr(api, "ALIGN_HOST_CELLS", 1 << 40)
    p = seedgen.case("tile_edges_self")
    given = []
    real = api.align_windows_pairs_host
    monkeypatch.setattr(api, "align_windows_pairs_host", lambda a, f, pairs, **k: (given.append(seedgen.pairs_of(pairs)), real(a, f, pairs, **k))[1])
    monkeypatch.setattr(api, "align_windows_host", lambda *a, **k: pytest.fail("the all-pairs call in a seeded align"))
    got = align_lists(p, seed=True)
    assert given == [list(seedgen.expected("tile_edges_self"))]
    assert [(g.a, g.b, g.offset_frames, g.first_frame_a, g.n_windows, round(g.mean_distance * g.n_windows)) for g in got] == \
        list(seedgen.expected_records("tile_edges_self"))


def test_seeded_align_splits_above_the_pair_limit(monkeypatch):
    monkeypatch.setattr(api, "ALIGN_HOST_CELLS", 1 << 40)
    for name in ("tile_edges_self", "tile_edges"):
        p = seedgen.case(name)
        whole, whole_all = align_lists(p), align_lists(p, api.align_all, guard=1)
        cand = align_lists(p, api.candidate_pairs)
        seeds = []
        real = api.align_seed_pairs_host
        monkeypatch.setattr(api, "align_seed_pairs_host",
                            lambda a, f, **k: (seeds.append((len(f) - 1, None if k.get("b_first") is None else len(k["b_first"]) - 1)), real(a, f, **k))[1])
        monkeypatch.setattr(api, "ALIGN_MAX_PAIRS", 100)  # blocks of 10 videos
        assert align_lists(p, seed=True) == whole
        assert len(seeds) == (10 if p.b_hashes is None else 16) and all((a * (a - 1) // 2 if b is None else a * b) <= 100 for a, b in seeds)
        assert align_lists(p, api.align_all, guard=1, seed=True) == whole_all
        assert align_lists(p, api.candidate_pairs) == cand
        monkeypatch.setattr(api, "ALIGN_FIRST_CAPACITY", 2)  # and the retry on a too-small buffer, of the seed call as of the align call
        assert align_lists(p, seed=True) == whole
        monkeypatch.undo()
        monkeypatch.setattr(api, "ALIGN_HOST_CELLS", 1 << 40)
