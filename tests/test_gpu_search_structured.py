"""HIP search vs the CPU oracle on hashes whose bits are NOT fair coin flips (hashgen.structured_pairs): all-zero, all-one,
half-set and one-bit hashes with pairs exactly on and one over the tolerance, their differing bits inside or outside the
prefix the kernels test first.  On iid hashes a true hit's prefix distance sits ~60 bits under the tolerance, and a prefix
popcount over the wrong dwords, a stale one, or > for >= at the threshold changes nothing; here each of them loses hits
(test_search_structured_corpus.py shows that on a numpy twin of the test).  Everything is == the oracle."""
import functools

import numpy as np
import pytest

import hashgen as hg
from oracle import vdf_oracle as orc

pytestmark = pytest.mark.gpu
DUR = 100  # every duration: all windows are the whole set


def _dur(n):
    return np.full(n, DUR, np.uint32)


@functools.lru_cache(maxsize=None)
def _refs(tol, prefix):
    """(case, the oracle's search_with_references on it): once per (tolerance, prefix), shared by both backends where they
    test the same prefix"""
    case = hg.refs_case(hg.corpus_rng(tol, prefix), tol, prefix)
    return case, orc.search_refs_sorted(case.cand, _dur(len(case.cand)), case.refs, _dur(len(case.refs)), tol)


@functools.lru_cache(maxsize=None)
def _self(tol, prefix, n):
    case = hg.self_case(hg.corpus_rng(tol, prefix), tol, prefix, n)
    return case, orc.search_self_sorted(case.cand, _dur(n), tol)


def _early_exit_bits(backend, step):
    inst = hg.instantiated_step(backend, step)
    return 64 * (inst + 1) if inst < 15 else 0


def _check_refs(eng, backend, step, tol):
    case, want = _refs(tol, hg.tested_dwords(backend, step))
    got = eng.search_refs_sorted(case.cand, _dur(len(case.cand)), case.refs, _dur(len(case.refs)), tol)
    assert got == want
    # the corpus was built for the prefix this launch really tested
    assert eng.last_stats()["early_exit_bits"] == _early_exit_bits(backend, step)
    if tol < 1024:  # pairs on both sides of the tolerance: some references match, and never everything
        assert 0 < sum(len(m) for _, m in got) < len(case.cand) * len(case.refs)


def _check_self(eng, backend, step, tol, n):
    case, want = _self(tol, hg.tested_dwords(backend, step), n)
    assert eng.search_self_sorted(case.cand, _dur(n), tol) == want
    assert eng.last_stats()["early_exit_bits"] == _early_exit_bits(backend, step)
    assert len(want) > 0


@pytest.mark.parametrize("tol", hg.AUTO_TOLERANCES)
def test_refs_structured_pairs_on_both_sides_of_every_tolerance(engine, tol):
    """search_with_references outputs every hit: ~800 references (four 256-row tiles, the last one partly padding) against
    their partners among 1100 candidates (nine 128-column stages, the last one partly padding), at the tolerances on both
    sides of every automatic step change and at the ends of the range."""
    _check_refs(engine, engine.backend, hg.auto_step(tol), tol)


@pytest.mark.parametrize("n", [1100, 513])
@pytest.mark.parametrize("tol", hg.AUTO_TOLERANCES)
def test_self_salted_pairs_on_both_sides_of_every_tolerance(engine, tol, n):
    """search() compares groups, so only the salted bases (isolated pairs: a lost hit is a lost group).  1100 = three 512-row
    tiles, 513 = one tile and a one-row remainder."""
    _check_self(engine, engine.backend, hg.auto_step(tol), tol, n)


@pytest.mark.parametrize("step,tol", hg.FORCED_STEP_TOLERANCES)
@pytest.mark.parametrize("backend", ["mfma", "valu"])
def test_every_instantiated_step_on_its_own_structured_corpus(backend, step, tol, monkeypatch):
    """Every kernel instance - the ones that keep the row term in LDS (steps 13 and up) included - against the corpus built
    from ITS prefix, in both modes."""
    import vid_dup_finder_lib_amd as vdf

    monkeypatch.setenv("VDF_SEARCH_BACKEND", backend)
    monkeypatch.setenv("VDF_MFMA_PRUNE_STEP", str(step))
    eng = vdf.Engine(0)
    try:
        _check_refs(eng, backend, step, tol)
        _check_self(eng, backend, step, tol, 1100)
    finally:
        eng.close()


def test_pinned_database_keeps_no_prefix_popcount_across_tolerances(engine):
    """The pinned database's expansion holds the column popcounts of ONE prefix.  Searches at 350, 120, 350, 400, 120, 1024, 0,
    350 change the prefix in both directions; the candidates carry the structured pairs of every one of those tolerances
    (tail dwords all ones: a popcount left over from a longer prefix raises the threshold and loses their hits)."""
    import torch

    from vid_dup_finder_lib_amd import engine as ve

    order = [350, 120, 350, 400, 120, 1024, 0, 350]
    rng = np.random.default_rng(2024)
    parts = [hg.structured_pairs(rng, tol, hg.tested_dwords(engine.backend, hg.auto_step(tol)), reps=1 if tol < 32 else 2)
             for tol in sorted(set(order))]
    cand = np.concatenate([p.b for p in parts] + [hg.random_hashes(rng, 100)])
    refs_all = np.concatenate([p.a for p in parts])
    cand, refs_all = cand[rng.permutation(len(cand))], refs_all[rng.permutation(len(refs_all))]
    cd = _dur(len(cand))
    tw = torch.from_numpy(cand.view(np.int64).copy()).cuda()
    td = torch.from_numpy(cd.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    engine.pin_database(tw.data_ptr(), len(cand))
    try:
        for k, tol in enumerate(order):
            rw = refs_all[np.random.default_rng(k).choice(len(refs_all), size=700, replace=False)]
            a = torch.from_numpy(rw.view(np.int64).copy()).cuda()
            b = torch.from_numpy(_dur(len(rw)).view(np.int32).copy()).cuda()
            torch.cuda.synchronize()
            hits, n = engine.search_refs_device(tw.data_ptr(), td.data_ptr(), len(cand), a.data_ptr(), b.data_ptr(), len(rw), tol)
            assert n == len(hits)
            want = orc.search_refs_sorted(cand, cd, rw, _dur(len(rw)), tol)
            assert ve.groups_from_ref_hits(hits) == want, (k, tol)
            assert len(want) > 0
    finally:
        engine.pin_database(0, 0)


def _sparse_set():
    rng = np.random.default_rng(700)
    one_bit = np.zeros((400, 1024), np.uint8)
    one_bit[np.arange(400), rng.choice(1024, size=400, replace=False)] = 1  # padding bits among them
    words = np.concatenate([np.zeros((700, hg.HASH_WORDS), np.uint64), np.packbits(one_bit, axis=1, bitorder="little").view(np.uint64)])
    return words[rng.permutation(len(words))], rng.choice(len(words), size=300, replace=False)


def _check_sparse(eng):
    words, pick = _sparse_set()
    d = _dur(len(words))
    for tol in (0, 1, 350):
        assert eng.search_self_sorted(words, d, tol) == orc.search_self_sorted(words, d, tol)
        got = eng.search_refs_sorted(words, d, words[pick], d[pick], tol)
        assert got == orc.search_refs_sorted(words, d, words[pick], d[pick], tol)
        assert sum(len(m) for _, m in got) >= 300


def test_sparse_rows_against_the_padding(engine):
    """700 all-zero hashes and 400 with one set bit (what black or static clips hash to).  The zero rows and columns the
    operands are padded with are at prefix distance <= 1 from every one of them: every padded column is a suspect, and
    only the column bound and the windows keep it out of the result."""
    _check_sparse(engine)


def test_sparse_rows_through_the_suspect_queue_overflow(monkeypatch):
    """The same with a 64-entry suspect queue: every launch overflows and goes through the overflow protocol."""
    import vid_dup_finder_lib_amd as vdf

    monkeypatch.setenv("VDF_CAND_CAPACITY", "64")
    monkeypatch.setenv("VDF_SEARCH_BACKEND", "mfma")
    eng = vdf.Engine(0)
    try:
        _check_sparse(eng)
    finally:
        eng.close()


def test_groups_max_distance_on_complements_padding_and_identical_members(engine):
    """The extremes of the Sorting::Distance key: a group with a complement pair (1024), one whose members differ in the
    padding bits only (24), one of identical members (0) - and each with a reference that is what sets the maximum."""
    rng = np.random.default_rng(78)
    h = hg.random_hashes(rng, 4)
    pad = np.zeros(hg.HASH_WORDS, np.uint64)
    pad[15] = np.uint64(0xFFFFFF) << np.uint64(40)
    ones = np.full(hg.HASH_WORDS, np.uint64(0xFFFFFFFFFFFFFFFF))
    w = np.stack([h[0], ~h[0], h[0],            # 0..2: complement pair + an identical member
                  h[1], h[1] ^ pad, h[1],       # 3..5: padding-only difference
                  h[2], h[2], h[2],             # 6..8: identical
                  np.zeros(hg.HASH_WORDS, np.uint64), ones, pad,  # 9..11: all zero / all 1024 bits / padding only
                  h[3]])
    groups = [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10], [9, 11], [10, 11], [6, 12], [2, 0], [8, 7, 6, 3]]
    brute = lambda hs: max(orc.hamming(hs[i], hs[j]) for i in range(len(hs)) for j in range(i + 1, len(hs)))  # noqa: E731
    want = [brute([w[x] for x in g]) for g in groups]
    assert want[:6] == [1024, 24, 0, 1024, 24, 1000] and want[7] == 0
    assert engine.groups_max_distance(w, groups).tolist() == want
    # with a reference member (contained_paths = duplicates, then the reference)
    rw = np.stack([~h[2], h[2] ^ pad, h[2], ones])
    ref_groups = [[6, 7, 8], [6, 7, 8], [6, 7, 8], [9, 11], [3, 4]]
    ref_index = [0, 1, 2, 3, 1]
    want_r = [brute([w[x] for x in g] + [rw[r]]) for g, r in zip(ref_groups, ref_index)]
    assert want_r[:4] == [1024, 24, 0, 1024]
    assert engine.groups_max_distance(w, ref_groups, ref_hashes=rw, ref_index=ref_index).tolist() == want_r
