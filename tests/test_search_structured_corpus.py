"""The structured pair corpus (hashgen.structured_pairs) and the numpy twin of the search's prefix test, on the CPU.

The GPU tests (test_gpu_search_structured.py) can only show that today's kernels agree with the oracle on this corpus.
What makes that worth something is shown here: for every (backend, step, tolerance) those tests search at, every plausible
slip in the prefix test - modelled as a mutant of the twin - gives a WRONG answer on at least one pair of the corpus, unless
the slip changes nothing at that combination, and then the combination is listed as such below, not skipped.

A pair is reported when the prefix test keeps it AND the exact pass finds it within the tolerance.  A mutant of the prefix
test is wrong on a pair when it drops one that is within the tolerance (the exact pass never sees it: a lost hit); keeping a
pair that is not is harmless, the exact pass decides.  "pad_masked" is the one slip that would sit in the exact pass too
(bits 1000..1023 cleared wherever bits are counted): it reports pairs up to 24 over the tolerance.  Three classes follow:
  identity  the mutant's prefix test computes the same as the original on every input
  harmless  it differs, but only ever keeps more: the reported pairs stay right
  lethal    it must report a wrong set of pairs on the corpus
"""
import functools

import numpy as np
import pytest

import hashgen as hg
from oracle import vdf_oracle as orc

COMBOS = hg.search_combos()


def _id(combo):
    return "%s-step%d-tol%d" % combo


@functools.lru_cache(maxsize=None)
def _case(tol, prefix):
    return hg.refs_case(hg.corpus_rng(tol, prefix), tol, prefix)


@functools.lru_cache(maxsize=None)
def _dist(tol, prefix):
    """[reference, candidate] distances of the case by brute force: computed once, read by every test"""
    case = _case(tol, prefix)
    d = hg.all_distances(case.refs, case.cand)
    d.setflags(write=False)
    return d


def expected_class(mutant, prefix, tol):
    """From the arithmetic alone (never from what the twin returns)."""
    full = len(prefix) == 32
    streamed_not_linear = tuple(prefix) != tuple(range(len(prefix)))
    if mutant == "strict":
        # wrong exactly on a pair whose prefix distance equals min(tol, 1024): the corpus holds one wherever the prefix has that many bits
        return "lethal" if min(tol, 1024) <= 32 * len(prefix) else "identity"
    if mutant == "linear":
        # VALU prefixes and the full hash ARE dwords 0 .. len - 1
        return "lethal" if streamed_not_linear and tol < 1024 else "identity"
    if mutant == "full_pop":
        return "identity" if full else "lethal" if tol < 1024 else "harmless"
    if isinstance(mutant, tuple):
        stale = set(range(mutant[1])) | set(16 + s for s in range(mutant[1]))
        if stale == set(prefix):
            return "identity"  # ("stale", 13) at step 12, ("stale", 7) at step 6, ("stale", 16) on the full hash
        if stale < set(prefix):
            # a column popcount that is too SMALL lowers the threshold: more suspects, no lost hit (from 1024 on every pair is kept anyway)
            return "harmless" if tol < 1024 else "identity"
        assert stale > set(prefix)
        return "lethal" if tol < 1024 else "harmless"
    if mutant == "pad_masked":
        # a pair tol + 1 apart with a differing padding bit is reported; from 1024 on every pair is a hit either way
        return "lethal" if tol < 1024 else "identity"
    if mutant == "tol_unclamped":
        # (pbK - tol) / 2 is an exact f32 half-integer for any tolerance below 2^24, and acc >= -512 passes either way once
        # tol >= 1024: the clamp is arithmetic hygiene, not a decision - identity at EVERY tolerance
        return "identity"
    raise AssertionError(mutant)


def _mutants_for(backend, prefix):
    # the VALU kernel has no precomputed column popcounts that could be stale; its full-length test shares the prefix of
    # the matrix-core step 16 and is covered there
    return [m for m in hg.MUTANTS if not isinstance(m, tuple) or backend == "mfma"]


def test_tested_dwords_table():
    """The prefix per instantiated step, spelled out (hamming.hip: k-step s = dwords s and 16 + s; VALU: 14 / 22 / 26 dwords)."""
    assert hg.tested_dwords("mfma", 6) == (0, 1, 2, 3, 4, 5, 6, 16, 17, 18, 19, 20, 21, 22)
    assert hg.tested_dwords("mfma", 12) == tuple(range(13)) + tuple(range(16, 29))
    assert hg.tested_dwords("mfma", 14) == tuple(range(15)) + tuple(range(16, 31))
    assert [len(hg.tested_dwords("mfma", s)) for s in range(17)] == [14] * 7 + [18] * 2 + [22] * 2 + [24, 26, 28, 30, 32, 32]
    assert [len(hg.tested_dwords("valu", s)) for s in range(17)] == [14] * 7 + [22] * 4 + [26] * 2 + [32] * 4
    assert hg.tested_dwords("valu", 10) == tuple(range(22))
    # the automatic step changes exactly at the edges the GPU tests straddle
    steps = [hg.auto_step(t) for t in range(0, 1100)]
    assert [t for t in range(1, 1100) if steps[t] != steps[t - 1]] == [181, 210, 240, 269, 298, 328, 358, 388, 418]
    assert [e + 1 for e in hg.AUTO_STEP_EDGES] == [t for t in range(1, 1100)
                                                   if hg.tested_dwords("mfma", steps[t]) != hg.tested_dwords("mfma", steps[t - 1])]
    assert (steps[0], steps[181], steps[240], steps[298], steps[328], steps[358], steps[388], steps[418]) == (6, 7, 9, 11, 12, 13, 14, 16)


@pytest.mark.parametrize("combo", COMBOS, ids=_id)
def test_corpus_is_what_it_claims_and_the_twin_keeps_every_hit(combo):
    backend, step, tol = combo
    prefix = hg.tested_dwords(backend, step)
    case = _case(tol, prefix)
    sp = case.pairs
    # distances: against an independent brute force, through the shuffle
    dist = _dist(tol, prefix)
    assert np.array_equal(dist[case.ref_of, case.cand_of], sp.distance)
    assert np.array_equal(sp.distance, [hg.hamming(x, y) for x, y in zip(sp.a, sp.b)])
    # placements: where `exact`, the prefix distance is all of it ("in", and "dword d" for d inside) or none of it ("out")
    sel = sorted(prefix)
    pre = (hg._dword_counts(sp.a ^ sp.b)[:, sel]).sum(1)
    plc = np.array(sp.placement)
    assert np.array_equal(pre[(plc == "in") & sp.exact], sp.distance[(plc == "in") & sp.exact])
    assert not pre[(plc == "out") & sp.exact].any()
    assert set(sp.family) == set(hg.FAMILIES) and sp.salted.any() and not sp.salted.all()
    for where in ("in", "out"):  # both sides of the tolerance, from every base, plain and salted
        for k in {min(tol, 1024), min(tol + 1, 1024)}:
            m = (plc == where) & (sp.distance == k)
            assert {(f, s) for f, s in zip(np.array(sp.family)[m], sp.salted[m])} == {(f, s) for f in hg.FAMILIES for s in (False, True)}
    assert ((plc == "in") & sp.exact & (sp.distance == min(tol, 1024))).any() == (min(tol, 1024) <= 32 * len(prefix))
    if tol < 32:
        assert {p for p in plc if p.startswith("dword")} == {"dword%d" % d for d in range(32)}
    assert (sp.distance[plc == "complement"] == 1024).all()
    # the unmutated twin never drops a hit, and on the full hash it is the decision
    keep = hg.prefix_filter_twin(sp.a, sp.b, prefix, tol)
    hit = sp.distance <= tol
    assert keep[hit].all()
    assert np.array_equal(keep, pre <= tol)
    if len(prefix) == 32:
        assert np.array_equal(keep, hit)
    # ... also on the unplanted hits of the search rectangle (a sample of them: identical bases give tens of thousands)
    rr, cc = np.nonzero(dist <= tol)
    some = np.random.default_rng(tol).permutation(len(rr))[:4000]
    rr, cc = rr[some], cc[some]
    assert hg.prefix_filter_twin(case.refs[rr], case.cand[cc], prefix, tol).all()


@pytest.mark.parametrize("combo", [c for c in COMBOS if c[2] in hg.AUTO_TOLERANCES and c[1] == hg.instantiated_step(c[0], hg.auto_step(c[2]))], ids=_id)
def test_shuffles_put_boundary_pairs_on_every_position_of_a_tile(combo):
    """Pairs exactly on the tolerance (or one over) reach every wave, both 32-row tiles of a wave and both lane groups (the C
    layout's rows 4 g + ...) of a row tile, every 32-column sub-tile of a 128-column stage, the partly padded last row tile
    and the last, partly padded stage - in both modes, and in self mode at both sizes the last row of the set."""
    backend, step, tol = combo
    prefix = hg.tested_dwords(backend, step)

    def covered(rows, cols, tile_rows, n_rows, n_cols):
        assert {(r % tile_rows) // 64 for r in rows} == set(range(tile_rows // 64))
        assert {(r % 64) // 32 for r in rows} == {0, 1} and {(r % 8) // 4 for r in rows} == {0, 1}
        assert {(c % 128) // 32 for c in cols} == {0, 1, 2, 3}
        assert max(rows) >= (n_rows - 1) // tile_rows * tile_rows - (tile_rows if n_rows % tile_rows == 1 else 0)
        assert max(cols) >= (n_cols - 1) // 128 * 128

    case = _case(tol, prefix)
    near = np.abs(case.pairs.distance - min(tol, 1024)) <= 1
    covered(case.ref_of[near], case.cand_of[near], 256, len(case.refs), len(case.cand))
    for n in (1100, 513):
        sc = hg.self_case(hg.corpus_rng(tol, prefix), tol, prefix, n)
        near = np.abs(sc.pairs.distance - min(tol, 1024)) <= 1
        lo, hi = np.minimum(sc.ref_of, sc.cand_of)[near], np.maximum(sc.ref_of, sc.cand_of)[near]
        covered(lo, hi, 512, n, n)
        assert len(sc.cand) == n and max(hi) == n - 1
        assert sorted(np.concatenate([sc.ref_of, sc.cand_of]).tolist()) == sorted(set(np.concatenate([sc.ref_of, sc.cand_of]).tolist()))
        assert all(hg.hamming(sc.cand[i], sc.cand[j]) == d for i, j, d in zip(sc.ref_of[:40], sc.cand_of[:40], sc.pairs.distance[:40]))


@pytest.mark.parametrize("combo", COMBOS, ids=_id)
def test_every_mutant_is_killed_wherever_it_is_not_the_identity(combo):
    backend, step, tol = combo
    prefix = hg.tested_dwords(backend, step)
    sp = _case(tol, prefix).pairs
    hit = sp.distance <= tol
    orig = hg.prefix_filter_twin(sp.a, sp.b, prefix, tol)
    pad = np.uint64((1 << 40) - 1)
    am, bm = sp.a.copy(), sp.b.copy()
    am[:, 15] &= pad
    bm[:, 15] &= pad
    masked_hit = hg._dword_counts(am ^ bm).sum(1) <= tol
    report = {}
    for mutant in _mutants_for(backend, prefix):
        keep = hg.prefix_filter_twin(sp.a, sp.b, prefix, tol, mutant)
        reported = keep & (masked_hit if mutant == "pad_masked" else hit)
        lost, extra = int((hit & ~reported).sum()), int((~hit & reported).sum())
        cls = expected_class(mutant, prefix, tol)
        report[str(mutant)] = (cls, lost, extra)
        if cls == "identity":
            assert np.array_equal(keep, orig) and lost == 0 and extra == 0, (mutant, combo)
        elif cls == "harmless":
            assert lost == 0 and extra == 0 and (keep & ~orig).any() and not (orig & ~keep).any(), (mutant, combo)
        else:
            assert lost + extra > 0, (mutant, combo)
    print(_id(combo), report)


def test_identity_combinations_are_these():
    """The combinations at which a mutant cannot be told from the original, listed (a change to the grid shows up here)."""
    ident = {}
    for backend, step, tol in COMBOS:
        prefix = hg.tested_dwords(backend, step)
        for mutant in _mutants_for(backend, prefix):
            if expected_class(mutant, prefix, tol) != "lethal":
                ident.setdefault(str(mutant), set()).add((backend, len(prefix), expected_class(mutant, prefix, tol)))
    full_tols = sorted({tol for b, s, tol in COMBOS if len(hg.tested_dwords(b, s)) == 32})
    assert 418 in full_tols and 1024 in full_tols
    assert ident == {
        # strict is lethal everywhere: every combination has a pair exactly min(tol, 1024) apart inside the prefix
        "linear": {("valu", 14, "identity"), ("valu", 22, "identity"), ("valu", 26, "identity"), ("valu", 32, "identity"),
                   ("mfma", 32, "identity")},
        "full_pop": {("valu", 32, "identity"), ("mfma", 32, "identity")},
        "('stale', 7)": {("mfma", 14, "identity"), ("mfma", 32, "identity")} | {("mfma", n, "harmless") for n in (18, 22, 24, 26, 28, 30, 32)},
        "('stale', 13)": {("mfma", 26, "identity"), ("mfma", 32, "identity")} | {("mfma", n, "harmless") for n in (28, 30, 32)},
        "('stale', 16)": {("mfma", 32, "identity")},
        # pad_masked: only at tolerances >= 1024 (nothing to reject), which the full-length test serves
        "pad_masked": {("valu", 32, "identity"), ("mfma", 32, "identity")},
        "tol_unclamped": {(b, n, "identity") for b in ("mfma", "valu") for n in (14, 18, 22, 24, 26, 28, 30, 32) if (b, n) not in
                          (("valu", 18), ("valu", 24), ("valu", 28), ("valu", 30))},
    }


@pytest.mark.parametrize("combo", COMBOS, ids=_id)
def test_oracle_refs_search_returns_exactly_the_pairs_within_tolerance(combo):
    """The expected value of the GPU tests: the oracle's search_with_references on the corpus = every (reference, candidate)
    at <= tol by brute force, the planted pairs among them - no pair is left out of a comparison."""
    backend, step, tol = combo
    prefix = hg.tested_dwords(backend, step)
    case = _case(tol, prefix)
    dur_c, dur_r = np.full(len(case.cand), 100, np.uint32), np.full(len(case.refs), 100, np.uint32)
    got = orc.search_refs_sorted(case.cand, dur_c, case.refs, dur_r, tol)
    dist = _dist(tol, prefix)
    want = [(r, np.flatnonzero(dist[r] <= tol).tolist()) for r in range(len(case.refs)) if (dist[r] <= tol).any()]
    assert got == want
    pairs = {(r, c) for r, m in got for c in m}
    planted = set(zip(case.ref_of.tolist(), case.cand_of.tolist()))
    assert {p for p, d in zip(zip(case.ref_of.tolist(), case.cand_of.tolist()), case.pairs.distance) if d <= tol} == pairs & planted


def test_measure_mutant_losses_on_iid_planted_set():
    """A measurement, not a check (DESIGN.md 4.3 quotes it): how many of the true hits of the largest iid planted set of
    test_gpu_search_parity.py each mutant loses at the matrix-core prefix of tolerances 350 and 120.  Only the unmutated twin
    is asserted."""
    words, dur = hg.planted_set(np.random.default_rng(12), 20000, n_clusters=400, durations="zero")
    res = orc.search_refs_sorted(words, dur, words, dur, 350)  # every pair within 350, once
    rows = np.array([r for r, m in res for c in m if c > r], np.int64)
    cols = np.array([c for r, m in res for c in m if c > r], np.int64)
    dist = hg._dword_counts(words[rows] ^ words[cols]).sum(1)
    for tol in (350, 120):
        a, b = words[rows[dist <= tol]], words[cols[dist <= tol]]
        prefix = hg.tested_dwords("mfma", hg.auto_step(tol))
        assert hg.prefix_filter_twin(a, b, prefix, tol).all()
        lost = {str(m): int((~hg.prefix_filter_twin(a, b, prefix, tol, m)).sum()) for m in hg.MUTANTS}
        print("planted_set(n=20000, seed 12), tol %d, %d dwords: %d hits; lost per mutant: %s" % (tol, len(prefix), len(a), lost))
