"""align_rates and best_rates on the CPU: "which of my videos is a retimed copy of which, at which of these rates".  The corpus is
retimedgen.corpus(true, 7) for each true rate in 6/5, 5/4, 3/2, 2/1 - two sources A, four files B at den / num of the sources' frames - the windows are
the oracle's at each of the five candidate rates (what hash_frame_windows(rates=) returns on the GPU), tolerance 0.35, min_run 2.  align_rates must be
the brute-force twin per rate, best_rates must name the TRUE rate on all four excerpt pairs, and the unrelated file B3 gets no record.  The wrong rates
do produce records for the excerpt pairs - asserted below - so the ranking decides something."""
import pytest

import retimedgen
import windowgen

CANDIDATES = [(1, 1), (6, 5), (5, 4), (3, 2), (2, 1)]
TRUE = [(6, 5), (5, 4), (3, 2), (2, 1)]
TOLERANCE, MIN_RUN = 0.35, 2
_CACHE, _WRONG = {}, {}


def hashed(true):
    """({rate: windows of A}, windows of B, {rate: oracle words of A}, oracle words of B) of the corpus whose copies run at `true`"""
    import vid_dup_finder_lib_amd as vdf

    if true not in _CACHE:
        A, B = retimedgen.corpus(true, 7)
        wa = {r: [retimedgen.oracle_windows(v, r)[0] for v in A] for r in CANDIDATES}
        wb = [windowgen.oracle_windows(v, 1)[0] for v in B]
        mk = lambda ws, tag: [[vdf.VideoHash(w, f"{tag}{i}", 10 + i) for w in words] for i, words in enumerate(ws)]
        _CACHE[true] = ({r: mk(wa[r], "a") for r in CANDIDATES}, mk(wb, "b"), wa, wb)
    return _CACHE[true]


@pytest.mark.parametrize("true", TRUE)
def test_align_rates_is_the_twin_per_rate(true):
    import vid_dup_finder_lib_amd as vdf

    va, vb, wa, wb = hashed(true)
    got = vdf.align_rates(va, vb, TOLERANCE, MIN_RUN)
    assert list(got) == CANDIDATES
    for r in CANDIDATES:
        assert [tuple(x[:10]) for x in got[r]] == retimedgen.align_retimed_twin(wa[r], wb, r, vdf.engine.tolerance_int(TOLERANCE), MIN_RUN), (true, r)
        assert got[r] == vdf.align_retimed(va[r], vb, r, TOLERANCE, min_run=MIN_RUN), (true, r)  # native=True is align_rates' default: the composition's list


@pytest.mark.parametrize("true", TRUE)
def test_best_rates_names_the_true_rate_on_every_excerpt(true):
    import vid_dup_finder_lib_amd as vdf

    va, vb, _, _ = hashed(true)
    result = vdf.align_rates(va, vb, TOLERANCE, MIN_RUN)
    best = vdf.best_rates(result, TOLERANCE)
    assert [(r.a, r.b) for r in best] == sorted((r.a, r.b) for r in best) and len({(r.a, r.b) for r in best}) == len(best)
    by_pair = {(r.a, r.b): r for r in best}
    assert not any(b == 3 for _, b in by_pair), "the unrelated file got a record"
    wrong = 0
    for pair in retimedgen.EXCERPTS:
        r = by_pair[pair]
        assert (r.num, r.den) == true, (true, pair, r)
        assert r in result[true]
        for other in CANDIDATES:
            for x in result[other]:
                if other != true and (x.a, x.b) == pair:
                    wrong += 1
                    # (on this corpus the mean distances are 0 ... 85.25 at the true rate and 192 ... 345 at the nearest wrong one)
                    assert x.mean_distance > r.mean_distance, (true, other, x)
    _WRONG[true] = wrong


def test_the_wrong_rates_do_produce_records():
    """the ranking of best_rates decides something: summed over the four corpora, rates other than the true one have records for the excerpt pairs"""
    for true in TRUE:
        if true not in _WRONG:
            test_best_rates_names_the_true_rate_on_every_excerpt(true)
    assert sum(_WRONG.values()) >= 1, _WRONG


def test_best_rates_score_and_ties():
    import vid_dup_finder_lib_amd as vdf

    R = vdf.RetimedAlignment
    # frames of B covered x margin: 3/2 covers 36 frames of B at distance 10 (36 * 341), 1/1 covers 20 at distance 0 (20 * 351); n_windows would say 1/1
    a = R(0, 1, 1, 1, 0, 0, 20, 20, 5, 0.0)
    b = R(0, 1, 3, 2, 0, 0, 37, 36, 11, 10.0)
    c = R(2, 0, 6, 5, 0, 0, 19, 16, 1, 0.0)
    assert vdf.best_rates({(1, 1): [a], (3, 2): [b, c]}, 0.35) == [b, c]
    assert vdf.best_rates({(3, 2): [b, c], (1, 1): [a]}, 0.35) == [b, c]
    # a tie goes to the rate that comes first in the caller's list
    t1, t2 = R(0, 0, 1, 1, 0, 0, 16, 16, 1, 0.0), R(0, 0, 6, 5, 3, 0, 19, 16, 1, 0.0)
    assert vdf.best_rates({(1, 1): [t1], (6, 5): [t2]}, 0.35) == [t1] and vdf.best_rates({(6, 5): [t2], (1, 1): [t1]}, 0.35) == [t2]
    assert vdf.best_rates({}, 0.35) == [] and vdf.best_rates({(1, 1): []}, 0.35) == []
