"""api.align_retimed on the host forms (engine=None, inputs under ALIGN_HOST_CELLS; no GPU) against a brute-force numpy twin written from its definition
(tests/retimedgen.py: every pair, every phase, every start, cells (ka + num m, kb + den m)).  Corpus: six videos of noise frames at 16 x 16 hashed by the
oracle - two sources and four files at den / num of their frames, B[j] = A[c + (j * num) // den]: excerpts from c = 0, 7 and 13, one file with two excerpts,
one unrelated.  The records must be the twin's field for field, at mean distance 0 on the excerpts - and the plain windows of the same files, aligned on
diagonals, must NOT see the excerpts: that blindness is what the retimed windows are for.  At 6/5 plain windows do match in fragments at tolerance 0.35
(five of six frames are shared and a window drifts by one frame in six), so there the blindness is asserted at 0.2."""
import numpy as np
import pytest

import retimedgen
import windowgen

SEED = {(6, 5): 65, (3, 2): 32, (2, 1): 21}
PLAIN_TOLERANCE = {(6, 5): 0.2, (3, 2): 0.35, (2, 1): 0.35}
_CACHE = {}


def hashed(rate):
    """(windows_a retimed at `rate`, windows_b plain, plain windows of A, their words) as lists of VideoHash lists - oracle hashes, made once per rate."""
    import vid_dup_finder_lib_amd as vdf

    if rate not in _CACHE:
        A, B = retimedgen.corpus(rate, SEED[rate])
        wa = [retimedgen.oracle_windows(v, rate)[0] for v in A]
        wb = [windowgen.oracle_windows(v, 1)[0] for v in B]
        wa_plain = [windowgen.oracle_windows(v, 1)[0] for v in A]
        mk = lambda ws, tag: [[vdf.VideoHash(w, f"{tag}{i}", 10 + i) for w in words] for i, words in enumerate(ws)]
        _CACHE[rate] = (mk(wa, "a"), mk(wb, "b"), mk(wa_plain, "a"), wa, wb)
    return _CACHE[rate]


def _fields(recs):
    return [tuple(r[:10]) for r in recs]


@pytest.mark.parametrize("rate", sorted(SEED))
def test_align_retimed_equals_the_brute_force_twin_and_finds_every_excerpt(rate):
    import vid_dup_finder_lib_amd as vdf

    num, den = rate
    va, vb, _, wa, wb = hashed(rate)
    for tolerance, min_run in ((0.35, 1), (0.35, 2), (0.0, 2)):
        got = vdf.align_retimed(va, vb, rate, tolerance, min_run=min_run)
        want = retimedgen.align_retimed_twin(wa, wb, rate, vdf.engine.tolerance_int(tolerance), min_run)
        assert _fields(got) == want, (rate, tolerance, min_run)
        by_pair = {(r.a, r.b): r for r in got}
        assert set(retimedgen.EXCERPTS) <= set(by_pair)
        for (a, b), (c, fb0, nb) in retimedgen.EXCERPTS.items():
            r = by_pair[(a, b)]
            assert (r.num, r.den) == rate and r.path_a == f"a{a}" and r.path_b == f"b{b}"
            if tolerance > 0 and b == 2:
                continue  # beside other content a window with a few foreign frames is still within 0.35: the run is longer than the excerpt, at a distance
            n = (nb - 16) // den + 1  # the windows of b at multiples of den that lie inside the excerpt (fb0 is one)
            assert r.mean_distance == 0 and (r.first_frame_a, r.first_frame_b, r.n_windows) == (c, fb0, n), (rate, a, b, r)
            assert r.n_frames_a == (n - 1) * num + retimedgen.span(rate) and r.n_frames_b == (n - 1) * den + 16
        if tolerance == 0.0:
            assert sorted(by_pair) == sorted(retimedgen.EXCERPTS)  # nothing else is an exact copy: the unrelated file pairs with nothing
    # a rate that is not in lowest terms is the same rate
    assert vdf.align_retimed(va, vb, (2 * num, 2 * den), 0.35, min_run=2) == vdf.align_retimed(va, vb, rate, 0.35, min_run=2)


@pytest.mark.parametrize("rate", sorted(SEED))
def test_plain_windows_on_diagonals_do_not_see_the_excerpts(rate):
    import vid_dup_finder_lib_amd as vdf

    _, vb, va_plain, _, _ = hashed(rate)
    plain = vdf.align(va_plain, vb, PLAIN_TOLERANCE[rate], min_run=2)
    assert not [(r.a, r.b) for r in plain if (r.a, r.b) in retimedgen.EXCERPTS], (rate, plain)


def test_static_flags_are_subsampled_with_the_windows():
    import vid_dup_finder_lib_amd as vdf

    rate = (3, 2)
    va, vb, _, wa, wb = hashed(rate)
    sa = [np.zeros(len(w), np.uint8) for w in va]
    sb = [np.zeros(len(w), np.uint8) for w in vb]
    sb[0][4] = 1  # window 4 of b0 abstains: the stretch of (0, 0) is cut in two at sub-sampled window 2
    got = {(r.a, r.b): r for r in vdf.align_retimed(va, vb, rate, 0.0, static_a=sa, static_b=sb)}
    whole = {(r.a, r.b): r for r in vdf.align_retimed(va, vb, rate, 0.0)}
    assert whole[(0, 0)].n_windows == 13 and (got[(0, 0)].first_frame_b, got[(0, 0)].n_windows) == (6, 10)
    assert got[(1, 1)] == whole[(1, 1)]


def test_argument_errors():
    import vid_dup_finder_lib_amd as vdf

    va, vb, _, _, _ = hashed((3, 2))
    for bad in ((33, 32), (1, 2), (5, 2), (3, 0), (0, 0), 1.5, (3,)):
        with pytest.raises(ValueError):
            vdf.align_retimed(va, vb, bad, 0.35)
    assert vdf.align_retimed([], vb, (3, 2), 0.35) == [] and vdf.align_retimed(va, [], (3, 2), 0.35) == []
