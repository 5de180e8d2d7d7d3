"""Shared by the tests of the align call over (rate, a, b) triples (vdf_align_windows_rates*): the twin of the definition in
include/vdf.h and the problems both the CPU test of the _host form and the GPU test of the kernel solve.  numpy and the generators of the calls
this one is made of - tests/seedrategen.py (the layout and the candidate set), tests/retimedaligngen.py (the twin of one rate and its plants),
tests/aligngen.py, tests/hashgen.py - nothing is imported from the library.  Records are compared for equality.

The twin: per rate r, retimedaligngen.align_retimed_twin on seedrategen.block(p, r) against B, every record tagged with r and
n_frames_b = (n_windows - 1) den + 16, concatenated in rate order.

Problems are seedrategen.Problem.  Unlike seedrategen._layout, which repeats one row of window counts, the window counts here DIFFER PER RATE, as
real hash output does (n_win_r = F - span_r + 1): a kernel that reads the wrong row of a_first then walks the wrong windows."""
from __future__ import annotations

import functools

import numpy as np

import aligngen
import hashgen
import retimedaligngen as rgen
import seedrategen as sgen
from seedrategen import Problem, reduced

USUAL_RATES = sgen.USUAL_RATES
FIELDS = ("a", "b", "rate", "first_a", "first_b", "n_windows", "dist_sum", "n_frames_b")


def span(rate) -> int:
    num, den = reduced(rate)
    return (15 * num) // den + 1


def window_counts(frames, rate) -> list:
    """what a hash call leaves of videos of `frames` frames at `rate`, stride 1 (a video shorter than the span: none)"""
    return [max(0, int(f) - span(rate) + 1) for f in frames]


def layout(rng, rates, counts_a, cb, a_base=0, b_base=0, tol=350, min_run=1) -> Problem:
    """random hashes in the calls' layout; counts_a[r]: the window counts of A's videos in block r; every block of A begins a_base rows into its
    rows (a_first[r, 0] = a_base) and B b_base rows into its array"""
    assert len(counts_a) == len(rates) and len({len(c) for c in counts_a}) == 1
    a_first = np.stack([a_base + aligngen.first_of(c) for c in counts_a]).astype(np.uint32)
    a_rate_first = np.zeros(len(rates) + 1, np.int64)
    a_rate_first[1:] = np.cumsum([a_base + int(sum(c)) for c in counts_a])
    b_first = (b_base + aligngen.first_of(cb)).astype(np.uint32)
    return Problem(hashgen.random_hashes(rng, int(a_rate_first[-1])), a_first, a_rate_first, hashgen.random_hashes(rng, int(b_first[-1])), b_first,
                   tuple(rates), tol, min_run)


def _absolute(p: Problem, r: int) -> rgen.Problem:
    """block r over the WHOLE arrays of p (views, so a plant lands in p): a_first counts rows of p.a_hashes"""
    return rgen.Problem(p.a_hashes, (int(p.a_rate_first[r]) + p.a_first[r].astype(np.int64)), p.b_hashes, p.b_first, p.rates[r], p.tol, p.min_run)


def plant(rng, p: Problem, r, a, b, phase, i0, j0, n, flips=0):
    """retimedaligngen.plant into triple (r, a, b): row den (j0 + m) of b := row phase + num (i0 + m) of video a of block r, `flips` bits changed.
    B is shared by the rates: plants of different triples of one b must use different rows of it."""
    rgen.plant(rng, _absolute(p, r), a, b, phase, i0, j0, n, flips)


def block_problem(p: Problem, r: int) -> rgen.Problem:
    ah, af, ak = sgen.block(p, r)
    return rgen.Problem(ah, af, p.b_hashes, p.b_first, p.rates[r], p.tol, p.min_run, ak, p.b_skip)


def all_triples(p: Problem) -> list:
    n_a, n_b = p.a_first.shape[1] - 1, len(p.b_first) - 1
    return [(r, a, b) for r in range(len(p.rates)) for a in range(n_a) for b in range(n_b) if not (p.exclude_same and a == b)]


def twin(p: Problem, triples=None) -> list:
    """-> the records [(a, b, rate, first_a, first_b, n_windows, dist_sum, n_frames_b)] in (rate, a, b) order; triples: only these (rate, a, b),
    None: all of them (without a == b under exclude_same)"""
    triples = all_triples(p) if triples is None else [tuple(int(x) for x in t) for t in triples]
    out = []
    for r in range(len(p.rates)):
        pairs = [(a, b) for rr, a, b in triples if rr == r]
        if not pairs:
            continue
        den = reduced(p.rates[r])[1]
        for a, b, fa, fb, n, s in rgen.align_retimed_twin(block_problem(p, r), pairs=pairs):
            out.append((a, b, r, fa, fb, n, s, (n - 1) * den + 16))
    return out


def candidates(p: Problem) -> list:
    """the candidate set of the seed call as (rate, a, b): what seed = 1 walks"""
    return [(r, a, b) for a, b, r in sgen.seed_rates_twin(p)]


def records(rec) -> list:
    """a structured array of the library's (ALIGN_RATE_DTYPE) as the twin's tuples"""
    return [tuple(int(x[k]) for k in FIELDS) for x in rec]


def triple_array(triples) -> np.ndarray:
    """(rate, a, b) tuples as [n, 3] integers, the form Engine.align_windows_rates takes beside the seed call's own records"""
    return np.asarray(list(triples), dtype=np.int64).reshape(-1, 3)


# ---- the problems -----------------------------------------------------------------------------------------------------------------------
MIXED_RATES = ((1, 1), (3, 2), (6, 5), (32, 17))
MIXED_COUNTS = ([1, 2, 3, 130], [1, 3, 2, 131], [1, 2, 4, 129], [1, 4, 2, 130])   # per rate: the same videos, other window counts
MIXED_LIST = ((0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0),      # four triples of one unit each: ONE workgroup, four rates
              (3, 0, 1), (3, 1, 1), (3, 3, 0), (3, 3, 2))       # and a few more at the last rate, one with 32 phases of one band


def _mixed(a_base=0, b_base=0, skips=False):
    """Four rates whose units meet in one workgroup: videos of 1, 2, 3 and 130 windows (give or take, per rate) against 1, 2 and 129.  Units per
    triple run from 1 (1 x 1 windows) to 5 (1/1: 258 diagonals) and 3 x 2 (3/2); at 32/17 a video of 4 windows has 28 empty phases."""
    rng = np.random.default_rng([91, 1, a_base, b_base, int(skips)])
    p = layout(rng, MIXED_RATES, MIXED_COUNTS, [1, 2, 129], a_base, b_base, tol=350, min_run=1)
    for r in range(len(MIXED_RATES)):   # window 0 of video 0 of every block is window 0 of video 0 of B: a record per rate from a 1 x 1 matrix
        p.a_hashes[int(p.a_rate_first[r]) + int(p.a_first[r, 0])] = p.b_hashes[int(p.b_first[0])]
    # one line per rate in (r, 3, 2), on rows of B that no other plant uses: 60 .. 67 | 0, 2, .. 18 | 30, 35, .. 50 | 85, 102, 119
    plant(rng, p, 0, 3, 2, 0, 40, 60, 8, (0, 30))
    plant(rng, p, 1, 3, 2, 2, 5, 0, 10, (0, 30))
    plant(rng, p, 2, 3, 2, 4, 3, 6, 5, (0, 30))
    plant(rng, p, 3, 3, 2, 7, 1, 5, 3, (0, 30))
    if skips:
        a_skip, b_skip = np.zeros(len(p.a_hashes), np.uint8), np.zeros(len(p.b_hashes), np.uint8)
        a_skip[rng.random(len(a_skip)) < 0.03] = 7
        b_skip[rng.random(len(b_skip)) < 0.03] = 255
        den = 2
        b_skip[int(p.b_first[2]) + den * 4] = 1     # cuts the 3/2 line in two: 4 | 5
        a_skip[int(p.a_rate_first[0]) + int(p.a_first[0, 3]) + 43] = 1   # and the 1/1 line: 3 | 4
        p = p._replace(a_skip=a_skip, b_skip=b_skip)
    return p


def _bands3():
    """Three bands: 200 x 130 windows at 3/2 (sub-matrices 67 x 65: 131 diagonals) in slot 1, tolerance 500 - about every second cell a match"""
    rng = np.random.default_rng([91, 2])
    return layout(rng, ((1, 1), (3, 2)), ([7, 3], [200, 2]), [130, 0, 5], tol=500, min_run=2)


PLANTED_RATES = ((3, 2), (6, 4), (3, 2), (9, 6), (12, 8), (15, 10), (30, 20), (24, 16))   # all 3/2: retimedaligngen._planted's geometry, a slot per line


def _planted(min_run):
    """DESIGN 4.17's planted lines - the four edges, the last diagonal of band 0 and the first of band 1, a run split by one miss, distances tol
    and tol + 1, runs of 5 under min_run 5 and 6, the main diagonal - line i in triple (i, i, i): each in a different rate slot.  Blocks of
    200 windows in the planted videos (v == r), 200 .. 202 in the others."""
    rng = np.random.default_rng([91, 3, min_run])
    p = layout(rng, PLANTED_RATES, [[200 if v == r else 200 + (r + v) % 3 for v in range(8)] for r in range(8)], [130] * 8, tol=350, min_run=min_run)
    t = p.tol
    plant(rng, p, 0, 0, 0, 1, 0, 10, 5, (0, 30))
    plant(rng, p, 0, 0, 0, 2, 61, 30, 5, (0, 30))
    plant(rng, p, 1, 1, 1, 0, 20, 0, 6, (0, 30))
    plant(rng, p, 1, 1, 1, 1, 12, 59, 6, (0, 30))
    plant(rng, p, 2, 2, 2, 0, 30, 27, 7, 3)
    plant(rng, p, 2, 2, 2, 0, 45, 43, 7, 2)
    plant(rng, p, 3, 3, 3, 1, 30, 27, 7, 2)
    plant(rng, p, 3, 3, 3, 1, 45, 43, 7, 3)
    plant(rng, p, 4, 4, 4, 2, 10, 20, 11, 4)
    p.b_hashes[int(p.b_first[4]) + 2 * 25] = hashgen.random_hashes(rng, 1)[0]
    plant(rng, p, 5, 5, 5, 0, 8, 9, 1, t)
    plant(rng, p, 5, 5, 5, 1, 40, 3, 1, t + 1)
    plant(rng, p, 6, 6, 6, 1, 50, 50, 5, (0, 30))
    plant(rng, p, 7, 7, 7, 0, 0, 0, 65, (0, 40))
    return p


def _tie_trap():
    """retimedaligngen._tie_trap (6/5: level 1 and level 2 of the reduction disagree with one comparator) in slot 2 of a five-rate list"""
    rng = np.random.default_rng([91, 4])
    rates = ((1, 1), (2, 1), (6, 5), (3, 2), (5, 4))
    p = layout(rng, rates, [[90 + r - 2, 90, 90 - (r - 2)] if r != 2 else [90, 90, 90] for r in range(5)], [80, 80, 80], tol=350)
    for a, ph, i0, j0 in ((0, 2, 9, 6), (0, 2, 4, 11), (0, 4, 7, 0), (1, 1, 5, 2), (1, 3, 4, 9), (2, 0, 6, 1), (2, 5, 6, 10)):
        plant(rng, p, 2, a, a, ph, i0, j0, 4)
    return p


def _twins(rate_a, rate_b):
    """the same block twice, under a rate and under an unreduced spelling of it, with a third rate between them: equal records in two slots"""
    rng = np.random.default_rng([91, 5, rate_a[0]])
    q = layout(rng, (rate_a, (1, 1)), ([70, 5, 40], [9, 9, 9]), [60, 9], tol=350, min_run=2)
    num, den = reduced(rate_a)
    plant(rng, q, 0, 0, 0, 3 % num, 0, 0, min((70 - 4) // num + 1, 59 // den + 1), (0, 20))
    plant(rng, q, 0, 2, 1, 1 % num, 0, 0, min(39 // num, 8 // den + 1), 5)
    lo, hi = int(q.a_rate_first[0]), int(q.a_rate_first[1])
    a_hashes = np.concatenate([q.a_hashes, q.a_hashes[lo:hi]])
    return q._replace(a_hashes=a_hashes, a_first=np.concatenate([q.a_first, q.a_first[:1]]),
                      a_rate_first=np.concatenate([q.a_rate_first, [len(a_hashes)]]), rates=(rate_a, (1, 1), rate_b))


def _dense():
    """all hashes equal: every triple of non-empty videos has a record, whole diagonals are runs, ties everywhere"""
    rng = np.random.default_rng([91, 6])
    h = hashgen.random_hashes(rng, 1)
    p = layout(rng, ((1, 1), (3, 2), (6, 5)), ([70, 64, 1], [66, 65, 3], [71, 2, 7]), [65, 40, 1], tol=350, min_run=2)
    return p._replace(a_hashes=np.repeat(h, len(p.a_hashes), axis=0), b_hashes=np.repeat(h, len(p.b_hashes), axis=0))


def _square():
    """a library against itself at two rates: the diagonal triples all have records, exclude_same drops them"""
    q = sgen.square()
    return q._replace(exclude_same=True)


def random_problem(rng) -> Problem:
    """One seeded random problem: 1 .. 8 rates, at most 6 x 6 videos of at most 150 windows, window counts that differ per rate, random bases and
    skip bytes, planted stretches along each rate's slope with 0 .. tol + 40 bits flipped."""
    pool = [(1, 1), (2, 1), (3, 2), (5, 4), (6, 5), (4, 3), (6, 4), (2, 2), (31, 16), (32, 17), (64, 34)]
    rates = tuple(pool[int(i)] for i in rng.integers(0, len(pool), size=int(rng.integers(1, 9))))
    n_a, n_b = int(rng.integers(1, 7)), int(rng.integers(1, 7))
    frames = rng.integers(0, 166, size=n_a)
    counts_a = [[min(150, c) for c in window_counts(frames + int(rng.integers(0, 20)), rate)] for rate in rates]
    cb = [int(rng.integers(0, 151)) for _ in range(n_b)]
    p = layout(rng, rates, counts_a, cb, int(rng.integers(0, 7)), int(rng.integers(0, 7)), tol=int(rng.choice([150, 250, 350, 400])),
               min_run=int(rng.integers(1, 5)))
    for _ in range(int(rng.integers(2, 14))):
        r = int(rng.integers(0, len(rates)))
        num, den = reduced(rates[r])
        a, b = int(rng.integers(0, n_a)), int(rng.integers(0, n_b))
        if counts_a[r][a] == 0 or cb[b] == 0:
            continue
        ka, kb = int(rng.integers(0, counts_a[r][a])), int(rng.integers(0, cb[b]))
        for m in range(int(rng.integers(1, 9))):
            if ka + num * m < counts_a[r][a] and kb + den * m < cb[b]:
                row_a = int(p.a_rate_first[r]) + int(p.a_first[r, a]) + ka + num * m
                p.a_hashes[row_a] = aligngen.flipped(p.b_hashes[int(p.b_first[b]) + kb + den * m], int(rng.integers(0, p.tol + 41)), rng)
    a_skip = (rng.random(len(p.a_hashes)) < 0.1).astype(np.uint8) if rng.random() < 0.6 else None
    b_skip = (rng.random(len(p.b_hashes)) < 0.1).astype(np.uint8) if rng.random() < 0.6 else None
    return p._replace(a_skip=a_skip, b_skip=b_skip)


CASES = {
    "mixed": _mixed,
    "mixed_offsets": functools.partial(_mixed, 5, 3, True),
    "bands3": _bands3,
    **{f"planted_min_run_{m}": functools.partial(_planted, m) for m in (1, 5, 6)},
    "tie_trap": _tie_trap,
    "twins_6_5": functools.partial(_twins, (6, 5), (12, 10)),
    "twins_32_17": functools.partial(_twins, (32, 17), (64, 34)),
    "square": _square,
    "dense": _dense,
}
PLANTED = ("mixed", "mixed_offsets", "planted_min_run_1", "planted_min_run_5", "planted_min_run_6", "tie_trap", "twins_6_5", "twins_32_17", "square")
# the cases the GPU test runs with seed = 1: their candidate sets are small beside their triples (dense excepted); the CPU test runs seed = 1 on all
SEEDED = ("planted_min_run_1", "planted_min_run_5", "planted_min_run_6", "tie_trap", "square", "dense")


@functools.lru_cache(maxsize=None)
def case(name: str) -> Problem:
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name: str) -> tuple:
    return tuple(twin(case(name)))


@functools.lru_cache(maxsize=None)
def expected_candidates(name: str) -> tuple:
    return tuple(candidates(case(name)))


def n_triples(p: Problem) -> int:
    return len(all_triples(p))


def check_non_vacuous(name: str):
    """The conditions the cases must meet, on the twin's own output: every case has a record; every case but the dense one has a triple without
    one; the mixed cases have records in at least three slots; the twin's candidate set of a seeded case is under one tenth of all triples,
    except in the dense case."""
    p, want = case(name), expected(name)
    assert len(want) >= 1, name
    if name != "dense":
        assert len(want) < n_triples(p), name
    if name.startswith("mixed"):
        assert len({w[2] for w in want}) >= 3, name
    if name in SEEDED and name != "dense":
        assert 10 * len(expected_candidates(name)) < n_triples(p), (name, len(expected_candidates(name)), n_triples(p))
