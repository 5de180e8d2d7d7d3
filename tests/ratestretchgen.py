"""Shared by the tests of the stretches call over (rate, a, b) triples (vdf_align_windows_rates_stretches*): a numpy twin of the
definition in include/vdf.h, independent of the C++, and the problems both the CPU test of the _host form and the GPU test of the masked rates
kernel solve.  numpy and the generators of the calls this one is made of - tests/ratealigngen.py (the layout and the plants), tests/retimedaligngen.py
(the runs of a sub-matrix and the two-level reduction), tests/hashgen.py - nothing is imported from the library.  Records are compared for equality.

The twin, per triple: the brute-force distance matrix of video a of block r against video b; a boolean mask of the same shape, IN THE ROWS OF THE
TWO VIDEOS; per rank the runs of every phase's sub-matrix dist[p::num, 0::den] on the cells that are ok and not masked, the phase-bests and the
two-level reduction; then the record's rectangle - rows [first_a - ga, first_a + num (n - 1) + 1 + ga) x [first_b - guard, first_b + den (n - 1) + 1
+ guard), clipped, ga = ceil(guard num / den) - is set in the mask.  own_phase_only: the WRONG masking, which sets only the rows of the record's own
phase - the phase trap uses it to show that it would be caught.

A case is (problem, max_stretches, guard)."""
from __future__ import annotations

import functools

import numpy as np

import aligngen
import hashgen
import ratealigngen as gen
import retimedaligngen as rgen
from seedrategen import Problem, reduced

FIELDS = gen.FIELDS + ("rank",)


def rect_of(first_a, first_b, n, rate, guard, Na, Nb):
    """-> (a_lo, a_hi, b_lo, b_hi) in rows of the two videos; python integers, nothing wraps"""
    num, den = rate
    ga = -(-guard * num // den)
    return (max(0, first_a - ga), min(Na, first_a + num * (n - 1) + 1 + ga), max(0, first_b - guard), min(Nb, first_b + den * (n - 1) + 1 + guard))


def triple_stretches(dist, ok, rate, tol, min_run, max_stretches, guard, own_phase_only=False):
    """dist, ok [Na, Nb] of one triple -> [(first_a, first_b, n_windows, dist_sum, rank)]"""
    num, den = rate
    Na, Nb = dist.shape
    masked = np.zeros((Na, Nb), bool)
    out = []
    for rank in range(max_stretches):
        rec = rgen.two_level(rgen.pair_runs(dist, ok & ~masked, rate, tol, min_run), rate)
        if rec is None:
            break
        fa, fb, n, s = (int(x) for x in rec)
        out.append((fa, fb, n, s, rank))
        a_lo, a_hi, b_lo, b_hi = rect_of(fa, fb, n, rate, guard, Na, Nb)
        if own_phase_only:
            rows = np.arange(a_lo, a_hi)
            rows = rows[rows % num == fa % num]
            masked[rows[:, None], np.arange(b_lo, b_hi)[None, :]] = True
        else:
            masked[a_lo:a_hi, b_lo:b_hi] = True
    return out


def twin(p: Problem, max_stretches, guard, triples=None, own_phase_only=False) -> list:
    """-> the records [(a, b, rate, first_a, first_b, n_windows, dist_sum, n_frames_b, rank)] in (rate, a, b, rank) order; triples: only these
    (rate, a, b), None: all of them (without a == b under exclude_same)"""
    triples = gen.all_triples(p) if triples is None else [tuple(int(x) for x in t) for t in triples]
    tol = min(int(p.tol), 1024)
    out = []
    for r in range(len(p.rates)):
        mine = [(a, b) for rr, a, b in triples if rr == r]
        if not mine:
            continue
        q = gen.block_problem(p, r)
        rate = reduced(p.rates[r])
        dist, ok = rgen._cells(q)
        for a, b in mine:
            a0, a1, b0, b1 = int(q.a_first[a]), int(q.a_first[a + 1]), int(q.b_first[b]), int(q.b_first[b + 1])
            for fa, fb, n, s, rank in triple_stretches(dist[a0:a1, b0:b1], ok[a0:a1, b0:b1], rate, tol, p.min_run, max_stretches, guard, own_phase_only):
                out.append((a, b, r, fa, fb, n, s, (n - 1) * rate[1] + 16, rank))
    return out


def records(rec) -> list:
    """a structured array of the library's (ALIGN_RATE_STRETCH_DTYPE) as the twin's tuples"""
    return [tuple(int(x[k]) for k in FIELDS) for x in rec]


def cells_of(w, rate):
    """the cells of a record, in rows of the two videos: [(row of a, row of b)]"""
    num, den = rate
    return [(w[3] + num * m, w[4] + den * m) for m in range(w[5])]


# ---- the problems -----------------------------------------------------------------------------------------------------------------------
THREE = ((1, 1), (6, 5), (3, 2))


def _with_skips(rng, p, frac=0.03):
    a_skip, b_skip = np.zeros(len(p.a_hashes), np.uint8), np.zeros(len(p.b_hashes), np.uint8)
    a_skip[rng.random(len(a_skip)) < frac] = 7
    b_skip[rng.random(len(b_skip)) < frac] = 255
    return p._replace(a_skip=a_skip, b_skip=b_skip)


def _cut(a_base=0, b_base=0, skips=False):
    """b 1 is a copy of a 2 at 6/5 with a middle part cut out: cells 0 .. 7 of phase 0 from the first rows of both videos (the rectangle is clamped
    at row 0 of both), then - 29 rows of a further on than the line would go - cells of phase 3 up to the LAST rows of both (clamped at Na and Nb):
    two stretches on two lines first_b - first_a den / num.  Other videos are unrelated: the survivors of round 1 are one triple of a chunk of many."""
    rng = np.random.default_rng([92, 1, a_base, b_base, int(skips)])
    p = gen.layout(rng, THREE, ([30, 9, 111, 0], [31, 9, 112, 2], [29, 8, 110, 1]), [40, 81, 3], a_base, b_base, tol=350, min_run=2)
    gen.plant(rng, p, 1, 2, 1, 0, 0, 0, 8, (0, 30))        # a rows 0, 6 .. 42; b rows 0, 5 .. 35
    gen.plant(rng, p, 1, 2, 1, 3, 12, 10, 7, (0, 30))      # a rows 75, 81 .. 111 = Na - 1; b rows 50, 55 .. 80 = Nb - 1
    return _with_skips(rng, p) if skips else p, 4, 15


def _twice():
    """one part of a 0 at 3/2 appears at two places in b 0: two records with overlapping A ranges"""
    rng = np.random.default_rng([92, 2])
    p = gen.layout(rng, THREE, ([20, 60], [21, 61], [80, 62]), [120, 30], tol=350, min_run=1)
    gen.plant(rng, p, 2, 0, 0, 1, 5, 2, 9, (0, 30))        # a rows 16 .. 40; b rows 4 .. 20
    gen.plant(rng, p, 2, 0, 0, 1, 7, 40, 6, (0, 30))       # a rows 22 .. 37 again; b rows 80 .. 90
    return p, 4, 15


def _replaced():
    """two runs on one line of (6/5, a 1, b 0), around a replaced scene of three cells"""
    rng = np.random.default_rng([92, 3])
    p = gen.layout(rng, THREE, ([9, 130], [9, 131], [9, 129]), [115, 4], tol=350, min_run=2)
    gen.plant(rng, p, 1, 1, 0, 4, 1, 2, 19, (0, 30))       # cells (1 + m, 2 + m): b rows 10 .. 100
    for m in (8, 9, 10):
        p.b_hashes[int(p.b_first[0]) + 5 * (2 + m)] = hashgen.random_hashes(rng, 1)[0]
    return p, 4, 3


def _exactly():
    """max_stretches = 3: (6/5, a 0, b 0) holds exactly three stretches, (6/5, a 1, b 1) five, (3/2, a 0, b 1) one"""
    rng = np.random.default_rng([92, 4])
    p = gen.layout(rng, THREE, ([100, 100], [200, 210], [100, 90]), [170, 175], tol=350, min_run=2)
    for k in range(3):
        gen.plant(rng, p, 1, 0, 0, k, 10 * k + 1, 10 * k, 3 + k, (0, 30))
    for k in range(5):
        gen.plant(rng, p, 1, 1, 1, 5 - k, 6 * k, 6 * k + 1, 3 + (k % 2), (0, 30))
    gen.plant(rng, p, 2, 0, 1, 2, 3, 40, 4, 0)
    return p, 3, 2


def _unrelated():
    rng = np.random.default_rng([92, 5])
    return gen.layout(rng, THREE, ([30, 9, 50], [31, 9, 51], [29, 8, 52]), [40, 31, 3], tol=350, min_run=1), 4, 15


FOUR = ((1, 1), (3, 2), (6, 5), (2, 1))
FOUR_LIST = ((0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (3, 2, 1))


def _four_rates(a_base=0, b_base=0, skips=False):
    """Video 0 of A has ONE window at every rate: the triples (r, 0, 0) are one unit each, and listed first they are the four waves of one workgroup,
    in round 0 and in every masked round, each with its own rectangles: rows 0, 10 and 20 of b 0 - multiples of every den - are that window with 0,
    5 and 9 bits changed, so every (r, 0, 0) has three stretches of one window.  (2/1, a 2, b 1) has two stretches of its own."""
    rng = np.random.default_rng([92, 6, a_base, b_base, int(skips)])
    p = gen.layout(rng, FOUR, ([1, 2, 40], [1, 3, 41], [1, 2, 42], [1, 4, 43]), [30, 25], a_base, b_base, tol=350, min_run=1)
    h = hashgen.random_hashes(rng, 1)[0]
    for r in range(4):
        p.a_hashes[int(p.a_rate_first[r]) + int(p.a_first[r, 0])] = h
    for row, flips in ((0, 0), (10, 5), (20, 9)):
        p.b_hashes[int(p.b_first[0]) + row] = aligngen.flipped(h, flips, rng)
    gen.plant(rng, p, 3, 2, 1, 0, 2, 1, 5, (0, 30))
    gen.plant(rng, p, 3, 2, 1, 1, 12, 12, 4, (0, 30))
    if skips:
        p = _with_skips(rng, p, 0.02)
        p.b_skip[int(p.b_first[0]) + np.array([0, 10, 20])] = 0
        for r in range(4):
            p.a_skip[int(p.a_rate_first[r]) + int(p.a_first[r, 0])] = 0
    return p, 4, 2


def _bands3():
    """(3/2, a 0, b 0) with 200 x 134 windows and tolerance 500: sub-matrices of 67 x 67 cells = 133 diagonals = three bands per phase, about every
    second cell a match; a planted stretch of 40 cells on the main diagonal of phase 1 - its rectangle crosses both band boundaries"""
    rng = np.random.default_rng([92, 7])
    p = gen.layout(rng, ((1, 1), (3, 2)), ([7, 3], [200, 2]), [134, 0, 5], tol=500, min_run=2)
    gen.plant(rng, p, 1, 0, 0, 1, 10, 10, 40, (0, 60))
    return p, 4, 6


def _seven():
    """nine stretches in (6/5, a 0, b 0): with max_stretches = 8 the last round runs with seven rectangles"""
    rng = np.random.default_rng([92, 8])
    p = gen.layout(rng, ((6, 5), (1, 1)), ([340, 5], [20, 5]), [290, 7], tol=350, min_run=2)
    for k in range(9):
        gen.plant(rng, p, 0, 0, 0, k % 6, 6 * k, 6 * k, 3 + (k % 3), (0, 30))
    return p, 8, 3


def _dense():
    """every window matches every window at tolerance 1024: every triple of non-empty videos runs all eight rounds"""
    rng = np.random.default_rng([92, 9])
    return gen.layout(rng, THREE, ([20, 7, 0], [22, 7, 1], [21, 8, 1]), [18, 5], tol=1024, min_run=1), 8, 1


def _square():
    """a library of three videos against itself at two rates: every diagonal triple (r, v, v) and the triple (1, 0, 2) hold two stretches each;
    exclude_same drops the diagonal ones"""
    rng = np.random.default_rng([92, 12])
    p = gen.layout(rng, ((1, 1), (6, 5)), ([60, 50, 55], [70, 60, 66]), [60, 50, 55], tol=350, min_run=2)
    for v in range(3):
        gen.plant(rng, p, 0, v, v, 0, 1 + v, 0, 5, (0, 30))
        gen.plant(rng, p, 0, v, v, 0, 30, 40, 4, (0, 30))
        gen.plant(rng, p, 1, v, v, 2 + v, 0, 3, 3, (0, 30))
        gen.plant(rng, p, 1, v, v, 1, 6, 7, 3, (0, 30))
    gen.plant(rng, p, 1, 0, 2, 4, 1, 5, 2, 0)
    gen.plant(rng, p, 1, 0, 2, 0, 8, 0, 3, 0)
    return p._replace(exclude_same=True), 3, 1


CASES = {
    "square": _square,
    "cut_6_5": _cut,
    "cut_6_5_offsets": functools.partial(_cut, 5, 3, True),
    "used_twice": _twice,
    "replaced_scene": _replaced,
    "exactly_max": _exactly,
    "unrelated": _unrelated,
    "four_rates": _four_rates,
    "four_rates_offsets": functools.partial(_four_rates, 5, 3, True),
    "bands3": _bands3,
    "seven_rects": _seven,
    "dense": _dense,
}
PLANTED = ("square", "cut_6_5", "cut_6_5_offsets", "used_twice", "replaced_scene", "exactly_max", "four_rates", "four_rates_offsets", "bands3", "seven_rects", "dense")
SEEDED = ("square", "cut_6_5", "cut_6_5_offsets", "used_twice", "replaced_scene", "exactly_max", "unrelated", "four_rates_offsets", "seven_rects", "dense")


@functools.lru_cache(maxsize=None)
def case(name: str):
    """-> (problem, max_stretches, guard)"""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name: str) -> tuple:
    return tuple(twin(*case(name)))


def check_non_vacuous(name: str):
    """on the twin's own output: every planted case holds a rank-1 record; the unrelated library holds none at all"""
    want = expected(name)
    if name == "unrelated":
        assert want == ()
        return
    assert any(w[8] == 1 for w in want), name
    p, most, guard = case(name)
    assert max(w[8] for w in want) <= most - 1
    if name.startswith("cut_6_5"):
        a, b = [w for w in want if (w[2], w[0], w[1]) == (1, 2, 1)][:2]
        assert [w[8] for w in (a, b)] == [0, 1] and a[4] * 6 - a[3] * 5 != b[4] * 6 - b[3] * 5          # two lines
        na, nb = int(p.a_first[1, 3] - p.a_first[1, 2]), int(p.b_first[2] - p.b_first[1])
        rects = [rect_of(w[3], w[4], w[5], (6, 5), guard, na, nb) for w in (a, b)]
        assert {0, na} <= {x for r in rects for x in r[:2]} and {0, nb} <= {x for r in rects for x in r[2:]}     # clamped at row 0 and at Na / Nb
    if name == "used_twice":
        a, b = [w for w in want if (w[2], w[0], w[1]) == (2, 0, 0)][:2]
        assert set(range(a[3], a[3] + 3 * a[5])) & set(range(b[3], b[3] + 3 * b[5]))                      # overlapping A ranges
    if name == "replaced_scene":
        a, b = [w for w in want if (w[2], w[0], w[1]) == (1, 1, 0)][:2]
        assert a[4] * 6 - a[3] * 5 == b[4] * 6 - b[3] * 5                                                # one line
    if name == "exactly_max":
        per = lambda t: [w[8] for w in want if (w[2], w[0], w[1]) == t]
        assert per((1, 0, 0)) == [0, 1, 2] and per((1, 1, 1)) == [0, 1, 2] and per((2, 0, 1)) == [0] and most == 3
        assert len([w for w in twin(p, 8, guard, [(1, 0, 0), (1, 1, 1)])]) == 3 + 5
    if name.startswith("four_rates"):
        for r in range(4):
            assert [w[8] for w in want if (w[2], w[0], w[1]) == (r, 0, 0)] == [0, 1, 2], (name, r)
    if name == "seven_rects":
        assert [w[8] for w in want if (w[2], w[0], w[1]) == (0, 0, 0)] == list(range(8)) and most == 8
    if name == "dense":
        assert max(w[8] for w in want) == 7


def random_problem(rng):
    """ratealigngen.random_problem, and in one of its triples up to four more planted lines: -> (problem, max_stretches, guard)"""
    p = gen.random_problem(rng)
    n_a, n_b = p.a_first.shape[1] - 1, len(p.b_first) - 1
    sizes = [(int(p.a_first[r, a + 1] - p.a_first[r, a]), int(p.b_first[b + 1] - p.b_first[b]), r, a, b)
             for r in range(len(p.rates)) for a in range(n_a) for b in range(n_b)]
    na, nb, r, a, b = max(sizes, key=lambda s: min(s[0], s[1]))
    num, den = reduced(p.rates[r])
    n = p.min_run + int(rng.integers(0, 3))
    for k in range(int(rng.integers(2, 5))):
        ph, i0, j0 = int(rng.integers(0, num)), int(rng.integers(0, 4)) + k * (n + 2), int(rng.integers(0, 4)) + (3 - k) * (n + 2)
        if ph + num * (i0 + n - 1) < na and den * (j0 + n - 1) < nb:
            gen.plant(rng, p, r, a, b, ph, i0, j0, n, (0, 40))
    return p, int(rng.integers(1, 9)), int(rng.choice([0, 1, 3, 15, 40]))


def slow_content(guard=2):
    """The phase trap: a's windows at 6/5 change SLOWLY - row k + 1 is row k with 40 bits changed, so rows up to about eight apart lie within the
    tolerance, as the windows of real video one frame apart do - and rows 10, 15 .. 40 of b are rows 23, 29 .. 59 of a (phase 5), exactly.  The
    stretch is also visible, a little worse, from every other phase.  min_run 1.  -> (problem, max_stretches, guard)"""
    rng = np.random.default_rng([92, 10])
    p = gen.layout(rng, ((6, 5),), ([100],), [60], tol=350, min_run=1)
    for k in range(1, 100):
        p.a_hashes[k] = aligngen.flipped(p.a_hashes[k - 1], 40, rng)
    gen.plant(rng, p, 0, 0, 0, 5, 3, 2, 7, 0)
    return p, 4, guard
