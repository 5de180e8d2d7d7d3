"""Shared by the tests of the seeded retimed call (vdf_align_seed_pairs_rates*): a numpy twin of the definition in include/vdf.h,
the composition it must equal (vdf_align_seed_pairs on the sub-sampled sets, united over the phases), and the problems both the CPU tests of the
host form and the GPU tests of the seed kernel solve.  numpy, tests/hashgen.py and tests/aligngen.py only: nothing is imported from the library
(the composition takes the library's seed call as an argument).  Triples are compared for equality.

The twin: under rate r = num / den (lowest terms) the seeds of video a are its windows ka of block r with (ka // num) % min_run == 0, the rows of
video b its windows kb with kb % den == 0; (a, b) is a candidate under r iff some seed and some row, neither skipped, lie within tol of each
other - brute-force distances on the strided sets."""
from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional

import numpy as np

import aligngen
import hashgen

USUAL_RATES = ((1, 1), (2, 1), (3, 2), (5, 4), (6, 5))
B_COUNTS = (0, 1, 4, 700, 5, 1900)         # 2610 rows: six tiles of 512 at den 1; 523 rows at den 5 - a second tile of 11 rows, waves 1 - 3 padding
A_COUNTS = (0, 1, 2, 3, 31, 33, 600)       # per rate block: empty phases in the short videos; 670 windows per block


class Problem(NamedTuple):
    a_hashes: np.ndarray            # [rows, 16] u64: rate-major, block r holds the retimed windows of A's videos at rates[r]
    a_first: np.ndarray             # [n_rates, n_a + 1] u32
    a_rate_first: np.ndarray        # [n_rates + 1] int64: window k of video i at rate r is row a_rate_first[r] + a_first[r, i] + k
    b_hashes: np.ndarray            # plain windows of B's videos
    b_first: np.ndarray             # [n_b + 1] u32
    rates: tuple                    # ((num, den), ...), not necessarily reduced
    tol: int
    min_run: int = 1
    a_skip: Optional[np.ndarray] = None
    b_skip: Optional[np.ndarray] = None
    exclude_same: bool = False


def reduced(rate):
    g = math.gcd(int(rate[0]), int(rate[1]))
    return int(rate[0]) // g, int(rate[1]) // g


def _strided(p: Problem, r: int):
    """the seeds of block r and the rows of B under rates[r], skipped windows dropped: (rows of a_hashes, their videos, rows of b_hashes, their videos)"""
    num, den = reduced(p.rates[r])
    fa, base = p.a_first[r].astype(np.int64), int(p.a_rate_first[r])
    sa, va, sb, vb = [], [], [], []
    for a in range(len(fa) - 1):
        ka = np.arange(fa[a + 1] - fa[a])
        ka = ka[(ka // num) % p.min_run == 0]
        sa.append(base + fa[a] + ka)
        va.append(np.full(len(ka), a))
    fb = p.b_first.astype(np.int64)
    for b in range(len(fb) - 1):
        kb = np.arange(0, fb[b + 1] - fb[b], den)
        sb.append(fb[b] + kb)
        vb.append(np.full(len(kb), b))
    sa, va, sb, vb = (np.concatenate(x + [np.zeros(0, np.int64)]).astype(np.int64) for x in (sa, va, sb, vb))
    if p.a_skip is not None:
        keep = np.asarray(p.a_skip)[sa] == 0
        sa, va = sa[keep], va[keep]
    if p.b_skip is not None:
        keep = np.asarray(p.b_skip)[sb] == 0
        sb, vb = sb[keep], vb[keep]
    return sa, va, sb, vb


def seed_rates_twin(p: Problem) -> list:
    """-> the candidate triples [(a, b, rate index)] in (rate, a, b) order"""
    tol = min(int(p.tol), 1024)
    out = []
    for r in range(len(p.rates)):
        sa, va, sb, vb = _strided(p, r)
        if not len(sa) or not len(sb):
            continue
        i, j = np.nonzero(hashgen.all_distances(p.a_hashes[sa], p.b_hashes[sb]) <= tol)
        pairs = {(int(a), int(b)) for a, b in np.unique(np.stack([va[i], vb[j]], 1), axis=0)} if len(i) else set()
        out += [(a, b, r) for a, b in sorted(pairs) if not (p.exclude_same and a == b)]
    return out


def composition(p: Problem, seed_pairs_host) -> list:
    """The union over the phases p < num of seed_pairs_host - the library's align_seed_pairs_host - on (windows p, p + num, ... of block r's
    videos; windows 0, den, ... of B's), per rate: what the one call must equal."""
    out = []
    fb = p.b_first.astype(np.int64)
    for r in range(len(p.rates)):
        num, den = reduced(p.rates[r])
        fa, base = p.a_first[r].astype(np.int64), int(p.a_rate_first[r])
        rows_b = [fb[b] + np.arange(0, fb[b + 1] - fb[b], den) for b in range(len(fb) - 1)]
        sub_b = np.concatenate(rows_b + [np.zeros(0, np.int64)]).astype(np.int64)
        first_b = aligngen.first_of([len(x) for x in rows_b])
        found = set()
        for ph in range(num):
            rows_a = [base + fa[a] + np.arange(ph, fa[a + 1] - fa[a], num) for a in range(len(fa) - 1)]
            sub_a = np.concatenate(rows_a + [np.zeros(0, np.int64)]).astype(np.int64)
            first_a = aligngen.first_of([len(x) for x in rows_a])
            cap = max(1, (len(fa) - 1) * (len(fb) - 1))
            pairs, n = seed_pairs_host(p.a_hashes[sub_a], first_a, p.b_hashes[sub_b], first_b, tol_int=p.tol, min_run=p.min_run,
                                       a_skip=None if p.a_skip is None else np.asarray(p.a_skip)[sub_a],
                                       b_skip=None if p.b_skip is None else np.asarray(p.b_skip)[sub_b], capacity=cap)
            assert n == len(pairs)
            found |= {(int(q["a"]), int(q["b"])) for q in pairs}
        out += [(a, b, r) for a, b in sorted(found) if not (p.exclude_same and a == b)]
    return out


def triples_of(arr) -> list:
    """a structured array of the library's (VIDEO_PAIR_RATE_DTYPE) as the twin's tuples"""
    return [(int(t["a"]), int(t["b"]), int(t["rate"])) for t in arr]


def block(p: Problem, r: int):
    """block r as the A side of the retimed align calls: (hashes, first, skip)"""
    lo, hi = int(p.a_rate_first[r]), int(p.a_rate_first[r + 1])
    return p.a_hashes[lo:hi], p.a_first[r], None if p.a_skip is None else np.asarray(p.a_skip)[lo:hi]


# ---- builders ---------------------------------------------------------------------------------------------------------------------------
def _layout(rng, rates, ca, cb, a_base, b_base):
    """random hashes in the calls' layout: every block of A and B begin a_base / b_base rows into their arrays"""
    n_rates = len(rates)
    a_first = np.stack([a_base + aligngen.first_of(ca) for _ in range(n_rates)]).astype(np.uint32)
    per_block = a_base + int(sum(ca))
    a_rate_first = np.arange(n_rates + 1, dtype=np.int64) * per_block
    a_hashes = hashgen.random_hashes(rng, int(a_rate_first[-1]))
    b_first = (b_base + aligngen.first_of(cb)).astype(np.uint32)
    b_hashes = hashgen.random_hashes(rng, int(b_first[-1]))
    return a_hashes, a_first, a_rate_first, b_hashes, b_first


KINDS = ("at_tol", "above_tol", "off_row", "no_seed", "skip_a", "skip_b", "none", "none", "none")


def planted(rates=USUAL_RATES, tol=350, min_run=2, seed=0, ca=A_COUNTS, cb=B_COUNTS, a_base=5, b_base=3) -> Problem:
    """Random hashes - 1000 fair bits lie more than 6 sigma above 400 apart - with single planted cells, one kind per (rate, a, b) in a fixed
    rotation: a seed and a row at distance exactly tol (a candidate) and tol + 1 (none); a seed against a window of b with kb % den != 0; a
    window that is no seed against a row; a seed and a row at distance 0 with the seed's or the row's skip byte set.  The rows used are, per
    class of den, the first and last rows of the tiles of 512 and of the waves of 128 gathered rows, and the class's last row."""
    rng = np.random.default_rng([83, seed, tol, min_run])
    a_hashes, a_first, a_rate_first, b_hashes, b_first = _layout(rng, rates, ca, cb, a_base, b_base)
    a_skip, b_skip = np.zeros(len(a_hashes), np.uint8), np.zeros(len(b_hashes), np.uint8)
    fb = b_first.astype(np.int64)
    used_b = set()      # rows of B that a plant relies on: the skip_b plants take others
    free_a = {}         # (rate, a) -> the seeds and the other windows of the video no plant has used yet

    def gathered(den):  # the class's rows as the kernel sees them: [(b, kb)]
        return [(b, kb) for b in range(len(cb)) for kb in range(0, cb[b], den)]

    def rows_of(den, b):
        g = gathered(den)
        edges = [i for i in (0, 63, 64, 127, 128, 255, 256, 511, 512, 639, 640, 1023, 1024, len(g) - 1) if i < len(g)]
        return [g[i][1] for i in edges if g[i][0] == b] or [g[i][1] for i in range(len(g)) if g[i][0] == b]

    count = 0
    for r, rate in enumerate(rates):
        num, den = reduced(rate)
        for a in range(len(ca)):
            ka_all = np.arange(ca[a])
            free_a[(r, a)] = [list(ka_all[(ka_all // num) % min_run == 0]), list(ka_all[(ka_all // num) % min_run != 0])]
            for b in range(len(cb)):
                kind = KINDS[(3 * r + 2 * a + b) % len(KINDS)]
                if a == len(ca) - 1 and b == 3 % len(cb):
                    kind = "at_tol"       # every rate has a candidate ...
                if a == len(ca) - 2 and b == len(cb) - 1:
                    kind = "above_tol"    # ... and a near miss
                count += 1
                seeds, others = free_a[(r, a)]
                if kind == "none" or cb[b] == 0 or not seeds:
                    continue
                good_rows = rows_of(den, b)
                kb = good_rows[count % len(good_rows)]
                if kind == "off_row":
                    if den == 1 or cb[b] < 2:
                        continue
                    kb = min(kb + 1 + count % (den - 1), cb[b] - 1)
                    if kb % den == 0:
                        continue
                if kind == "no_seed":
                    if not others:
                        continue
                    ka = others.pop(count % len(others))
                else:
                    ka = seeds.pop(-1 if count % 2 else 0)   # the video's first and last seeds first
                if kind == "skip_b":
                    free = [k for k in range(0, cb[b], den) if int(fb[b]) + k not in used_b]
                    if not free:
                        continue
                    kb = free[count % len(free)]
                    b_skip[int(fb[b]) + kb] = 1
                else:
                    if b_skip[int(fb[b]) + kb]:
                        continue
                    used_b.add(int(fb[b]) + kb)
                row_a = int(a_rate_first[r]) + int(a_first[r, a]) + int(ka)
                dist = {"at_tol": tol, "above_tol": tol + 1}.get(kind, 0)
                a_hashes[row_a] = aligngen.flipped(b_hashes[int(fb[b]) + kb], dist, rng)
                if kind == "skip_a":
                    a_skip[row_a] = 1
    return Problem(a_hashes, a_first, a_rate_first, b_hashes, b_first, tuple(rates), tol, min_run, a_skip, b_skip)


def square(n=7, tol=350, min_run=1, seed=0) -> Problem:
    """n x n videos of a few windows, rates 1/1 and 3/2, every diagonal pair (i, i) and a few others planted: the exclude_same problem"""
    rng = np.random.default_rng([83, 7, seed])
    counts = [3 + (i * 5) % 11 for i in range(n)]
    rates = ((1, 1), (3, 2))
    a_hashes, a_first, a_rate_first, b_hashes, b_first = _layout(rng, rates, counts, counts, 0, 0)
    for r in range(len(rates)):
        for i in range(n):
            for ka, j in enumerate([i, (i + 2) % n] if i % 3 else [i]):   # window 0 of video i is window 0 of video i of B, window 1 another video's
                a_hashes[int(a_rate_first[r]) + int(a_first[r, i]) + ka] = b_hashes[int(b_first[j])]
    return Problem(a_hashes, a_first, a_rate_first, b_hashes, b_first, rates, tol, min_run)


def random_problem(rng) -> Problem:
    """One seeded random problem in the style of tests/alignfuzz.py: 1 .. 4 rates, a few videos of 0 .. 90 windows, random first-array bases,
    random skip bytes, planted stretches along the rate's slope with 0 .. tol + 40 bits flipped, so cells land on both sides of the tolerance."""
    pool = [(1, 1), (2, 1), (3, 2), (5, 4), (6, 5), (4, 3), (6, 4), (2, 2), (31, 16), (32, 17), (64, 34)]
    rates = tuple(pool[int(i)] for i in rng.integers(0, len(pool), size=int(rng.integers(1, 5))))
    tol = int(rng.choice([150, 250, 350, 400]))
    min_run = int(rng.integers(1, 5))
    ca = [int(rng.integers(0, 91)) for _ in range(int(rng.integers(1, 8)))]
    cb = [int(rng.integers(0, 300)) for _ in range(int(rng.integers(1, 8)))]
    a_hashes, a_first, a_rate_first, b_hashes, b_first = _layout(rng, rates, ca, cb, int(rng.integers(0, 7)), int(rng.integers(0, 7)))
    for _ in range(int(rng.integers(2, 14))):
        r = int(rng.integers(0, len(rates)))
        num, den = reduced(rates[r])
        a, b = int(rng.integers(0, len(ca))), int(rng.integers(0, len(cb)))
        if ca[a] == 0 or cb[b] == 0:
            continue
        ka, kb = int(rng.integers(0, ca[a])), int(rng.integers(0, cb[b]))
        for m in range(int(rng.integers(1, 6))):
            if ka + num * m < ca[a] and kb + den * m < cb[b]:
                flips = int(rng.integers(0, tol + 41))
                a_hashes[int(a_rate_first[r]) + int(a_first[r, a]) + ka + num * m] = aligngen.flipped(b_hashes[int(b_first[b]) + kb + den * m], flips, rng)
    a_skip = (rng.random(len(a_hashes)) < 0.1).astype(np.uint8) if rng.random() < 0.6 else None
    b_skip = (rng.random(len(b_hashes)) < 0.1).astype(np.uint8) if rng.random() < 0.6 else None
    return Problem(a_hashes, a_first, a_rate_first, b_hashes, b_first, rates, tol, min_run, a_skip, b_skip)


CASES = {
    "tol150_run1": functools.partial(planted, tol=150, min_run=1, seed=1),
    "tol250_run2": functools.partial(planted, tol=250, min_run=2, seed=2),
    "tol350_run3": functools.partial(planted, tol=350, min_run=3, seed=3),
    "tol400_run2": functools.partial(planted, tol=400, min_run=2, seed=4),
    "big_num": functools.partial(planted, rates=((31, 16), (32, 17)), tol=350, min_run=2, seed=5),
    "one_rate": functools.partial(planted, rates=((3, 2),), tol=350, min_run=2, seed=6),
    "duplicates": functools.partial(planted, rates=((64, 34), (32, 17), (3, 2), (6, 4), (3, 2)), tol=350, min_run=2, seed=7),
}
SPARSE = tuple(CASES)   # the cases whose only matches are planted: the non-vacuity condition holds on each of them


@functools.lru_cache(maxsize=None)
def case(name: str) -> Problem:
    if name == "dense":   # tolerance 500: about half of all cells of random hashes match - the bitmap's read-before-atomic path
        return planted(tol=500, min_run=2, seed=8)
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name: str) -> tuple:
    return tuple(seed_rates_twin(case(name)))
