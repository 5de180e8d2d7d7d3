"""Shared by the tests of the native retimed alignment: a numpy twin of the definition in include/vdf.h
(vdf_align_windows_retimed*) - phases, sub-matrices, skip bytes, the two-level reduction - and the problems both the CPU test of the _host forms
and the GPU test of the kernel solve.  numpy + tests/hashgen.py + tests/aligngen.py's builders only: nothing is imported from the library.
Records are compared for equality - there are no tolerances.

Random 1000-bit hashes sit 500 +- 16 apart: at tolerance 350 nothing matches but what a builder planted, at tolerance 500 about every second
cell matches and runs, ties and band crossings are everywhere."""
from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional

import numpy as np

import aligngen
import hashgen


class Problem(NamedTuple):
    a_hashes: np.ndarray            # [windows, 16] u64: retimed windows of A's videos
    a_first: np.ndarray             # [videos + 1] u32
    b_hashes: np.ndarray            # plain windows of B's videos
    b_first: np.ndarray
    rate: tuple                     # (num, den), not necessarily reduced
    tol: int
    min_run: int = 1
    a_skip: Optional[np.ndarray] = None
    b_skip: Optional[np.ndarray] = None


def reduced(rate):
    g = math.gcd(*rate)
    return rate[0] // g, rate[1] // g


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
def diagonal_runs(dist: np.ndarray, ok: np.ndarray, tol: int, min_run: int):
    """dist, ok [na, nb] of one sub-matrix -> every competing run [(score, offset, i0, n, dist_sum)]: per diagonal the maximal stretches of cells
    with ok and dist <= tol, found with one diff and one cumsum per diagonal."""
    na, nb = dist.shape
    m = ok & (dist <= tol)
    runs = []
    for d in range(-(na - 1), nb):
        md = np.diagonal(m, d)
        if not md.any():
            continue
        edges = np.diff(np.concatenate(([0], md.astype(np.int8), [0])))
        starts, ends = np.flatnonzero(edges == 1), np.flatnonzero(edges == -1)
        cs = np.concatenate(([0], np.cumsum(np.where(md, np.diagonal(dist, d), 0))))
        for st, en in zip(starts.tolist(), ends.tolist()):
            n, s = en - st, int(cs[en] - cs[st])
            if n >= min_run:
                runs.append((n * (tol + 1) - s, d, st + max(0, -d), n, s))
    return runs


def pair_runs(dist: np.ndarray, ok: np.ndarray, rate, tol: int, min_run: int):
    """dist, ok [Na, Nb] of one pair of videos -> {phase: its competing runs}: the sub-matrix of phase p is rows p, p + num, ... x columns 0, den, ..."""
    num, den = rate
    return {p: diagonal_runs(dist[p::num, 0::den], ok[p::num, 0::den], tol, min_run) for p in range(num) if p < dist.shape[0] and dist.shape[1]}


def two_level(runs_by_phase, rate):
    """-> (first_a, first_b, n_windows, dist_sum) or None.  Level 1, inside a phase: score, then the smaller offset, then the smaller i0.
    Level 2, across the phases: score, then the smaller first_a = p + num i0, then the smaller first_b = den (i0 + offset)."""
    num, den = rate
    best = None
    for p, runs in sorted(runs_by_phase.items()):
        if not runs:
            continue
        score, off, i0, n, s = min(runs, key=lambda r: (-r[0], r[1], r[2]))
        key = (-score, p + num * i0, den * (i0 + off))
        if best is None or key < best[0]:
            best = (key, n, s)
    return None if best is None else (best[0][1], best[0][2], best[1], best[2])


def one_level(runs_by_phase, rate):
    """what ONE comparator (score, first_a, first_b) over all runs of all phases would report - not the definition; the tie trap shows the difference"""
    num, den = rate
    flat = [(-score, p + num * i0, den * (i0 + off), n, s) for p, runs in runs_by_phase.items() for score, off, i0, n, s in runs]
    return None if not flat else min(flat)[1:]


def _cells(p: Problem):
    dist = hashgen.all_distances(p.a_hashes, p.b_hashes) if len(p.a_hashes) and len(p.b_hashes) else np.zeros((len(p.a_hashes), len(p.b_hashes)), np.int64)
    ska = np.zeros(len(p.a_hashes), bool) if p.a_skip is None else np.asarray(p.a_skip) != 0
    skb = np.zeros(len(p.b_hashes), bool) if p.b_skip is None else np.asarray(p.b_skip) != 0
    return dist, ~ska[:, None] & ~skb[None, :]


def align_retimed_twin(p: Problem, pairs=None, reduce=two_level):
    """-> the records [(a, b, first_a, first_b, n_windows, dist_sum)] in (a, b) order; pairs: only these (a, b)"""
    tol, rate = min(int(p.tol), 1024), reduced(p.rate)
    dist, ok = _cells(p)
    n_a, n_b = len(p.a_first) - 1, len(p.b_first) - 1
    out = []
    for a, b in (pairs if pairs is not None else [(a, b) for a in range(n_a) for b in range(n_b)]):
        a0, a1, b0, b1 = int(p.a_first[a]), int(p.a_first[a + 1]), int(p.b_first[b]), int(p.b_first[b + 1])
        r = reduce(pair_runs(dist[a0:a1, b0:b1], ok[a0:a1, b0:b1], rate, tol, p.min_run), rate)
        if r is not None:
            out.append((a, b) + tuple(int(x) for x in r))
    return out


def records(rec) -> list:
    """a structured array of the library's (ALIGN_RETIMED_DTYPE) as the twin's tuples"""
    return [tuple(int(r[k]) for k in ("a", "b", "first_a", "first_b", "n_windows", "dist_sum")) for r in rec]


# ---- builders ---------------------------------------------------------------------------------------------------------------------------
def plant(rng, p: Problem, a, b, phase, i0, j0, n, flips=0):
    """cells (i0 + m, j0 + m), m < n, of phase `phase` of pair (a, b): row den (j0 + m) of b := row phase + num (i0 + m) of a with `flips` bits
    changed (an int, or (lo, hi): drawn per cell)"""
    num, den = reduced(p.rate)
    for m in range(n):
        k = flips if isinstance(flips, int) else int(rng.integers(flips[0], flips[1] + 1))
        ra, rb = int(p.a_first[a]) + phase + num * (i0 + m), int(p.b_first[b]) + den * (j0 + m)
        assert ra < p.a_first[a + 1] and rb < p.b_first[b + 1], "a planted cell outside its videos"
        p.b_hashes[rb] = aligngen.flipped(p.a_hashes[ra], k, rng)


def _noise(seed, ca, cb, rate, tol, min_run=1):
    rng = np.random.default_rng([78, seed])
    ah, af = aligngen.videos(rng, ca)
    bh, bf = aligngen.videos(rng, cb)
    return rng, Problem(ah, af, bh, bf, rate, tol, min_run)


def _band_boundaries():
    # 3 / 2: sub-matrices up to 67 x 65 cells = 131 diagonals = 3 bands; phases with p >= Na; empty videos.  About every second cell matches.
    return _noise(1, [0, 1, 2, 3, 200, 201], [0, 1, 2, 129, 130], (3, 2), 500)[1]


def _planted(min_run):
    """3 / 2, pair (i, i) for every i: A 200 windows -> 67, 67, 66 rows per phase, B 130 -> 65 columns; band 0 of the 67-row phases ends at offset -3,
    band 1 begins at -2"""
    rng, p = _noise(2, [200] * 8, [130] * 8, (3, 2), 350, min_run)
    t = p.tol
    plant(rng, p, 0, 0, 1, 0, 10, 5, (0, 30))       # touches the top edge (i = 0)
    plant(rng, p, 0, 0, 2, 61, 30, 5, (0, 30))      # ... and the bottom edge of phase 2 (66 rows)
    plant(rng, p, 1, 1, 0, 20, 0, 6, (0, 30))       # the left edge (j = 0)
    plant(rng, p, 1, 1, 1, 12, 59, 6, (0, 30))      # the right edge (j = 64)
    plant(rng, p, 2, 2, 0, 30, 27, 7, 3)            # the last diagonal of band 0 ...
    plant(rng, p, 2, 2, 0, 45, 43, 7, 2)            # ... and the first of band 1: the better one
    plant(rng, p, 3, 3, 1, 30, 27, 7, 2)            # the same with the better run in band 0
    plant(rng, p, 3, 3, 1, 45, 43, 7, 3)
    plant(rng, p, 4, 4, 2, 10, 20, 11, 4)           # two runs on one line, one miss between them: 5 | 5
    p.b_hashes[int(p.b_first[4]) + 2 * 25] = hashgen.random_hashes(rng, 1)[0]
    plant(rng, p, 5, 5, 0, 8, 9, 1, t)              # exactly on the tolerance: a run of one
    plant(rng, p, 5, 5, 1, 40, 3, 1, t + 1)         # one over: nothing
    plant(rng, p, 6, 6, 1, 50, 50, 5, (0, 30))      # min_run = 5 keeps it, 6 drops it
    plant(rng, p, 7, 7, 0, 0, 0, 65, (0, 40))       # the main diagonal, corner to edge
    return p


def _rates(rate, noisy):
    num, den = reduced(rate)
    rng, p = _noise(4, [70, 5], [40, 9], rate, 500 if noisy else 350)
    if not noisy:
        n = min((70 - 3 - 1) // num + 1, (40 - 1) // den + 1)
        plant(rng, p, 0, 0, 3 % num, 0, 0, n, (0, 20))                        # a line from the corner, as long as both videos allow
        if num > 1 and (70 - 1 - 1) // num >= 1 and (40 - 1) // den >= 1:
            plant(rng, p, 0, 1, 1 % num, 1, 0, min(2, (9 - 1) // den + 1), 5)  # and a short one in another phase against the short video
    return p


def _skip(noisy):
    # first arrays that are no multiples of 4: A 0, 5, 75, 78; B 0, 3, 45, 90 - the scalar read of A's skip byte lands on every byte of its dword
    rng, p = _noise(5, [5, 70, 3], [3, 42, 45], (3, 2), 500 if noisy else 350)
    a_skip, b_skip = np.zeros(len(p.a_hashes), np.uint8), np.zeros(len(p.b_hashes), np.uint8)
    if noisy:
        a_skip[rng.random(len(a_skip)) < 0.15] = 1
        b_skip[rng.random(len(b_skip)) < 0.15] = 200
    else:
        plant(rng, p, 1, 1, 1, 2, 3, 15, (0, 30))      # rows 5 + 1 + 3 (2 + m) of A, rows 3 + 2 (3 + m) of B
        plant(rng, p, 1, 2, 2, 0, 6, 12, 10)           # rows 5 + 2 + 3 m of A, rows 45 + 2 (6 + m) of B
        a_skip[5 + 1 + 3 * (2 + 6)] = 1                 # cuts the first run in two: 6 | 8
        b_skip[45 + 2 * (6 + 4)] = 255                  # and the second: 4 | 7
        a_skip[5 + 3 * 4] = 9                           # phase 0 of video 1: no run there, nothing changes
    return p._replace(a_skip=a_skip, b_skip=b_skip)


def _dense(rate=(3, 2)):
    rng = np.random.default_rng([78, 6])
    h = hashgen.random_hashes(rng, 1)
    ca, cb = [200, 64, 65, 1], [129, 200, 63]
    return Problem(np.repeat(h, sum(ca), axis=0), aligngen.first_of(ca), np.repeat(h, sum(cb), axis=0), aligngen.first_of(cb), rate, 350)


def _tie_trap():
    """6 / 5; 90 windows of A: 15 rows per phase, 80 of B: 16 columns; exact copies of 4 cells, so every run scores 4 (tol + 1).
    Pair (0, 0): phase 2 holds R1 = (offset -3, i0 9) and R2 = (offset 7, i0 4) - level 1 keeps R1, the smaller offset, although R2 starts
    earlier; phase 4 holds R3 = (offset -7, i0 7).  first_a: R1 2 + 54 = 56, R2 2 + 24 = 26, R3 4 + 42 = 46: the two-level rule reports R3
    (46 < 56), ONE comparator over all runs of all phases would report R2 (26).  Pair (1, 1): phases 1 and 3 tie, first_a 31 and 27: the later
    phase wins.  Pair (2, 2): phases 0 and 5 tie at the same i0, first_a 36 and 41: the earlier phase wins."""
    rng, p = _noise(3, [90, 90, 90], [80, 80, 80], (6, 5), 350)
    plant(rng, p, 0, 0, 2, 9, 6, 4)      # R1: cells (9, 6) ... (12, 9)
    plant(rng, p, 0, 0, 2, 4, 11, 4)     # R2: cells (4, 11) ... (7, 14)
    plant(rng, p, 0, 0, 4, 7, 0, 4)      # R3: cells (7, 0) ... (10, 3) of phase 4
    plant(rng, p, 1, 1, 1, 5, 2, 4)
    plant(rng, p, 1, 1, 3, 4, 9, 4)
    plant(rng, p, 2, 2, 0, 6, 1, 4)
    plant(rng, p, 2, 2, 5, 6, 10, 4)
    return p


RATES = ((1, 1), (2, 1), (6, 5), (31, 16), (32, 17))

CASES = {
    "band_boundaries": _band_boundaries,
    **{f"planted_min_run_{m}": functools.partial(_planted, m) for m in (1, 5, 6)},
    "tie_trap": _tie_trap,
    **{f"rate_{r[0]}_{r[1]}": functools.partial(_rates, r, False) for r in RATES},
    **{f"rate_{r[0]}_{r[1]}_noise": functools.partial(_rates, r, True) for r in RATES},
    "skip_cuts": lambda: _skip(False),
    "skip_noise": lambda: _skip(True),
    "dense_3_2": _dense,
    "dense_6_5": lambda: _dense((6, 5)),
}


@functools.lru_cache(maxsize=None)
def case(name: str) -> Problem:
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name: str) -> tuple:
    return tuple(align_retimed_twin(case(name)))
