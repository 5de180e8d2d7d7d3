"""Shared by the align tests: a numpy twin of the definition in include/vdf.h (vdf_align_windows) and the problems both
the CPU test of vdf_align_windows_host and the GPU test of the kernel solve.  numpy + tests/hashgen.py only: nothing is imported from
the library, so a change on either side shows as a disagreement.  Records are compared for equality - there are no tolerances.

Random 1000-bit hashes sit 500 +- 16 apart, so at tolerances up to 350 nothing matches but what a builder planted."""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import numpy as np

import hashgen


class Problem(NamedTuple):
    a_hashes: np.ndarray            # [windows, 16] u64
    a_first: np.ndarray             # [videos + 1] u32
    b_hashes: Optional[np.ndarray]  # None: self mode
    b_first: Optional[np.ndarray]
    tol: int
    min_run: int = 1
    a_skip: Optional[np.ndarray] = None
    b_skip: Optional[np.ndarray] = None


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
def best_run(dist: np.ndarray, ok: np.ndarray, tol: int, min_run: int):
    """dist [Na, Nb] distances, ok [Na, Nb] False where a window abstains -> (offset, start_a, n_windows, dist_sum) or None: a literal walk
    of every diagonal, runs of consecutive cells with ok and dist <= tol, the best by score = n (tol + 1) - dist_sum, ties to the smaller
    offset, then the smaller start."""
    na, nb = dist.shape
    best, best_key = None, None
    for d in range(-(na - 1), nb):
        runs, cur = [], None
        for ka in range(max(0, -d), min(na, nb - d)):
            kb = ka + d
            if ok[ka, kb] and dist[ka, kb] <= tol:
                if cur is None:
                    cur = [ka, 0, 0]
                cur[1] += 1
                cur[2] += int(dist[ka, kb])
            elif cur is not None:
                runs.append(cur)
                cur = None
        if cur is not None:
            runs.append(cur)
        for start, n, s in runs:
            if n < min_run:
                continue
            key = (-(n * (tol + 1) - s), d, start)
            if best_key is None or key < best_key:
                best_key, best = key, (d, start, n, s)
    return best


def align_twin(p: Problem):
    """-> the records [(a, b, offset, start_a, n_windows, dist_sum)] in (a, b) order"""
    tol = min(int(p.tol), 1024)
    self_mode = p.b_hashes is None
    bh, bf, bs = (p.a_hashes, p.a_first, p.a_skip) if self_mode else (p.b_hashes, p.b_first, p.b_skip)
    dist = hashgen.all_distances(p.a_hashes, bh) if len(p.a_hashes) and len(bh) else np.zeros((len(p.a_hashes), len(bh)), np.int64)
    ska = np.zeros(len(p.a_hashes), bool) if p.a_skip is None else np.asarray(p.a_skip) != 0
    skb = np.zeros(len(bh), bool) if bs is None else np.asarray(bs) != 0
    ok = ~ska[:, None] & ~skb[None, :]
    out = []
    for a in range(len(p.a_first) - 1):
        for b in range(a + 1 if self_mode else 0, len(bf) - 1):
            a0, a1, b0, b1 = int(p.a_first[a]), int(p.a_first[a + 1]), int(bf[b]), int(bf[b + 1])
            if a1 == a0 or b1 == b0:
                continue
            r = best_run(dist[a0:a1, b0:b1], ok[a0:a1, b0:b1], tol, p.min_run)
            if r is not None:
                out.append((a, b) + r)
    return out


def records(rec) -> list:
    """a structured array of the library's (ALIGN_DTYPE) as the twin's tuples"""
    return [tuple(int(r[k]) for k in ("a", "b", "offset", "start_a", "n_windows", "dist_sum")) for r in rec]


# ---- builders ---------------------------------------------------------------------------------------------------------------------------
def first_of(counts) -> np.ndarray:
    f = np.zeros(len(counts) + 1, np.uint32)
    f[1:] = np.cumsum(counts)
    return f


def videos(rng, counts):
    return hashgen.random_hashes(rng, int(sum(counts))), first_of(counts)


def flipped(h: np.ndarray, k: int, rng) -> np.ndarray:
    return hashgen.hash_with_spatial_distance(h, k, rng) if k else h.copy()


def plant(rng, ah, af, a, ka, bh, bf, b, kb, n, flips=0):
    """windows kb .. kb + n of video b of B := windows ka .. ka + n of video a of A, each with `flips` bits changed (an int, or (lo, hi):
    drawn per window)"""
    for i in range(n):
        k = flips if isinstance(flips, int) else int(rng.integers(flips[0], flips[1] + 1))
        bh[int(bf[b]) + kb + i] = flipped(ah[int(af[a]) + ka + i], k, rng)


def _pairs_problem(seed, shapes, plants, tol=350, min_run=1):
    """video i of A (shapes[i][0] windows) against video i of B (shapes[i][1]): plants = [(i, ka, kb, n, flips)]; the other pairs stay empty"""
    rng = np.random.default_rng([77, seed])
    ah, af = videos(rng, [s[0] for s in shapes])
    bh, bf = videos(rng, [s[1] for s in shapes])
    for i, ka, kb, n, flips in plants:
        plant(rng, ah, af, i, ka, bh, bf, i, kb, n, flips)
    return Problem(ah, af, bh, bf, tol, min_run)


def _mixed_counts():
    rng = np.random.default_rng([77, 1])
    ca = [1, 2, 63, 64, 65, 127, 128, 129, 200]
    cb = [200, 0, 65, 1, 128, 64, 2, 129, 63, 127]
    ah, af = videos(rng, ca)
    bh, bf = videos(rng, cb)
    for b, nb in enumerate(cb):  # every video of B holds a shifted copy out of two videos of A
        for a in (b % len(ca), (3 * b + 4) % len(ca)):
            n = int(rng.integers(1, min(ca[a], nb) + 1)) if nb else 0
            if n:
                plant(rng, ah, af, a, int(rng.integers(0, ca[a] - n + 1)), bh, bf, b, int(rng.integers(0, nb - n + 1)), n, (0, 40))
    return Problem(ah, af, bh, bf, 350)


def _tolerance(tol):
    t = min(tol, 1024)
    rng = np.random.default_rng([77, 2, tol])
    ah, af = videos(rng, [3, 3, 3])
    bh, bf = videos(rng, [3, 3, 3])
    bh[int(bf[0]) + 1] = flipped(ah[int(af[0]) + 2], t, rng)              # exactly on the tolerance
    bh[int(bf[1]) + 2] = flipped(ah[int(af[1]) + 0], min(t + 1, 1024), rng)  # one over (tolerances from 1024 on admit every cell)
    return Problem(ah, af, bh, bf, tol)


def _min_run(min_run):
    # X: one exact cell, 351; Y: two cells 200 off, 2 x 151 = 302; Z: sixteen cells 335 off, 16 x 16 = 256 - the filter decides
    return _pairs_problem(3, [(60, 60)], [(0, 2, 40, 1, 0), (0, 10, 20, 2, 200), (0, 30, 3, 16, 335)], min_run=min_run)


def _skip(whole):
    p = _pairs_problem(4, [(50, 45), (30, 30)], [(0, 10, 5, 20, (0, 30)), (1, 3, 8, 12, 10)])
    a_skip, b_skip = np.zeros(len(p.a_hashes), np.uint8), np.zeros(len(p.b_hashes), np.uint8)
    if whole:
        a_skip[int(p.a_first[0]) + 10:int(p.a_first[0]) + 30:2] = 1   # every other window of the run on A's side ...
        b_skip[int(p.b_first[0]) + 6:int(p.b_first[0]) + 25:2] = 7    # ... and the cells between them on B's side: pair 0 is silent
    else:
        a_skip[int(p.a_first[0]) + 20] = 1                              # cuts pair 0's run in two: 10 | 9
        b_skip[int(p.b_first[1]) + 8 + 4] = 255                         # and pair 1's: 4 | 7
    return p._replace(a_skip=a_skip, b_skip=b_skip)


def _static(ca, cb=None):
    rng = np.random.default_rng([77, 5])
    h = hashgen.random_hashes(rng, 1)
    ah = np.repeat(h, sum(ca), axis=0)
    if cb is None:
        return Problem(ah, first_of(ca), None, None, 350)
    return Problem(ah, first_of(ca), np.repeat(h, sum(cb), axis=0), first_of(cb), 350)


def _self_mode():
    rng = np.random.default_rng([77, 6])
    counts = [40, 90, 64, 130, 17, 65, 1, 100, 0, 33, 70, 128]
    ah, af = videos(rng, counts)
    for src, dst, ka, kb, n in ((0, 1, 5, 50, 30), (1, 3, 0, 66, 64), (2, 5, 10, 0, 54), (3, 7, 100, 3, 30), (4, 9, 0, 16, 17), (0, 10, 0, 30, 40),
                                (7, 11, 20, 60, 68), (5, 11, 1, 0, 50), (6, 10, 0, 69, 1)):
        plant(rng, ah, af, src, ka, ah, af, dst, kb, n, (0, 40))
    return Problem(ah, af, None, None, 350, 2)


def _band_neighbours(second_better):
    na = 100  # band 0 of the pair ends at offset -(na - 1) + 63 = -36, band 1 begins at -35
    return _pairs_problem(7, [(na, 90)], [(0, 40, 4, 10, 5 if second_better else 0), (0, 60, 25, 10, 0 if second_better else 5)])


CASES = {
    "mixed_counts": _mixed_counts,
    "first_diagonal": lambda: _pairs_problem(10, [(70, 50), (1, 1), (1, 40), (40, 1)], [(0, 69, 0, 1, 3), (1, 0, 0, 1, 0), (2, 0, 0, 1, 1), (3, 39, 0, 1, 2)]),
    "last_diagonal": lambda: _pairs_problem(11, [(70, 50), (2, 130), (130, 2)], [(0, 0, 49, 1, 3), (1, 0, 129, 1, 0), (2, 0, 1, 1, 9)]),
    "edges": lambda: _pairs_problem(12, [(80, 90)] * 4, [(0, 0, 17, 9, (0, 20)), (1, 23, 0, 9, (0, 20)), (2, 71, 30, 9, (0, 20)), (3, 12, 81, 9, (0, 20))]),
    "reload_wrap": lambda: _pairs_problem(13, [(200, 200), (200, 140)], [(0, 60, 65, 70, (0, 40)), (1, 60, 1, 70, (0, 40))]),
    "band_neighbours_first": lambda: _band_neighbours(False),
    "band_neighbours_second": lambda: _band_neighbours(True),
    "two_runs_one_diagonal": lambda: _pairs_problem(14, [(120, 120)], [(0, 5, 10, 12, 40), (0, 50, 55, 12, 4)]),
    "tie_two_diagonals": lambda: _pairs_problem(15, [(90, 90), (90, 90)], [(0, 50, 60, 8, 0), (0, 10, 3, 8, 0), (1, 10, 3, 8, 6), (1, 50, 60, 8, 6)]),
    "tie_one_diagonal": lambda: _pairs_problem(16, [(90, 90)], [(0, 40, 47, 6, 2), (0, 8, 15, 6, 2)]),
    **{f"tolerance_{t}": functools.partial(_tolerance, t) for t in (0, 1, 350, 1024, 5000)},
    **{f"min_run_{m}": functools.partial(_min_run, m) for m in (1, 2, 16)},
    "skip_cuts": lambda: _skip(False),
    "skip_silences": lambda: _skip(True),
    "static_equal": lambda: _static([70], [70]),
    "static_a_shorter": lambda: _static([40, 3], [100, 64]),
    "static_a_longer": lambda: _static([129], [65]),
    "static_self": lambda: _static([30, 70, 64, 1]),
    "self_mode": _self_mode,
}


@functools.lru_cache(maxsize=None)
def case(name: str) -> Problem:
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name: str) -> tuple:
    return tuple(align_twin(case(name)))


def random_problem(rng) -> Problem:
    """a small problem of a few videos of 0 .. 12 windows out of a pool of 4 related hashes: runs, ties and edges everywhere"""
    pool = hashgen.random_hashes(rng, 2)
    pool = np.concatenate([pool, np.stack([flipped(pool[0], 3, rng), flipped(pool[1], 5, rng)])])

    def side():
        counts = [int(rng.integers(0, 13)) for _ in range(int(rng.integers(1, 5)))]
        return pool[rng.integers(0, len(pool), size=sum(counts))].reshape(-1, 16), first_of(counts)
    ah, af = side()
    tol, min_run = int(rng.choice([0, 3, 4, 5, 8, 350])), int(rng.integers(1, 4))
    a_skip = (rng.random(len(ah)) < 0.15).astype(np.uint8) if rng.random() < 0.5 else None
    if rng.random() < 0.4:
        return Problem(ah, af, None, None, tol, min_run, a_skip)
    bh, bf = side()
    b_skip = (rng.random(len(bh)) < 0.15).astype(np.uint8) if rng.random() < 0.5 else None
    return Problem(ah, af, bh, bf, tol, min_run, a_skip, b_skip)
