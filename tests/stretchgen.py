"""Shared by the tests of the align-stretches calls: a numpy twin of the definition in include/vdf.h
(vdf_align_windows_stretches) and the problems both the CPU test of the host form and the GPU test of the masked band kernel solve.  numpy,
tests/aligngen.py and tests/hashgen.py only: nothing is imported from the library.  Records are compared for equality.

The twin is aligngen.best_run in a loop: after every reported stretch its rectangle - the stretch's rows of A x its rows of B, each widened by
`guard` windows and clipped to the matrix - is cleared in `ok`, so that its cells are misses for every later rank."""
from __future__ import annotations

import functools

import numpy as np

import aligngen
import hashgen

MAX_STRETCHES = 8


def rect_of(offset, start_a, n, guard, na, nb):
    """-> (a_lo, a_hi, b_lo, b_hi): the rectangle a reported stretch masks, in plain python integers (nothing wraps)"""
    start_b = start_a + offset
    return max(0, start_a - guard), min(na, start_a + n + guard), max(0, start_b - guard), min(nb, start_b + n + guard)


def pair_stretches(dist, ok, tol, min_run, max_stretches, guard):
    """one pair -> [(offset, start_a, n_windows, dist_sum, rank)]"""
    ok = ok.copy()
    na, nb = dist.shape
    out = []
    for rank in range(max_stretches):
        r = aligngen.best_run(dist, ok, tol, min_run)
        if r is None:
            break
        out.append(r + (rank,))
        a_lo, a_hi, b_lo, b_hi = rect_of(r[0], r[1], r[2], guard, na, nb)
        ok[a_lo:a_hi, b_lo:b_hi] = False
    return out


def stretches_twin(p: aligngen.Problem, max_stretches: int, guard: int):
    """-> the records [(a, b, offset, start_a, n_windows, dist_sum, rank)] in (a, b, rank) order"""
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
            out += [(a, b) + r for r in pair_stretches(dist[a0:a1, b0:b1], ok[a0:a1, b0:b1], tol, p.min_run, max_stretches, guard)]
    return out


def records(rec) -> list:
    """a structured array of the library's (ALIGN_STRETCH_DTYPE) as the twin's tuples"""
    return [tuple(int(r[k]) for k in ("a", "b", "offset", "start_a", "n_windows", "dist_sum", "rank")) for r in rec]


# ---- builders ---------------------------------------------------------------------------------------------------------------------------
def _one_pair(seed, na, nb, plants, tol=350, min_run=1):
    return aligngen._pairs_problem(seed, [(na, nb)], [(0,) + p for p in plants], tol, min_run)


SLOW_SEED = 21
SLOW_GUARD = 6  # the smallest guard that leaves slow_content_echo with one record (test_align_stretches_host.py searches for it again)


def _slow_content_echo():
    """A changes slowly - every window is the one before with 60 bits changed - and B[30, 60) = A[20, 50): the neighbouring diagonals match too"""
    rng = np.random.default_rng([78, SLOW_SEED])
    ah = np.zeros((90, 16), np.uint64)
    ah[0] = hashgen.random_hashes(rng, 1)[0]
    for i in range(1, 90):
        ah[i] = hashgen.hash_with_spatial_distance(ah[i - 1], 60, rng)
    bh = hashgen.random_hashes(rng, 90)
    bh[30:60] = ah[20:50]
    return aligngen.Problem(ah, aligngen.first_of([90]), bh, aligngen.first_of([90]), 350, 3)


def _rect_across_bands():
    """200 x 200.  Rank 0 is A[60, 130) -> B[65, 135) (offset 5): its rectangle spans the diagonals -65 ... 74 - three bands - and its rows of B
    wrap the 64-row reload.  A[60, 130) has period 35, continued down to row 48 of A and, through the copy, up to row 147 of B: so diagonal 40
    holds ONE run of 59 cells, A[48, 107) -> B[88, 147), which the rectangle cuts into A[48, 60) and A[95, 107).  A[140, 170) -> B[10, 40)
    (offset -130) lies on a diagonal that passes beside the rectangle."""
    rng = np.random.default_rng([78, 2])
    ah, af = aligngen.videos(rng, [200])
    bh, bf = aligngen.videos(rng, [200])
    for k in range(95, 130):
        ah[k] = ah[k - 35]
    ah[48:60] = ah[83:95]
    bh[65:135] = ah[60:130]
    bh[135:147] = bh[100:112]
    aligngen.plant(rng, ah, af, 0, 140, bh, bf, 0, 10, 30, (0, 40))
    return aligngen.Problem(ah, af, bh, bf, 350)


def _min_run_after_mask(min_run=8):
    """A[20, 60) -> B[30, 70) (offset 10), and A[20, 60) has period 20, continued down to row 14: diagonal 30 holds a run of 26 cells,
    A[14, 40) -> B[44, 70), of which the rectangle of rank 0 leaves 6 - under min_run = 8"""
    rng = np.random.default_rng([78, 3])
    ah, af = aligngen.videos(rng, [80])
    bh, bf = aligngen.videos(rng, [90])
    ah[40:60] = ah[20:40]
    ah[14:20] = ah[34:40]
    bh[30:70] = ah[20:60]
    return aligngen.Problem(ah, af, bh, bf, 350, min_run)


BUILDERS = {
    "ad_removed": lambda: _one_pair(1, 200, 170, [(0, 0, 100, (0, 40)), (130, 100, 70, (0, 40))]),
    "repeat_in_b": lambda: _one_pair(2, 90, 150, [(20, 5, 30, (0, 40)), (25, 100, 30, (0, 40))]),
    "two_runs_one_diagonal": aligngen.CASES["two_runs_one_diagonal"],
    "static_tiles": lambda: aligngen._static([40], [100]),
    "slow_content_echo": _slow_content_echo,
    "rect_across_bands": _rect_across_bands,
    "guard_clipped": lambda: _one_pair(3, 60, 80, [(0, 50, 30, (0, 40)), (33, 10, 17, (0, 40))]),
    "min_run_after_mask": _min_run_after_mask,
    **{k: aligngen.CASES[k] for k in ("self_mode", "skip_cuts", "mixed_counts", "static_self", "static_a_shorter", "tolerance_5000")},
}
# the guards every case runs at (with max_stretches = 8; smaller max_stretches are the same records up to that rank)
GUARDS = {**{k: (0, 2) for k in BUILDERS}, "slow_content_echo": (0, SLOW_GUARD), "guard_clipped": (5,)}
CASES = sorted((name, g) for name in BUILDERS for g in GUARDS[name])


@functools.lru_cache(maxsize=None)
def case(name: str) -> aligngen.Problem:
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def expected(name: str, guard: int, max_stretches: int = MAX_STRETCHES) -> tuple:
    """the twin's records; a smaller max_stretches only drops the later ranks (rank r does not depend on it), so the walk is made once"""
    if max_stretches != MAX_STRETCHES:
        return tuple(r for r in expected(name, guard) if r[6] < max_stretches)
    return tuple(stretches_twin(case(name), MAX_STRETCHES, guard))
