"""Shared by the tests of the seed calls and of the align calls on a list of pairs: a numpy twin of the definitions in
include/vdf.h (vdf_align_seed_pairs, vdf_align_windows_pairs, vdf_align_windows_stretches_pairs) and the problems both the CPU tests of the
host forms and the GPU tests of the seed kernel solve.  numpy, tests/aligngen.py, tests/stretchgen.py and tests/hashgen.py only: nothing is
imported from the library.  Pairs and records are compared for equality.

The candidate set comes from the full distance matrix: pair (a, b) is a candidate iff some cell (ka, kb) matches with ka - counted inside
video a - a multiple of min_run.  The restricted records are the all-pairs twins' filtered by pair."""
from __future__ import annotations

import functools

import numpy as np

import aligngen
import hashgen
import stretchgen


def _matrices(p: aligngen.Problem):
    self_mode = p.b_hashes is None
    bh, bf, bs = (p.a_hashes, p.a_first, p.a_skip) if self_mode else (p.b_hashes, p.b_first, p.b_skip)
    dist = hashgen.all_distances(p.a_hashes, bh) if len(p.a_hashes) and len(bh) else np.zeros((len(p.a_hashes), len(bh)), np.int64)
    ska = np.zeros(len(p.a_hashes), bool) if p.a_skip is None else np.asarray(p.a_skip) != 0
    skb = np.zeros(len(bh), bool) if bs is None else np.asarray(bs) != 0
    return self_mode, bf, dist, ~ska[:, None] & ~skb[None, :]


def seed_twin(p: aligngen.Problem, min_run=None) -> list:
    """-> the candidate pairs [(a, b)] in (a, b) order"""
    tol = min(int(p.tol), 1024)
    m = int(p.min_run if min_run is None else min_run)
    self_mode, bf, dist, ok = _matrices(p)
    match = ok & (dist <= tol)
    out = []
    for a in range(len(p.a_first) - 1):
        a0, a1 = int(p.a_first[a]), int(p.a_first[a + 1])
        rows = match[a0:a1:m]  # ka = 0, m, 2 m, ... of the video's own windows
        for b in range(a + 1 if self_mode else 0, len(bf) - 1):
            if rows[:, int(bf[b]):int(bf[b + 1])].any():
                out.append((a, b))
    return out


def pairs_twin(p: aligngen.Problem, pairs) -> list:
    """align_twin's records of the listed pairs"""
    want = set(map(tuple, pairs))
    return [r for r in aligngen.align_twin(p) if (r[0], r[1]) in want]


def stretches_pairs_twin(p: aligngen.Problem, pairs, max_stretches: int, guard: int) -> list:
    want = set(map(tuple, pairs))
    return [r for r in stretchgen.stretches_twin(p, max_stretches, guard) if (r[0], r[1]) in want]


def pairs_of(arr) -> list:
    """a structured array of the library's (VIDEO_PAIR_DTYPE) as the twin's tuples"""
    return [(int(r["a"]), int(r["b"])) for r in arr]


def all_pairs(p: aligngen.Problem) -> list:
    n_a = len(p.a_first) - 1
    if p.b_hashes is None:
        return [(a, b) for a in range(n_a) for b in range(a + 1, n_a)]
    return [(a, b) for a in range(n_a) for b in range(len(p.b_first) - 1)]


def sublist(p: aligngen.Problem, seed: int) -> list:
    """a hand-made sublist: about half of the call's pairs, in order"""
    rng = np.random.default_rng([79, seed])
    return [ab for ab in all_pairs(p) if rng.random() < 0.5]


# ---- builders ---------------------------------------------------------------------------------------------------------------------------
def phases(min_run: int, self_mode: bool = False) -> aligngen.Problem:
    """Runs of EXACTLY min_run windows that start at every residue 0 ... min_run - 1 of ka, one per pair, in videos whose first[v] is not a
    multiple of min_run.  Video 2 r of A holds the run of residue r at ka = min_run + r and pairs with video 2 r + 1 of B (self mode: with
    video 2 r + 2); the videos between them are one or two windows long, which puts every later first[v] off the array's grid.
    A run of min_run rows holds a multiple of min_run on ANY grid, so what tells a filter that samples every min_run-th row of the array
    from one that samples every min_run-th window of the VIDEO is the single cell: window 0 of video 2 r of A - a seed by the definition,
    off the array's grid - is also planted alone into the short video beside it (video 2 r of B; self mode: video 2 r + 1), a pair that
    is a candidate only through that seed."""
    rng = np.random.default_rng([79, 1, min_run, int(self_mode)])
    n = 3 * min_run + 2
    counts = []
    for r in range(min_run):
        counts += [n, 1 if (sum(counts) + n + 1) % min_run else 2]
    ah, af = aligngen.videos(rng, counts)
    assert min_run == 1 or all(int(af[2 * r]) % min_run for r in range(1, min_run)), "the videos must start off the array's grid"
    if self_mode:
        # the copy sits in the NEXT even video (the last one: in the odd one beside it, one window long, if min_run is 1)
        for r in range(min_run - 1):
            aligngen.plant(rng, ah, af, 2 * r, min_run + r, ah, af, 2 * r + 2, 1, min_run)
        for r in range(min_run):
            aligngen.plant(rng, ah, af, 2 * r, 0, ah, af, 2 * r + 1, 0, 1, 2)
        return aligngen.Problem(ah, af, None, None, 350, min_run)
    bh, bf = aligngen.videos(rng, [1 if i % 2 == 0 else n for i in range(2 * min_run)])
    for r in range(min_run):
        aligngen.plant(rng, ah, af, 2 * r, min_run + r, bh, bf, 2 * r + 1, 1 + r, min_run)
        aligngen.plant(rng, ah, af, 2 * r, 0, bh, bf, 2 * r, 0, 1, 2)
    return aligngen.Problem(ah, af, bh, bf, 350, min_run)


def tile_edges(self_mode: bool, min_run: int = 2, tol: int = 350) -> aligngen.Problem:
    """About 40 videos of 0 ... 60 windows per side: more than one tile of 512 rows of B and not a whole number of them, a video across the
    tile edge, more than one chunk of 256 seeds, empty videos first, last and in between; copies planted across all of it."""
    rng = np.random.default_rng([79, 2, int(self_mode)])

    def counts():
        c = [int(rng.integers(0, 61)) for _ in range(40)]
        c[0] = c[-1] = c[7] = c[8] = c[21] = 0
        return c
    ca = counts()
    ah, af = aligngen.videos(rng, ca)
    if self_mode:
        cb, bh, bf = ca, ah, af
    else:
        cb = counts()
        bh, bf = aligngen.videos(rng, cb)
    total_b = int(bf[-1])
    assert total_b > 512 and total_b % 512 and any(int(bf[v]) < 512 < int(bf[v + 1]) for v in range(len(cb))), "tiles: more than one, a ragged last, a video across"
    assert min_run > 3 or -(-int(af[-1]) // min_run) > 256, "more than one chunk of seeds"
    live_a, live_b = [v for v, n in enumerate(ca) if n >= 6], [v for v, n in enumerate(cb) if n >= 6]
    for _ in range(30):
        a, b = int(rng.choice(live_a)), int(rng.choice(live_b))
        if self_mode and a >= b:
            continue
        n = int(rng.integers(1, min(ca[a], cb[b]) + 1))
        aligngen.plant(rng, ah, af, a, int(rng.integers(0, ca[a] - n + 1)), bh, bf, b, int(rng.integers(0, cb[b] - n + 1)), n, (0, 40))
    return aligngen.Problem(ah, af, None if self_mode else bh, None if self_mode else bf, tol, min_run)


def skipped_seeds() -> aligngen.Problem:
    """Video 0 of A: its only seeds (ka = 0, 3, 6, ...) are skipped, and its copy in B starts on one - no candidate, though the unskipped
    windows match.  Video 1 of A is skipped whole.  Video 2 of A is copied into video 2 of B, which is skipped whole, and into video 3 of B,
    where only the window opposite the seed is skipped.  Video 3 of A is the control: a copy nobody skips."""
    rng = np.random.default_rng([79, 3])
    ah, af = aligngen.videos(rng, [12, 9, 12, 10])
    bh, bf = aligngen.videos(rng, [20, 9, 12, 12, 15])
    aligngen.plant(rng, ah, af, 0, 0, bh, bf, 0, 4, 12, 5)
    aligngen.plant(rng, ah, af, 1, 0, bh, bf, 1, 0, 9, 5)
    aligngen.plant(rng, ah, af, 2, 0, bh, bf, 2, 0, 12, 5)
    aligngen.plant(rng, ah, af, 2, 3, bh, bf, 3, 0, 3, 5)   # seed ka = 3 against kb = 0, skipped below; ka = 4, 5 are no seeds
    aligngen.plant(rng, ah, af, 3, 2, bh, bf, 4, 6, 8, 5)
    a_skip, b_skip = np.zeros(len(ah), np.uint8), np.zeros(len(bh), np.uint8)
    a_skip[int(af[0]):int(af[1]):3] = 1
    a_skip[int(af[1]):int(af[2])] = 9
    b_skip[int(bf[2]):int(bf[3])] = 1
    b_skip[int(bf[3])] = 255
    return aligngen.Problem(ah, af, bh, bf, 350, 3, a_skip, b_skip)


def early_exit(tol: int = 350) -> aligngen.Problem:
    """Three one-window pairs at the tolerance, for the exit after the first dwords of a hash (the kernel tests after 14, 22 or 26 of the 32
    dwords = 7, 11 or 13 of the 16 words): exactly tol apart with every differing bit in the LAST words (the partial distance is 0 where the
    kernel looks first), exactly tol apart with every differing bit in the FIRST words (the partial distance is already tol there), and
    tol + 1 apart with the differing bits packed into the last words - at tol <= 167 the first 13 words are equal, so there is nothing to
    see at any exit and the full distance decides; a larger tol + 1 does not fit behind the exit and spills forward.  Hits: the first two."""
    rng = np.random.default_rng([79, 4])
    ah, af = aligngen.videos(rng, [1, 1, 1])
    bh = ah.copy()

    def flip_bits(row, bits):
        for bit in bits:
            bh[row, bit // 64] ^= np.uint64(1) << np.uint64(bit % 64)
    usable = [w * 64 + i for w in range(16) for i in range(64 if w < 15 else 40)]  # the 1000 bits of a hash: word 15 holds 40
    last = [b for b in usable if b >= 10 * 64]      # 360 bits in words 10 ... 15
    tail = [b for b in usable if b >= 13 * 64]      # 168 bits in words 13 ... 15: behind every exit point
    assert tol <= len(last) and tol + 1 <= len(usable)
    flip_bits(0, last[-tol:] if tol else [])
    flip_bits(1, usable[:tol])
    flip_bits(2, (tail + [b for b in usable if b < 13 * 64][::-1])[:tol + 1] if tol + 1 > len(tail) else tail[:tol + 1])
    return aligngen.Problem(ah, af, bh, af.copy(), tol, 1)


BUILDERS = {
    **{f"phases_{m}": functools.partial(phases, m) for m in (1, 2, 3, 4, 5, 6)},
    **{f"phases_self_{m}": functools.partial(phases, m, True) for m in (2, 3, 5)},
    "tile_edges": functools.partial(tile_edges, False),
    "tile_edges_self": functools.partial(tile_edges, True),
    "tile_edges_tol0": functools.partial(tile_edges, False, 3, 0),
    "tile_edges_all": functools.partial(tile_edges, False, 2, 1024),
    "tile_edges_self_all": functools.partial(tile_edges, True, 2, 1024),
    "tile_edges_min_run_1": functools.partial(tile_edges, True, 1),
    "tile_edges_min_run_above": functools.partial(tile_edges, False, 61),
    "skipped_seeds": skipped_seeds,
    "early_exit": early_exit,
    "early_exit_tol_100": functools.partial(early_exit, 100),
}


@functools.lru_cache(maxsize=None)
def case(name: str) -> aligngen.Problem:
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def expected(name: str) -> tuple:
    return tuple(seed_twin(case(name)))


@functools.lru_cache(maxsize=None)
def expected_records(name: str) -> tuple:
    return tuple(aligngen.align_twin(case(name)))
