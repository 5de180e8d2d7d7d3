"""Seeded random problems for every align entry point (vdf_align_* and vdf_window_*) AT THE SIZES WHERE THE
KERNELS' STRUCTURE IS EXERCISED - what the hand-built cases of aligngen, stretchgen, seedgen, variantgen, seedvariantgen and retimedaligngen aim at
one situation at a time.  Shared by tests/test_align_fuzz_host.py (the _host definitions against the numpy twins, and the conditions that
keep this generator from being vacuous) and tests/test_gpu_align_fuzz.py (every device and host-array form against the _host definitions).
numpy, tests/hashgen.py and aligngen.Problem only: nothing is imported from the library, and its constants are WRITTEN DOWN here, not imported.

problem(seed, profile) is deterministic from np.random.default_rng([FUZZ, seed]) (its child stream number PROFILES.index(profile)).  The profiles, and the constant each size comes from:

  bands      2 - 5 videos per side; window counts from {0, 1, 2, 63, 64, 65, 127, 128, 129, 190 ... 260} and uniform 1 ... 260.
             kAlignBand = 64 (align_plan.h): 1 - 8 bands of 64 diagonals per pair, several reloads of a lane's row per band (a lane holds row
             kb of B as long as kb mod 64 is its number: align_row_lane), both orientations of the matrix, empty videos.
  tiles      B: 520 - 1100 windows = 2 - 3 seed tiles (kSeedTileRows = 512, align_plan.h) and 3 - 5 variant tiles (kSeedVariantsTileRows = 256),
             a video across every tile edge (no video begins on a multiple of 256), the last tile partly padding (the `wave_row0 >= n_rows` exit
             of both seed kernels, align.hip).  A: 300 - 700 windows at min_run 1, 540 - 700 at min_run 2 (the profile draws min_run from these two):
             more than one chunk of seeds (kSeedChunk = 256) with a partial last one, seeds of one video split over two chunks.  In self mode A has
             B's shape (700 - 1100 windows).  One exact copy nobody skips is planted behind chunk 0 and tile 0: the seed call always has a hit there.
  many_tiny  60 - 130 videos per side of 0 - 4 windows: 3 600 - 16 900 pairs - more than kAlignWaves = 4 (pair, band) units per workgroup, more
             than the 256 pairs of one block of the reductions (align.hip: 256 threads, one pair each), a pair bitmap of several hundred words -
             past the 256 words of one count block - with n_b no multiple of 32, so that a word holds bits of two values of a; the variants
             bitmap is up to seven of these one after the other.

reduced=True: the same draws at the size the numpy twins can walk cell by cell - bands: at most 3 videos per side of at most 140 windows (the
edges at 64 and 128 stay); tiles: B 520 - 600 windows, A just over one chunk of seeds; many_tiny: 60 - 95 videos per side.

The content is drawn independently of the profile - `pool` (every window out of 4 - 8 related hashes, some of them exactly on the tolerance:
dense matches, ties on every level, runs on all four edges), `planted` (a random background with 1 - 6 runs per related pair: lengths
above 64, runs that end on the last row or column, flips of tol - 3 ... tol + 3 bits per window placed in the last eight dwords, the first
fourteen or anywhere - what the four early-exit instantiations of the seed kernel, 14 / 22 / 26 / 32 check dwords, must and may drop), `static`
(one hash all over part of the videos, most of those windows skipped) - and so are the tolerance, min_run (a value more than half the
longest video is mostly drawn again below it: it would silence every call), the skip arrays (absent, 5 - 15 % or 60 %, in bursts), self mode, the
zero planes (H & Z == 0), the variant mask, the rate, max_stretches and the guard.  Lines of the rate's slope and stretches under a variant are
planted too.  Every plant reads A and writes B, in a shuffled order.  Nothing here is an error by include/vdf.h."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

import aligngen
import hashgen

FUZZ = 4171                      # the file's constant: problem(seed, ...) draws from default_rng([FUZZ, seed])
PROFILES = ("bands", "tiles", "many_tiny")
CONTENTS = ("pool", "planted", "static")

# ---- the library's constants, written down (a change there must be made here by hand: that is the point) ---------------------------------------
ALIGN_BAND = 64                  # align_plan.h kAlignBand: diagonals per band = lanes of a wave = rows of B a band holds at a time
ALIGN_WAVES = 4                  # align_plan.h kAlignWaves: (pair, band) units per workgroup
REDUCE_BLOCK = 256               # align.hip: align_reduce_kernel / align_scatter_kernel / align_seed_count_kernel, __launch_bounds__(256), one item per thread
SEED_TILE_ROWS = 512             # align_plan.h kSeedTileRows = 256 * kSeedRowsPerLane
SEED_VARIANTS_TILE_ROWS = 256    # align_plan.h kSeedVariantsTileRows
SEED_CHUNK = 256                 # align_plan.h kSeedChunk: seeds per unit
CHECK_WORDS = (14, 22, 26, 32)   # align.hip: the instantiations of align_seed_kernel's early exit

# 179 | 180, 297 | 298, 357 | 358: where check_words() below changes (tests/test_align_fuzz_host.py holds it against align_seed_check_words itself)
TOLERANCES = (0, 1, 179, 180, 297, 298, 350, 357, 358, 511, 1023, 1024, 5000)
MIN_RUNS = (1, 2, 3, 4, 5, 7, 16, 65)
RATES = ((1, 1), (25, 24), (6, 5), (5, 4), (3, 2), (2, 1), (32, 17))
MAX_STRETCHES = (1, 2, 4, 8)
GUARDS = (0, 1, 5, 1 << 20)
BAND_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129)

_ANY = np.arange(1000)
_LAST8 = np.arange(24 * 32, 1000)     # dwords 24 ... 31: behind every early exit
_FIRST14 = np.arange(0, 14 * 32)      # dwords 0 ... 13: in front of every early exit
_PLACEMENTS = {"any": _ANY, "last8": _LAST8, "first14": _FIRST14}


def check_words(tol: int) -> int:
    """align_plan.h align_seed_check_words, restated: the first w of 14, 22, 26 with 16 w >= tol + 1 + 2 (floor(sqrt(32 w)) + 1), else 32"""
    for w in CHECK_WORDS[:3]:
        if 16 * w >= tol + 1 + 2 * (int(np.floor(np.sqrt(32 * w))) + 1):
            return w
    return 32


class FuzzProblem(NamedTuple):
    p: aligngen.Problem             # the problem of the plain, stretches, seed and variants calls (self mode: b_hashes None)
    two: aligngen.Problem           # the two-sided draw (A is p's): what the retimed calls take; p itself unless p is in self mode
    a_zero: np.ndarray              # zero planes of both sides, H & Z == 0
    b_zero: np.ndarray
    mask: int                       # variant mask, bits 1 ... 7
    rate: tuple
    max_stretches: int
    guard: int
    pairs: np.ndarray               # [n, 2]: a strictly increasing sublist of p's pairs, pairs that name empty videos among them
    pairs_two: np.ndarray           # the same of `two` (pairs itself unless p is in self mode)
    triples: np.ndarray             # [n, 3] (variant, a, b): a strictly increasing sublist over all seven variants
    params: dict                    # what was drawn, for describe()

    @property
    def self_mode(self) -> bool:
        return self.p.b_hashes is None


# ---- bits ---------------------------------------------------------------------------------------------------------------------------------------
def _flip(h: np.ndarray, k: int, rng, region=_ANY) -> np.ndarray:
    """h with exactly min(k, 1000) of its bits 0 ... 999 changed: inside `region` as far as it reaches, the rest anywhere else"""
    k = int(min(max(k, 0), 1000))
    if k == 0:
        return h.copy()
    n1 = min(k, len(region))
    idx = rng.choice(region, size=n1, replace=False)
    if k > n1:
        idx = np.concatenate([idx, rng.choice(np.setdiff1d(_ANY, region), size=k - n1, replace=False)])
    bits = np.unpackbits(np.ascontiguousarray(h).view(np.uint8), bitorder="little")
    bits[idx] ^= 1
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


def _pack1000(bits: np.ndarray) -> np.ndarray:
    """[n, 1000] 0 / 1 -> [n, 16] u64"""
    b = np.zeros((len(bits), 1024), np.uint8)
    b[:, :1000] = bits
    return np.packbits(b, axis=1, bitorder="little").view(np.uint64).copy()


def variant_mask_words(v: int) -> np.ndarray:
    """M_v of include/vdf.h: bit i = 100 kt + 10 kx + ky is set iff (v0 kx + v1 ky + v2 kt) is odd"""
    i = np.arange(1000)
    kt, kx, ky = i // 100, (i // 10) % 10, i % 10
    return _pack1000(((((v & 1) * kx + ((v >> 1) & 1) * ky + ((v >> 2) & 1) * kt) & 1).astype(np.uint8))[None])[0]


def _planes(rng, hashes: np.ndarray, density: float) -> np.ndarray:
    if len(hashes) == 0 or density == 0.0:
        return np.zeros_like(hashes)
    return _pack1000((rng.random((len(hashes), 1000)) < density).astype(np.uint8)) & ~hashes


# ---- shapes -------------------------------------------------------------------------------------------------------------------------------------
def _band_counts(rng, reduced: bool) -> list:
    top = 140 if reduced else 260
    out = []
    for _ in range(int(rng.integers(2, 4 if reduced else 6))):
        if rng.random() < 0.5:
            c = int(rng.choice(BAND_COUNTS + ((int(rng.integers(130, 141)),) if reduced else (int(rng.integers(190, 261)),))))
        else:
            c = int(rng.integers(1, top + 1))
        out.append(c)
    if max(out) < 2 * ALIGN_BAND:  # one video of more than two bands' worth of windows on every side
        out[int(rng.integers(0, len(out)))] = int(rng.integers(130, top + 1))
    return out


def _tile_counts(rng, lo: int, hi: int) -> list:
    """videos of 0 ... 129 windows that add up to a total in [lo, hi]: the total no multiple of 256 and no video beginning on one"""
    for _ in range(1000):
        total = int(rng.integers(lo, hi + 1))
        out = []
        while sum(out) < total:
            kind = rng.random()
            out.append(min(0 if kind < 0.08 else int(rng.integers(1, 8)) if kind < 0.2 else int(rng.integers(20, 130)), total - sum(out)))
        first = np.cumsum(out)
        if total % SEED_VARIANTS_TILE_ROWS and not np.any(first[:-1] % SEED_VARIANTS_TILE_ROWS == 0):
            return out + [0] * int(rng.integers(0, 2))
    raise AssertionError("no tile shape found")


def _tiny_counts(rng, reduced: bool, not_multiple_of_32: bool) -> list:
    n = int(rng.integers(60, 96 if reduced else 131))
    if not_multiple_of_32 and n % 32 == 0:
        n += 1
    return [int(c) for c in rng.integers(0, 5, size=n)]


def _shapes(rng, profile: str, reduced: bool, self_mode: bool, min_run: int):
    if profile == "bands":
        return _band_counts(rng, reduced), _band_counts(rng, reduced)
    if profile == "many_tiny":
        return _tiny_counts(rng, reduced, self_mode), _tiny_counts(rng, reduced, True)
    assert profile == "tiles", profile
    b_range = (520, 600) if reduced else (520, 1100)
    if self_mode:       # A is its own B: two tiles of rows, and seeds behind chunk 0 that still have a later video to pair with
        a_range = (540, 600) if reduced else (700, 1100) if min_run == 1 else (800, 1100)
    elif reduced:
        a_range = (270, 320) if min_run == 1 else (530, 560)
    else:
        a_range = (300, 700) if min_run == 1 else (540, 700)
    return _tile_counts(rng, *a_range), _tile_counts(rng, *b_range)


# ---- content ------------------------------------------------------------------------------------------------------------------------------------
def _edge_flips(rng, t: int) -> int:
    return int(np.clip(rng.integers(t - 3, t + 4), 0, 1000))


def _pool_side(rng, pool, counts):
    return pool[rng.integers(0, len(pool), size=int(sum(counts)))].reshape(-1, 16).copy(), aligngen.first_of(counts)


def _pool(rng, t: int):
    """4 - 8 hashes: 2 - 4 unrelated ones and relatives of them - equal, a few bits off, and within 3 bits of the tolerance on either side"""
    pool = [h for h in hashgen.random_hashes(rng, int(rng.integers(2, 5)))]
    n_base = len(pool)
    while len(pool) < max(4, n_base + 1) or (len(pool) < 8 and rng.random() < 0.6):
        kind = rng.random()
        k = 0 if kind < 0.15 else int(rng.integers(1, 7)) if kind < 0.5 else _edge_flips(rng, t)
        pool.append(_flip(pool[int(rng.integers(0, n_base))], k, rng))
    return np.stack(pool)


def _copy_segments(rng, ah, af, bh, bf, self_mode: bool, n: int):
    """n times: a stretch of a video of A copied into a video of B (self mode: a later video of A) as it is - long runs, exact ties"""
    ca, cb = np.diff(af.astype(np.int64)), np.diff(bf.astype(np.int64))
    live_a, live_b = np.flatnonzero(ca > 0), np.flatnonzero(cb > 0)
    for _ in range(n):
        if not len(live_a) or not len(live_b):
            return
        a, b = int(rng.choice(live_a)), int(rng.choice(live_b))
        if self_mode and a >= b:
            continue
        m = int(rng.integers(1, min(ca[a], cb[b]) + 1))
        ka, kb = int(rng.integers(0, ca[a] - m + 1)), int(rng.integers(0, cb[b] - m + 1))
        bh[int(bf[b]) + kb:int(bf[b]) + kb + m] = ah[int(af[a]) + ka:int(af[a]) + ka + m]


def _plant_runs(rng, ah, af, a, bh, bf, b, t: int, log: list):
    """1 - 6 runs of pair (a, b): windows of b := windows of a with bits changed.  Per run: a length (often above 64 where the videos allow it),
    a position (often against the last row or column), a placement of the changed bits, and the share of windows that sit within 3 bits of the
    tolerance (the others are 0 ... 40 bits off, at most the tolerance)."""
    na, nb = int(af[a + 1] - af[a]), int(bf[b + 1] - bf[b])
    if na == 0 or nb == 0:
        return
    top = min(na, nb)
    for _ in range(int(rng.integers(1, 7))):
        kind = rng.random()
        n = int(rng.integers(min(65, top), top + 1)) if kind < 0.3 else int(rng.integers(1, min(top, 12) + 1)) if kind < 0.5 else int(rng.integers(1, top + 1))
        ka, kb = int(rng.integers(0, na - n + 1)), int(rng.integers(0, nb - n + 1))
        where = rng.random()
        if where < 0.15:
            ka = na - n           # ends on the last row
        elif where < 0.3:
            kb = nb - n           # ends on the last column
        elif where < 0.4:
            ka, kb = (0, kb) if rng.random() < 0.5 else (ka, 0)
        place = str(rng.choice(list(_PLACEMENTS)))
        edge_share = float(rng.choice([1.0, 0.3, 0.03], p=[0.15, 0.25, 0.6]))
        for i in range(n):
            k = _edge_flips(rng, t) if rng.random() < edge_share else int(rng.integers(0, min(t, 40) + 1))
            bh[int(bf[b]) + kb + i] = _flip(ah[int(af[a]) + ka + i], k, rng, _PLACEMENTS[place])
        log.append((a, b, ka, kb, n, place, edge_share))


def _plant_retimed(rng, ah, af, a, bh, bf, b, rate, t: int):
    """a line of slope num / den: row den (j0 + m) of b := row phase + num (i0 + m) of a, a few bits off"""
    num, den = rate
    na, nb = int(af[a + 1] - af[a]), int(bf[b + 1] - bf[b])
    phase = int(rng.integers(0, num))
    rows, cols = (na - phase + num - 1) // num if na > phase else 0, (nb + den - 1) // den
    if rows == 0 or cols == 0:
        return
    n = int(rng.integers(1, min(rows, cols) + 1))
    i0, j0 = int(rng.integers(0, rows - n + 1)), int(rng.integers(0, cols - n + 1))
    for m in range(n):
        k = _edge_flips(rng, t) if rng.random() < 0.1 else int(rng.integers(0, min(t, 40) + 1))
        bh[int(bf[b]) + den * (j0 + m)] = _flip(ah[int(af[a]) + phase + num * (i0 + m)], k, rng)


def _plant_variant(rng, ah, af, a, bh, bz, bf, b, v: int, t: int):
    """rows of b - hash AND plane - made so that the variant-v set of b shows windows of a at its derived rows kb ...: with x a window of a
    a few bits off and Z the row's plane without x's bits, H = (x ^ M_v) & ~Z gives (H ^ M_v) & ~Z = x and H & Z == 0.  With bit 2 of v the
    derived rows of b are its rows backwards.  Like every plant it writes B only (self mode: a later video of A)."""
    na, nb = int(af[a + 1] - af[a]), int(bf[b + 1] - bf[b])
    if na == 0 or nb == 0:
        return
    n = int(rng.integers(1, min(na, nb, 40) + 1))
    ka, kb = int(rng.integers(0, na - n + 1)), int(rng.integers(0, nb - n + 1))
    m = variant_mask_words(v)
    lo, hi = int(bf[b]), int(bf[b + 1])
    for i in range(n):
        dst = hi - 1 - (kb + i) if v & 4 else lo + kb + i
        k = _edge_flips(rng, t) if rng.random() < 0.1 else int(rng.integers(0, min(t, 40) + 1))
        x = _flip(ah[int(af[a]) + ka + i], k, rng)
        bz[dst] &= ~x
        bh[dst] = (x ^ m) & ~bz[dst]


def _related_pairs(rng, profile: str, n_a: int, n_b: int, self_mode: bool) -> list:
    if profile == "bands":
        out = [(a, b) for a in range(n_a) for b in range(n_b) if rng.random() < 0.8]
    else:
        n = int(rng.integers(30, 51)) if profile == "tiles" else int(rng.integers(n_a, 2 * n_a + 1))
        out = [(int(rng.integers(0, n_a)), int(rng.integers(0, n_b))) for _ in range(n)]
    return [(a, b) for a, b in out if not self_mode or a < b]


def _skip(rng, mode: str, n: int) -> Optional[np.ndarray]:
    """skip bytes (any non-zero value abstains) on 5 - 15 % (sparse) or 60 % (dense) of the windows, in bursts of 1 - 12 as static scenes come"""
    if mode == "absent":
        return None
    share = float(rng.uniform(0.05, 0.15)) if mode == "sparse" else 0.6
    sk = np.zeros(n, np.uint8)
    for _ in range(4 * n):
        if np.count_nonzero(sk) >= share * n:
            break
        at, m = int(rng.integers(0, n)), int(rng.integers(1, 13))
        sk[at:at + m] = rng.integers(1, 256, size=len(sk[at:at + m]))
    return sk


def _sublist(rng, n_a: int, n_b: int, ca, cb, self_mode: bool) -> np.ndarray:
    """about 40 % of the call's pairs in (a, b) order - 80 % of those that name a video without windows"""
    a, b = np.meshgrid(np.arange(n_a), np.arange(n_b), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    if self_mode:
        keep = a < b
        a, b = a[keep], b[keep]
    empty = (np.asarray(ca)[a] == 0) | (np.asarray(cb)[b] == 0)
    take = rng.random(len(a)) < np.where(empty, 0.8, 0.4)
    return np.stack([a[take], b[take]], axis=1).astype(np.int64)


def _triples(rng, n_a: int, n_b: int, self_mode: bool) -> np.ndarray:
    """about 15 % of all (variant, a, b), variants 1 ... 7 whatever the mask says, in order"""
    a, b = np.meshgrid(np.arange(n_a), np.arange(n_b), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    if self_mode:
        keep = a < b
        a, b = a[keep], b[keep]
    out = []
    for v in range(1, 8):
        take = rng.random(len(a)) < 0.15
        out.append(np.stack([np.full(int(take.sum()), v), a[take], b[take]], axis=1))
    return np.concatenate(out).astype(np.int64)


def _seeds_before(counts, min_run: int) -> np.ndarray:
    """[videos + 1]: the number of seeds (windows ka = 0, min_run, 2 min_run ... of every video) in front of video v"""
    return np.concatenate([[0], np.cumsum([-(-int(c) // min_run) for c in counts])])


def _tile_anchor(rng, ah, af, a_skip, bh, bf, b_skip, min_run: int, self_mode: bool):
    """an exact copy nobody skips, from a video of A whose seeds lie behind chunk 0 into a video of B whose rows lie behind tile 0 (self mode: a
    later video of A): the seed call has a hit outside the first tile and the first chunk whatever else was drawn.  -> (a, b) or None"""
    ca, cb = np.diff(af.astype(np.int64)), np.diff(bf.astype(np.int64))
    n = min_run + 1
    before = _seeds_before(ca, min_run)
    # (a, ka): a seed behind the first chunk with n windows of its video from it on
    cand_a = [(v, ka) for v in range(len(ca)) for ka in range(0, int(ca[v]) - n + 1, min_run) if before[v] + ka // min_run >= SEED_CHUNK]
    # (b, kb): n rows of one video behind the first tile
    cand_b = [(v, kb) for v in range(len(cb)) for kb in range(max(0, SEED_TILE_ROWS - int(bf[v])), int(cb[v]) - n + 1)]
    for i in rng.permutation(len(cand_a)).tolist():
        a, ka = cand_a[i]
        rows = [(v, kb) for v, kb in cand_b if not self_mode or a < v]
        if rows:
            b, kb = rows[int(rng.integers(0, len(rows)))]
            break
    else:
        return None
    bh[int(bf[b]) + kb:int(bf[b]) + kb + n] = ah[int(af[a]) + ka:int(af[a]) + ka + n]
    if self_mode:  # the copy must not run into its own source (a < b: other rows) - and A's skip array is B's
        b_skip = a_skip
    if a_skip is not None:
        a_skip[int(af[a]) + ka:int(af[a]) + ka + n] = 0
    if b_skip is not None:
        b_skip[int(bf[b]) + kb:int(bf[b]) + kb + n] = 0
    return a, ka, b, kb


# ---- the generator ------------------------------------------------------------------------------------------------------------------------------
def problem(seed: int, profile: str, reduced: bool = False) -> FuzzProblem:
    # one child stream per profile: seed s of one profile shares no draw with seed s of another
    rng = np.random.default_rng([FUZZ, int(seed)]).spawn(len(PROFILES))[PROFILES.index(profile)]
    self_mode = bool(rng.random() < 1 / 3)
    content = str(rng.choice(CONTENTS, p=[0.4, 0.4, 0.2]))
    tol = int(rng.choice(TOLERANCES))
    t = min(tol, 1024)
    min_run = int(rng.choice(MIN_RUNS))
    skip_modes = [str(rng.choice(["absent", "sparse", "dense"], p=[0.4, 0.4, 0.2])) for _ in range(2)]
    density = 0.0 if rng.random() < 0.15 else float(rng.uniform(0.0, 0.4))
    mask = int(rng.integers(1, 128)) << 1
    rate = RATES[int(rng.integers(0, len(RATES)))]
    max_stretches = int(rng.choice(MAX_STRETCHES, p=[0.1, 0.15, 0.35, 0.4]))
    guard = int(rng.choice(GUARDS, p=[0.35, 0.3, 0.25, 0.1]))
    if profile == "tiles":
        min_run = int(rng.choice([1, 2]))       # the profile's own: more than one chunk of seeds out of 300 - 700 windows
    ca, cb = _shapes(rng, profile, reduced, self_mode, min_run)
    longest = max(ca) if self_mode else min(max(ca), max(cb))
    if 2 * min_run > longest and rng.random() < 0.85:
        # a min_run that no video or hardly one can reach silences every call: mostly one of the list up to half the longest video (many_tiny: 1, 2)
        min_run = int(rng.choice([m for m in MIN_RUNS if m <= max(longest // 2, 1)]))

    # content.  The two-sided draw always; in self mode the same relations inside A as well.  Every plant READS windows of A and WRITES windows of B
    # (self mode: of a later video of A), in a shuffled order: a later one trims an earlier one, none is undone from the other side.
    plants: list = []
    todo: list = []
    if content == "pool":
        pool = _pool(rng, t)
        (ah, af), (bh, bf) = _pool_side(rng, pool, ca), _pool_side(rng, pool, cb)
        todo.append(lambda: _copy_segments(rng, ah, af, bh, bf, False, int(rng.integers(0, 4))))
        if self_mode:
            todo.append(lambda: _copy_segments(rng, ah, af, ah, af, True, int(rng.integers(1, 6))))
    else:
        (ah, af), (bh, bf) = aligngen.videos(rng, ca), aligngen.videos(rng, cb)
        if content == "static":
            s = hashgen.random_hashes(rng, 1)[0]
            static_a, static_b = rng.random(len(ca)) < rng.uniform(0.3, 0.6), rng.random(len(cb)) < rng.uniform(0.3, 0.6)
            for h, f, st in ((ah, af, static_a), (bh, bf, static_b)):
                for v in np.flatnonzero(st):
                    h[int(f[v]):int(f[v + 1])] = s
            skip_modes = ["sparse" if m == "absent" else m for m in skip_modes]
        for a, b in _related_pairs(rng, profile, len(ca), len(cb), False):
            todo.append(lambda a=a, b=b: _plant_runs(rng, ah, af, a, bh, bf, b, t, plants))
        if self_mode:
            for a, b in _related_pairs(rng, profile, len(ca), len(ca), True):
                todo.append(lambda a=a, b=b: _plant_runs(rng, ah, af, a, ah, af, b, t, plants))
        if rate != (1, 1):  # lines of the rate's slope
            for a, b in _related_pairs(rng, profile, len(ca), len(cb), False)[:{"bands": 4, "tiles": 20, "many_tiny": 60}[profile]]:
                todo.append(lambda a=a, b=b: _plant_retimed(rng, ah, af, a, bh, bf, b, rate, t))
    # zero planes, and stretches under a variant: rows of B (self mode: of A) whose variant set shows windows of A
    a_zero, b_zero = _planes(rng, ah, density), _planes(rng, bh, density)
    variants = [v for v in range(1, 8) if mask >> v & 1]
    for a, b in _related_pairs(rng, profile, len(ca), len(ca) if self_mode else len(cb), self_mode)[:{"bands": 4, "tiles": 12, "many_tiny": 40}[profile]]:
        v = int(rng.choice(variants)) if rng.random() < 0.8 else int(rng.integers(1, 8))
        if self_mode:
            todo.append(lambda a=a, b=b, v=v: _plant_variant(rng, ah, af, a, ah, a_zero, af, b, v, t))
        else:
            todo.append(lambda a=a, b=b, v=v: _plant_variant(rng, ah, af, a, bh, b_zero, bf, b, v, t))
    for i in rng.permutation(len(todo)).tolist():
        todo[i]()
    a_skip, b_skip = _skip(rng, skip_modes[0], len(ah)), _skip(rng, skip_modes[1], len(bh))
    if content == "static":  # most of the static windows abstain
        for h, f, st, sk in ((ah, af, static_a, a_skip), (bh, bf, static_b, b_skip)):
            for v in np.flatnonzero(st):
                lo, hi = int(f[v]), int(f[v + 1])
                keep = int(rng.integers(0, (hi - lo) // 4 + 1))   # all but one stretch of at most a quarter of the video
                at = lo + int(rng.integers(0, hi - lo - keep + 1))
                kept = sk[at:at + keep].copy()
                sk[lo:hi] = rng.integers(1, 256, size=hi - lo)
                sk[at:at + keep] = kept
    anchor = None
    if profile == "tiles":
        anchor = _tile_anchor(rng, ah, af, a_skip, ah if self_mode else bh, af if self_mode else bf, b_skip, min_run, self_mode)
        assert reduced or anchor is not None, "tiles: no video behind the first chunk of seeds and the first tile of rows"
    a_zero, b_zero = a_zero & ~ah, b_zero & ~bh   # the header's H & Z == 0, whatever was planted since

    two = aligngen.Problem(ah, af, bh, bf, tol, min_run, a_skip, b_skip)
    p = aligngen.Problem(ah, af, None, None, tol, min_run, a_skip, None) if self_mode else two
    pairs_two = _sublist(rng, len(ca), len(cb), ca, cb, False)
    pairs = _sublist(rng, len(ca), len(ca), ca, ca, True) if self_mode else pairs_two
    triples = _triples(rng, len(ca), len(ca) if self_mode else len(cb), self_mode)
    params = dict(seed=int(seed), profile=profile, reduced=reduced, self_mode=self_mode, content=content, tol=tol, check_words=check_words(t),
                  min_run=min_run, skip=skip_modes, zero_density=round(density, 3), variant_mask=bin(mask), rate=rate, max_stretches=max_stretches,
                  guard=guard, a_counts=list(ca), b_counts=list(cb), n_pairs_listed=len(pairs), n_triples_listed=len(triples), anchor=anchor,
                  plants=plants)
    return FuzzProblem(p, two, a_zero, b_zero, mask, rate, max_stretches, guard, pairs, pairs_two, triples, params)


def describe(seed: int, profile: str, reduced: bool = False) -> str:
    """what problem(seed, profile) drew, one parameter per line - with a failing (profile, seed) a complete report.  Printed and returned."""
    q = problem(seed, profile, reduced).params
    plants = q.pop("plants")
    lines = [f"alignfuzz.problem(seed={seed}, profile={profile!r}{', reduced=True' if reduced else ''})"]
    lines += [f"  {k} = {v}" for k, v in q.items()]
    lines += [f"  {len(plants)} planted runs (a, b, ka, kb, n, placement of the changed bits, share of windows on the tolerance):"]
    lines += [f"    {r}" for r in plants[:40]] + (["    ..."] if len(plants) > 40 else [])
    text = "\n".join(lines)
    print(text)
    return text


# ---- keyword arguments of the calls (host forms and Engine's host-array forms share them) -------------------------------------------------------------
def plain_args(p: aligngen.Problem) -> dict:
    return dict(a_hashes=p.a_hashes, a_first=p.a_first, b_hashes=p.b_hashes, b_first=p.b_first, tol_int=p.tol, min_run=p.min_run, a_skip=p.a_skip,
                b_skip=p.b_skip)


def variant_args(fp: FuzzProblem) -> dict:
    """without variant_mask: the list call takes none"""
    kw = plain_args(fp.p)
    kw.update(a_zero=fp.a_zero, b_zero=None if fp.self_mode else fp.b_zero)
    return kw


# ---- the calls: one table for the _host forms, Engine's host-array forms and its _device forms ------------------------------------------------------
ALIGN_FIELDS = ("a", "b", "offset", "start_a", "n_windows", "dist_sum")
STRETCH_FIELDS = ALIGN_FIELDS + ("rank",)
VARIANT_FIELDS = ("variant",) + ALIGN_FIELDS
PAIR_FIELDS = ("a", "b")
TRIPLE_FIELDS = ("variant", "a", "b")
RETIMED_FIELDS = ("a", "b", "first_a", "first_b", "n_windows", "dist_sum")


class Call(NamedTuple):
    entry: str          # how a failure names it: the function and, for the list forms, which list
    name: str           # Engine.<name>, Engine.<name>_device, <library>.<name>_host
    kw: dict            # host-array keyword arguments (no capacity)
    fields: tuple       # the record's fields in the twins' order


def table(rec, fields) -> np.ndarray:
    """a structured array of the library's, or a twin's list of tuples in `fields` order -> [n, len(fields)] int64"""
    if isinstance(rec, np.ndarray) and rec.dtype.names:
        return np.stack([rec[k].astype(np.int64) for k in fields], axis=1).reshape(-1, len(fields))
    return np.array(list(rec), np.int64).reshape(-1, len(fields))


def calls(fp: FuzzProblem) -> list:
    """the calls that take no list"""
    plain, var = plain_args(fp.p), variant_args(fp)
    return [Call("align_windows", "align_windows", plain, ALIGN_FIELDS),
            Call("align_windows_stretches", "align_windows_stretches", dict(plain, max_stretches=fp.max_stretches, guard=fp.guard), STRETCH_FIELDS),
            Call("align_seed_pairs", "align_seed_pairs", plain, PAIR_FIELDS),
            Call("align_windows_variants", "align_windows_variants", dict(var, variant_mask=fp.mask), VARIANT_FIELDS),
            Call("align_seed_pairs_variants", "align_seed_pairs_variants", dict(var, variant_mask=fp.mask), TRIPLE_FIELDS),
            Call("align_windows_retimed", "align_windows_retimed", dict(plain_args(fp.two), rate=fp.rate), RETIMED_FIELDS),
            Call("align_windows_retimed_pairs[sublist]", "align_windows_retimed_pairs", dict(plain_args(fp.two), rate=fp.rate, pairs=fp.pairs_two), RETIMED_FIELDS)]


def list_calls(fp: FuzzProblem, seed_pairs: np.ndarray, seed_triples: np.ndarray) -> list:
    """the calls on a list: on the seed calls' own output ([n, 2] pairs, [n, 3] (variant, a, b)) and on the drawn sublists"""
    plain, var = plain_args(fp.p), variant_args(fp)
    out = []
    for which, pairs, triples in (("seeds", seed_pairs, seed_triples), ("sublist", fp.pairs, fp.triples)):
        out += [Call(f"align_windows_pairs[{which}]", "align_windows_pairs", dict(plain, pairs=pairs), ALIGN_FIELDS),
                Call(f"align_windows_stretches_pairs[{which}]", "align_windows_stretches_pairs",
                     dict(plain, pairs=pairs, max_stretches=fp.max_stretches, guard=fp.guard), STRETCH_FIELDS),
                Call(f"align_windows_variants_pairs[{which}]", "align_windows_variants_pairs", dict(var, triples=triples), VARIANT_FIELDS)]
    return out


def host_form(vdf, call: Call, capacity: int):
    """the library's plain C++ definition of a call (vdf: the imported package) -> (table, found)"""
    rec, found = getattr(vdf, call.name + "_host")(capacity=capacity, **call.kw)
    return table(rec, call.fields), found


def first_difference(got: np.ndarray, want: np.ndarray, fields) -> str:
    """'' if the tables are equal, else the first row that differs, named field by field"""
    if got.shape == want.shape and np.array_equal(got, want):
        return ""
    n = min(len(got), len(want))
    rows = np.flatnonzero((got[:n] != want[:n]).any(axis=1))
    i = int(rows[0]) if len(rows) else n
    show = lambda t: dict(zip(fields, t[i].tolist())) if i < len(t) else "nothing"
    return f"{len(got)} records for {len(want)}; record {i}: got {show(got)}, want {show(want)}"
