"""Seeded random problems for the rate-list align entry points (vdf_align_seed_pairs_rates*, vdf_align_windows_rates*,
vdf_align_windows_rates_stretches*) AT THE SIZES WHERE THEIR KERNELS' STRUCTURE IS EXERCISED - what the hand-built cases of
seedrategen, ratealigngen and ratestretchgen aim at one situation at a time, and what their own random problems (at most 6 x 6 videos, 288 triples,
a bitmap of 13 words) are too small for.  Shared by tests/test_align_fuzz_rates_host.py (the _host definitions against the numpy twins, and the
conditions that keep this generator from being vacuous) and tests/test_gpu_zz_align_fuzz_rates.py (every device and host-array form against the
_host definitions).  numpy, alignfuzz, seedrategen, ratealigngen, ratestretchgen: nothing is imported from the library, and its constants are
WRITTEN DOWN (alignfuzz has them; the rate-list family's own are below).

problem(seed, profile) is deterministic from np.random.default_rng([FUZZ, seed]) (its child stream number PROFILES.index(profile)).  A problem is a
seedrategen.Problem: A rate-major, one block per rate, the window counts of a video DIFFERENT PER RATE as in ratealigngen.layout (but see
dup_equal), every block a_base rows into its rows and B b_base rows into its array.  The rates: 2 - 8 of RATE_POOL without repeats, in shuffled
order - shared dens (1/1 with 2/1, 5/4 with 7/4: one class of rows, two slots of the bitmap), the un-reduced duplicate 6/4 of 3/2, the large
numerators 31/16 and 32/17 (31 and 32 phases, most of them empty in a short video) - and always BOTH rates of one of the three two-slot classes:
a list drawn without one gets it added, so no problem has one rate (the GPU file runs a one-rate job per problem on its own).  With 3/2 and 6/4
both listed, every second problem makes the block of 6/4 a copy of the block of 3/2 (dup_equal: counts, hashes, skip bytes): two slots whose
records must be equal up to the rate index.  The profiles, and the constant each size comes from:

  bands      2 - 5 videos per side, 4 - 8 rates (kAlignWaves = 4, align_plan.h: the four waves of a workgroup serve units of different slots).  A
             TARGET rate with 2 <= num <= 7 is drawn and the window counts are built from SUB-MATRIX sizes - video a has rows x num windows (give
             or take less than num), video b cols x den - with rows and cols from {0, 1, 2, 63, 64, 65, 127, 128, 129} and uniform 1 ... 65: the
             edges of kAlignBand = 64 in the sub-matrix (ceil((Na - phase) / num) x ceil(Nb / den) cells), not in the video.  One video per side is
             long, rows + cols >= 130: three to five bands of 64 diagonals in every phase (more at the other rates), reloads and lane wraps inside a band (align_row_lane), masked
             rectangles across band boundaries.  Videos of 1 or 2 sub-rows are shorter than num: empty phases.  Empty videos.
  tiles      B: 1040 - 1480 windows in videos of 0 - 129: the class of den 2 (3/2 and 6/4, always listed) gathers more than kSeedTileRows = 512
             rows - two tiles - a class of den 1, where listed, three; the class of den 4 (5/4 or 7/4, one always listed) fewer than 384 - one
             tile whose wave 3 (rows 384 ... 511, 64 x kSeedRowsPerLane = 128 rows per wave) or waves 2 - 3 are padding only: the early return on a
             sentinel beside live waves.  No video of B begins on a tile edge of any listed class.  A: the two slots of the den-2 class hold more
             than kSeedChunk = 256 seeds together and the first of them fewer: chunk 0 spans the slot boundary, and there is a second chunk.
             min_run 1 or 2.  One exact copy nobody skips is planted from a seed behind chunk 0 into a video of B that lies wholly behind tile 0 of
             the den-2 class (alignfuzz._tile_anchor's idea on gathered rows): that triple's only hits lie behind tile 0.
  many_tiny  60 - 130 videos per side of 0 - 4 windows, 4 - 8 rates: 14 000 - 135 000 triples - several 256-item blocks (REDUCE_BLOCK) of
             align_reduce_rates_kernel, align_scan_kernel and align_scatter_kernel, compacted triple lists of the stretch rounds that cross a block,
             a capacity cut behind block 0 - and a rate-slotted bitmap of 450 - 4 300 words, past the 256 words of one count / scatter block, with
             n_a n_b no multiple of 32: every slot boundary falls inside a word.  Pool and static content are DENSE: most triples have a record.

reduced=True: sizes the numpy twins can walk - at most 3 rates; bands: at most 3 videos per side, the sub-matrix edges at 64 and 128 kept under
target 2/1 or 3/2; tiles: rates 1/1, 2/1 and one of den 4, B 520 - 600 windows (the 512-row edge in the class of den 1, a padded single tile in
the class of den 4), the two slots of den 1 just over 256 seeds; many_tiny: 60 - 95 videos per side.

The content is alignfuzz's three kinds - `pool` (every window of every block and of B out of 4 - 8 related hashes, some exactly on the tolerance:
dense matches, ties, runs on all edges), `planted` (a random background and lines along each rate's slope, placed by ratealigngen.plant: lengths
above 64 sub-rows, lines that end on the last row or column, flips of tol - 3 ... tol + 3 bits placed in the last eight dwords, the first fourteen
or anywhere - what the four early-exit instantiations 14 / 22 / 26 / 32 of align_seed_rates_kernel must and may drop), `static` (one hash all over
part of the videos, most of those windows skipped).  The tolerance is drawn from alignfuzz.TOLERANCES - the six values beside the early-exit edges
179 | 180, 297 | 298, 357 | 358 twice as often as the others - min_run from alignfuzz.MIN_RUNS (a value no sub-matrix can reach is mostly drawn
again), the skip arrays as alignfuzz draws them (absent, 5 - 15 %, 60 %), max_stretches and guard from alignfuzz's lists (many_tiny: mostly guard 0 or 1 - five rows mask a whole matrix of 4 x 4 windows).  exclude_same is drawn
where n_a = n_b (every third problem is square), and lines are planted in triples (r, v, v) there.  Every plant reads A and writes B, in a
shuffled order; B is shared by the rates, so a later line trims an earlier one.  Nothing here is an error by include/vdf.h."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import alignfuzz as fz
import hashgen
import ratealigngen as gen
import ratestretchgen as sg
from alignfuzz import Call, first_difference, table  # noqa: F401  (part of this module's interface)
from seedrategen import Problem, reduced as lowest

FUZZ = 4172                      # the file's constant: problem(seed, ...) draws from default_rng([FUZZ, seed])
PROFILES = fz.PROFILES

# ---- the library's constants, written down, where alignfuzz does not have them ---------------------------------------------------------------------
SEED_WAVE_ROWS = 128             # align.hip align_seed_rates_kernel: 64 lanes x kSeedRowsPerLane = 2 rows of a tile per wave, 4 waves per tile of 512
RATES_MAX = 8                    # align_seed_rates_plan.h kSeedRatesMax = VDF_WINDOWS_MAX_RATES: slots of the bitmap

RATE_POOL = ((1, 1), (2, 1), (5, 4), (7, 4), (3, 2), (6, 4), (31, 16), (32, 17))
CLASS_PAIRS = (((1, 1), (2, 1)), ((5, 4), (7, 4)), ((3, 2), (6, 4)))    # two slots, one class: equal dens in lowest terms
BAND_TARGETS = ((2, 1), (5, 4), (7, 4), (3, 2), (6, 4))                    # 2 <= num <= 7 in lowest terms
BAND_SUBS = (0, 1, 2, 63, 64, 65, 127, 128, 129)
EDGE_TOLERANCES = (179, 180, 297, 298, 357, 358)

TRIPLE_FIELDS = ("a", "b", "rate")      # the twins' orders: seedrategen.seed_rates_twin, ratealigngen.FIELDS, ratestretchgen.FIELDS
RATE_FIELDS = gen.FIELDS
RATE_STRETCH_FIELDS = sg.FIELDS
RETIMED_FIELDS = fz.RETIMED_FIELDS


class RateFuzzProblem(NamedTuple):
    p: Problem                      # seedrategen.Problem, exclude_same in it
    max_stretches: int
    guard: int
    triples: np.ndarray             # [n, 3] (rate, a, b): a strictly increasing sublist of all triples, triples of empty videos among them
    params: dict                    # what was drawn, for describe()

    @property
    def exclude_same(self) -> bool:
        return self.p.exclude_same


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------------------
def _pair_of(rate):
    return next((pair for pair in CLASS_PAIRS if rate in pair), None)


def counts_a(p: Problem, r: int) -> np.ndarray:
    return np.diff(p.a_first[r].astype(np.int64))


def counts_b(p: Problem) -> np.ndarray:
    return np.diff(p.b_first.astype(np.int64))


def sub_rows(na: int, num: int, phase: int = 0) -> int:
    return -(-(int(na) - phase) // num) if na > phase else 0


def sub_cols(nb: int, den: int) -> int:
    return -(-int(nb) // den)


def n_bands(rows: int, cols: int) -> int:
    """align_plan.h: the bands of a rows x cols matrix - its rows + cols - 1 diagonals in groups of kAlignBand"""
    return 0 if not rows or not cols else -(-(rows + cols - 1) // fz.ALIGN_BAND)


def classes(rates) -> list:
    """align_seed_rates_plan.h: [(den, [slots])] in the order of the first slot of each den (lowest terms)"""
    out = {}
    for slot, rate in enumerate(rates):
        out.setdefault(lowest(rate)[1], []).append(slot)
    return list(out.items())


def class_rows(cb, den: int) -> list:
    """the rows a class gathers: [(b, kb)] - kb = 0, den, 2 den ... of every video of B"""
    return [(b, kb) for b in range(len(cb)) for kb in range(0, int(cb[b]), den)]


def class_seeds(p: Problem, slots) -> list:
    """the seeds of a class in the plan's order: [(slot, a, ka)] by (slot, video, ka), ka a seed iff (ka // num) % min_run == 0"""
    out = []
    for slot in slots:
        num = lowest(p.rates[slot])[0]
        for a, n in enumerate(counts_a(p, slot).tolist()):
            out += [(slot, a, ka) for ka in range(n) if (ka // num) % p.min_run == 0]
    return out


def n_seeds(counts, num: int, min_run: int) -> int:
    return int(sum(np.count_nonzero((np.arange(int(c)) // num) % min_run == 0) for c in counts))


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------------------
def _draw_rates(rng, n: int, must) -> tuple:
    """`must`, both rates of a two-slot class (the one a rate of `must` belongs to, else a drawn one), and others of the pool up to n: shuffled"""
    rates = list(must)
    pair = next((q for q in map(_pair_of, rates) if q is not None), None) or CLASS_PAIRS[int(rng.integers(0, len(CLASS_PAIRS)))]
    rates += [r for r in pair if r not in rates]
    rest = [r for r in RATE_POOL if r not in rates]
    rates += [rest[int(i)] for i in rng.permutation(len(rest))[:max(0, n - len(rates))]]
    return tuple(rates[int(i)] for i in rng.permutation(len(rates)))


def _band_shapes(rng, reduced: bool, square: bool):
    """-> (sub-rows of A's videos, sub-columns of B's) under the target rate; square: as many videos of B as of A"""
    top = 3 if reduced else 5
    subs = BAND_SUBS[:6] if reduced else BAND_SUBS
    draw = lambda: int(rng.choice(subs)) if rng.random() < 0.5 else int(rng.integers(1, 41 if reduced else 66))
    n_rows, n_cols = int(rng.integers(2, top + 1)), int(rng.integers(2, top + 1))
    rows, cols = [draw() for _ in range(n_rows)], [draw() for _ in range(n_rows if square else n_cols)]
    i, j = int(rng.integers(0, len(rows))), int(rng.integers(0, len(cols)))
    if reduced:   # the edges at 64 and 128 stay: 64 or so against 64 or so (two bands), sometimes 128 against a few
        rows[i], cols[j] = (int(rng.choice((127, 128, 129))), int(rng.integers(1, 6))) if rng.random() < 0.3 else (int(rng.choice((63, 64, 65))), int(rng.choice((63, 64, 65))))
    else:         # rows + cols >= 130: at least three bands in phase 0
        rows[i] = int(rng.choice((127, 128, 129))) if rng.random() < 0.6 else int(rng.integers(66, 130))
        cols[j] = max(int(rng.choice((63, 64, 65, 127, 128, 129))), 130 - rows[i])
    return rows, cols


def _windows_of(rng, subs, stride: int) -> list:
    """videos of `subs` sub-rows under a stride: stride (s - 1) + 1 ... stride s windows"""
    return [0 if s == 0 else stride * (s - 1) + 1 + int(rng.integers(0, stride)) for s in subs]


def _per_rate(rng, base, rates, fixed=()) -> list:
    """the window counts of A's videos per rate: `base` at the rates of `fixed`, up to two more or fewer windows at the others (a video without
    windows keeps none at any rate)"""
    out = []
    for rate in rates:
        if rate in fixed:
            out.append([int(c) for c in base])
        else:
            out.append([0 if c == 0 else max(0, int(c) + int(rng.integers(-2, 3))) for c in base])
    return out


def _rows_behind(cb, den: int, n: int, whole: bool) -> list:
    """[(b, j0)]: n gathered rows j0 ... of video b that lie behind tile 0 of the class of `den`; whole: only in videos that begin behind it"""
    first = np.concatenate([[0], np.cumsum([sub_cols(c, den) for c in cb])])
    return [(b, j0) for b in range(len(cb)) for j0 in range(sub_cols(cb[b], den) - n + 1)
            if first[b] + j0 >= fz.SEED_TILE_ROWS and (not whole or first[b] >= fz.SEED_TILE_ROWS)]


def _tile_b(rng, lo: int, hi: int, dens, two_tiles: int, padded: int, whole: bool) -> list:
    """videos of 0 ... 129 windows, lo ... hi in all: the class of den `two_tiles` gathers more than 512 rows and has three rows of one video behind
    them (whole: of a video that begins behind them), the class of den `padded` at most 384 (its last wave is padding), and no video begins on a
    tile edge of any class of `dens`"""
    for _ in range(2000):
        total = int(rng.integers(lo, hi + 1))
        out = []
        while sum(out) < total:
            kind = rng.random()
            out.append(min(0 if kind < 0.08 else int(rng.integers(1, 8)) if kind < 0.2 else int(rng.integers(20, 130)), total - sum(out)))
        ok = bool(_rows_behind(out, two_tiles, 3, whole)) and len(class_rows(out, padded)) <= fz.SEED_TILE_ROWS - SEED_WAVE_ROWS
        for den in dens:
            first = np.cumsum([sub_cols(c, den) for c in out])[:-1]
            ok = ok and len(class_rows(out, den)) % fz.SEED_TILE_ROWS != 0 and not np.any((first % fz.SEED_TILE_ROWS == 0) & (first > 0))
        if ok:
            return out + [0] * int(rng.integers(0, 2))
    raise AssertionError("no tile shape found")


def _tile_a(rng, num: int, min_run: int) -> list:
    """3 - 7 videos whose seeds under num number 140 - 250: a slot of fewer than 256 seeds, two such slots more"""
    for _ in range(2000):
        out = [int(rng.integers(0, 3)) if rng.random() < 0.15 else int(rng.integers(10, 60 * min_run + 40)) for _ in range(int(rng.integers(3, 8)))]
        if 140 <= n_seeds(out, num, min_run) <= 250:
            return out
    raise AssertionError("no seed shape found")


def _tiny(rng, reduced: bool, square: bool):
    n_a, n_b = (int(rng.integers(60, 96 if reduced else 131)) for _ in range(2))
    n_b |= 1                    # n_a n_b is a multiple of 32 only if n_a is
    if square:
        n_a = n_b
    elif n_a % 32 == 0:
        n_a += 1
    return [int(c) for c in rng.integers(0, 5, size=n_a)], [int(c) for c in rng.integers(0, 5, size=n_b)]


# ---- content ----------------------------------------------------------------------------------------------------------------------------------------
def _row_a(p: Problem, r: int, a: int, ka: int) -> int:
    return int(p.a_rate_first[r]) + int(p.a_first[r, a]) + ka


def _plant_line(rng, p: Problem, r: int, a: int, b: int, t: int, log: list, exact: bool = False):
    """one line of the slope of rates[r] in triple (r, a, b), cells placed by ratealigngen.plant and then changed as alignfuzz._plant_runs changes
    them: a length (often above 64 where the sub-matrix allows it), a position (often against its last row or column), a placement of the changed
    bits and the share of cells within 3 bits of the tolerance (the others 0 ... 40 bits off, at most the tolerance)"""
    num, den = lowest(p.rates[r])
    na, nb = int(counts_a(p, r)[a]), int(counts_b(p)[b])
    if na == 0 or nb == 0:
        return
    phase = int(rng.integers(0, min(num, na)))
    rows, cols = sub_rows(na, num, phase), sub_cols(nb, den)
    top = min(rows, cols)
    kind = rng.random()
    n = int(rng.integers(min(65, top), top + 1)) if kind < 0.3 else int(rng.integers(1, min(top, 12) + 1)) if kind < 0.5 else int(rng.integers(1, top + 1))
    i0, j0 = int(rng.integers(0, rows - n + 1)), int(rng.integers(0, cols - n + 1))
    where = rng.random()
    if where < 0.15:
        i0 = rows - n        # ends on the last row
    elif where < 0.3:
        j0 = cols - n        # ends on the last column
    elif where < 0.4:
        i0, j0 = (0, j0) if rng.random() < 0.5 else (i0, 0)
    gen.plant(rng, p, r, a, b, phase, i0, j0, n, 0)
    place = str(rng.choice(list(fz._PLACEMENTS)))
    edge_share = 0.0 if exact else float(rng.choice([1.0, 0.3, 0.03], p=[0.15, 0.25, 0.6]))
    if not exact:
        for m in range(n):
            k = fz._edge_flips(rng, t) if rng.random() < edge_share else int(rng.integers(0, min(t, 40) + 1))
            row = int(p.b_first[b]) + den * (j0 + m)
            p.b_hashes[row] = fz._flip(p.b_hashes[row], k, rng, fz._PLACEMENTS[place])
    log.append((r, a, b, phase, i0, j0, n, place, edge_share))


def _related(rng, profile: str, n_rates: int, n_a: int, n_b: int, square: bool) -> list:
    if profile == "bands":
        share = min(0.6, 1.5 / n_rates)   # B is shared by the rates: more lines would leave no line whole
        out = [(r, a, b) for r in range(n_rates) for a in range(n_a) for b in range(n_b) if rng.random() < share]
    else:
        n = int(rng.integers(30, 51)) if profile == "tiles" else int(rng.integers(2 * n_a, 4 * n_a + 1))
        out = [(int(rng.integers(0, n_rates)), int(rng.integers(0, n_a)), int(rng.integers(0, n_b))) for _ in range(n)]
    if square:   # exclude_same needs triples that name one video twice
        out += [(int(rng.integers(0, n_rates)), v, v) for v in rng.integers(0, n_a, size=max(2, n_a // 8)).tolist()]
    return out


def _sublist(rng, p: Problem) -> np.ndarray:
    """about 40 % of all (rate, a, b) in order - 80 % of those that name a video without windows at that rate"""
    n_a, n_b = p.a_first.shape[1] - 1, len(p.b_first) - 1
    out = []
    for r in range(len(p.rates)):
        a, b = (x.reshape(-1) for x in np.meshgrid(np.arange(n_a), np.arange(n_b), indexing="ij"))
        empty = (counts_a(p, r)[a] == 0) | (counts_b(p)[b] == 0)
        take = rng.random(len(a)) < np.where(empty, 0.8, 0.4)
        out.append(np.stack([np.full(int(take.sum()), r), a[take], b[take]], axis=1))
    return np.concatenate(out).astype(np.int64)


def _tile_anchor(rng, p: Problem, slots, den: int, twin_slots, whole: bool):
    """an exact copy of min_run + 1 cells nobody skips, from a seed of the class `slots` behind its chunk 0 into rows of B that the class gathers
    behind its tile 0 - whole: in a video that begins behind it, so that the triple has no hit in tile 0.  -> (slot, a, ka, b, kb) or None"""
    n = p.min_run + 1
    behind = _rows_behind(counts_b(p), den, n, whole)
    nums = {slot: lowest(p.rates[slot])[0] for slot in slots}
    cand = [(slot, a, ka) for slot, a, ka in class_seeds(p, slots)[fz.SEED_CHUNK:]
            if sub_rows(counts_a(p, slot)[a], nums[slot], ka % nums[slot]) - ka // nums[slot] >= n]
    if not behind or not cand:
        return None
    slot, a, ka = cand[int(rng.integers(0, len(cand)))]
    b, j0 = behind[int(rng.integers(0, len(behind)))]
    num = nums[slot]
    gen.plant(rng, p, slot, a, b, ka % num, ka // num, j0, n, 0)
    for m in range(n):
        for s in {slot} | set(twin_slots if slot in twin_slots else ()):   # equal blocks stay equal
            if p.a_skip is not None:
                p.a_skip[_row_a(p, s, a, ka + num * m)] = 0
        if p.b_skip is not None:
            p.b_skip[int(p.b_first[b]) + den * (j0 + m)] = 0
    return slot, a, ka, b, den * j0


# ---- the generator ----------------------------------------------------------------------------------------------------------------------------------
def problem(seed: int, profile: str, reduced: bool = False) -> RateFuzzProblem:
    # one child stream per profile: seed s of one profile shares no draw with seed s of another
    rng = np.random.default_rng([FUZZ, int(seed)]).spawn(len(PROFILES))[PROFILES.index(profile)]
    content = str(rng.choice(fz.CONTENTS, p=[0.4, 0.4, 0.2]))
    weights = np.array([2.0 if x in EDGE_TOLERANCES else 1.0 for x in fz.TOLERANCES])
    tol = int(rng.choice(fz.TOLERANCES, p=weights / weights.sum()))
    t = min(tol, 1024)
    min_run = int(rng.choice(fz.MIN_RUNS))
    skip_modes = [str(rng.choice(["absent", "sparse", "dense"], p=[0.4, 0.4, 0.2])) for _ in range(2)]
    max_stretches = int(rng.choice(fz.MAX_STRETCHES, p=[0.1, 0.15, 0.35, 0.4]))
    # many_tiny: a guard of 5 rows masks a whole matrix of 4 x 4 windows and ends the rounds - mostly the small ones there
    guard = int(rng.choice(fz.GUARDS, p=[0.5, 0.35, 0.1, 0.05] if profile == "many_tiny" else [0.35, 0.3, 0.25, 0.1]))
    square = bool(rng.random() < 1 / 3)
    a_base, b_base = int(rng.integers(0, 7)), int(rng.integers(0, 7))
    target = None

    # the rates and the shapes
    if profile == "bands":
        target = (BAND_TARGETS[:1] + BAND_TARGETS[3:] if reduced else BAND_TARGETS)[int(rng.integers(0, 3 if reduced else len(BAND_TARGETS)))]
        rates = _draw_rates(rng, int(rng.integers(2, 4)) if reduced else int(rng.integers(4, RATES_MAX + 1)), [target])
        rows, cols = _band_shapes(rng, reduced, square)
        num, den = lowest(target)
        ca = _per_rate(rng, _windows_of(rng, rows, num), rates, fixed=(target,))
        cb = _windows_of(rng, cols, den)
    elif profile == "tiles":
        min_run = int(rng.choice([1, 2]))
        den4 = ((5, 4), (7, 4))[int(rng.integers(0, 2))]
        wide = CLASS_PAIRS[0] if reduced else CLASS_PAIRS[2]        # the two slots whose class has two tiles and more than a chunk of seeds
        rates = _draw_rates(rng, 3 if reduced else int(rng.integers(3, 7)), list(wide) + [den4])
        dens = sorted({lowest(r)[1] for r in rates})
        cb = _tile_b(rng, *((520, 600) if reduced else (1040, 1480)), dens, lowest(wide[0])[1], 4, not reduced)
        base = _tile_a(rng, max(lowest(r)[0] for r in wide), min_run)
        ca = _per_rate(rng, base, rates, fixed=wide)
        square = False
    else:
        assert profile == "many_tiny", profile
        rates = _draw_rates(rng, int(rng.integers(2, 4)) if reduced else int(rng.integers(4, RATES_MAX + 1)), [])
        base, cb = _tiny(rng, reduced, square)
        ca = [[int(np.clip(c + rng.integers(-1, 2), 0, 4)) if rng.random() < 0.3 else c for c in base] for _ in rates]
    exclude_same = bool(square and rng.random() < 0.6)
    dup = [rates.index(r) for r in CLASS_PAIRS[2]] if all(r in rates for r in CLASS_PAIRS[2]) else None
    dup_equal = bool(dup is not None and rng.random() < 0.5)
    if dup_equal:
        ca[dup[1]] = list(ca[dup[0]])
    # the longest diagonal of a sub-matrix - in bands under the target rate, whose sub-matrices the shapes were drawn for
    longest = max(min(sub_rows(max(ca[r]), lowest(rate)[0]), sub_cols(max(cb), lowest(rate)[1])) for r, rate in enumerate(rates) if target in (None, rate))
    if 3 * min_run > longest and rng.random() < 0.85:
        # a min_run that no sub-matrix or hardly one can reach silences every call: mostly one of the list up to a third of the longest (many_tiny: 1)
        min_run = int(rng.choice([m for m in fz.MIN_RUNS if m <= max(longest // 3, 1)]))

    p = gen.layout(rng, rates, ca, cb, a_base, b_base, tol=tol, min_run=min_run)
    n_a, n_b = len(ca[0]), len(cb)

    def block(r):
        return slice(int(p.a_rate_first[r]), int(p.a_rate_first[r + 1]))

    # content.  Every plant READS windows of A and WRITES windows of B, in a shuffled order: a later one trims an earlier one
    plants: list = []
    todo: list = []
    static_a = static_b = None
    if content == "pool":
        pool = fz._pool(rng, t)
        p.a_hashes[:] = pool[rng.integers(0, len(pool), size=len(p.a_hashes))]
        p.b_hashes[:] = pool[rng.integers(0, len(pool), size=len(p.b_hashes))]
        related = _related(rng, profile, len(rates), n_a, n_b, square)[:12]
        exact = True
    else:
        if content == "static":
            s = hashgen.random_hashes(rng, 1)[0]
            static_a, static_b = rng.random(n_a) < rng.uniform(0.3, 0.6), rng.random(n_b) < rng.uniform(0.3, 0.6)
            for r in range(len(rates)):
                for v in np.flatnonzero(static_a):
                    p.a_hashes[_row_a(p, r, v, 0):_row_a(p, r, v + 1, 0)] = s
            for v in np.flatnonzero(static_b):
                p.b_hashes[int(p.b_first[v]):int(p.b_first[v + 1])] = s
            skip_modes = ["sparse" if m == "absent" else m for m in skip_modes]
        related = _related(rng, profile, len(rates), n_a, n_b, square)
        exact = False
    if dup_equal:
        p.a_hashes[block(dup[1])] = p.a_hashes[block(dup[0])]
    for r, a, b in related:
        for _ in range(1 if exact else int(rng.integers(1, 4))):
            todo.append(lambda r=r, a=a, b=b: _plant_line(rng, p, r, a, b, t, plants, exact))
    for i in rng.permutation(len(todo)).tolist():
        todo[i]()
    a_skip, b_skip = fz._skip(rng, skip_modes[0], len(p.a_hashes)), fz._skip(rng, skip_modes[1], len(p.b_hashes))
    if content == "static":  # most of the static windows abstain: all but one stretch of at most a quarter of the video
        spans = [(_row_a(p, r, v, 0), _row_a(p, r, v + 1, 0), a_skip) for r in range(len(rates)) for v in np.flatnonzero(static_a)]
        spans += [(int(p.b_first[v]), int(p.b_first[v + 1]), b_skip) for v in np.flatnonzero(static_b)]
        for lo, hi, sk in spans:
            keep = int(rng.integers(0, (hi - lo) // 4 + 1))
            at = lo + int(rng.integers(0, hi - lo - keep + 1))
            kept = sk[at:at + keep].copy()
            sk[lo:hi] = rng.integers(1, 256, size=hi - lo)
            sk[at:at + keep] = kept
    if dup_equal and a_skip is not None:
        a_skip[block(dup[1])] = a_skip[block(dup[0])]
    p = p._replace(a_skip=a_skip, b_skip=b_skip, exclude_same=exclude_same)
    anchor = None
    if profile == "tiles":
        wide_slots = [rates.index(r) for r in wide]
        anchor = _tile_anchor(rng, p, sorted(wide_slots), lowest(wide[0])[1], dup if dup_equal else (), not reduced)
        assert anchor is not None, "tiles: no seed behind the first chunk or no video behind the first tile"
    triples = _sublist(rng, p)
    params = dict(seed=int(seed), profile=profile, reduced=reduced, content=content, tol=tol, check_words=fz.check_words(t), min_run=min_run, skip=skip_modes,
                  rates=rates, target=target, classes=classes(rates), dup_equal=dup_equal, exclude_same=exclude_same, max_stretches=max_stretches, guard=guard,
                  a_base=a_base, b_base=b_base, a_counts=[list(c) for c in ca] if profile != "many_tiny" else f"{n_a} videos of 0 - 4 windows",
                  b_counts=list(cb) if profile != "many_tiny" else f"{n_b} videos of 0 - 4 windows", n_triples=len(rates) * n_a * n_b,
                  n_triples_listed=len(triples), bitmap_words=-(-len(rates) * n_a * n_b // 32), anchor=anchor, plants=plants)
    return RateFuzzProblem(p, max_stretches, guard, triples, params)


def describe(seed: int, profile: str, reduced: bool = False) -> str:
    """what problem(seed, profile) drew, one parameter per line - with a failing (profile, seed) a complete report.  Printed and returned."""
    q = dict(problem(seed, profile, reduced).params)
    plants = q.pop("plants")
    lines = [f"ratefuzz.problem(seed={seed}, profile={profile!r}{', reduced=True' if reduced else ''})"]
    lines += [f"  {k} = {v}" for k, v in q.items()]
    lines += [f"  {len(plants)} planted lines (rate, a, b, phase, i0, j0, n, placement of the changed bits, share of cells on the tolerance):"]
    lines += [f"    {r}" for r in plants[:40]] + (["    ..."] if len(plants) > 40 else [])
    text = "\n".join(lines)
    print(text)
    return text


# ---- the calls: one table for the _host forms, Engine's host-array forms and its _device forms ---------------------------------------------------------
def rate_args(p: Problem, exclude_same=None) -> dict:
    """the host-array keyword arguments every call of the family takes"""
    return dict(a_hashes=p.a_hashes, a_first=p.a_first, b_hashes=p.b_hashes, b_first=p.b_first, rates=p.rates, tol_int=p.tol, min_run=p.min_run,
                a_rate_first=p.a_rate_first, a_skip=p.a_skip, b_skip=p.b_skip, exclude_same=p.exclude_same if exclude_same is None else exclude_same)


def calls(fp: RateFuzzProblem) -> list:
    """the calls that take no list: the seed call, and the align and the stretches call over every triple and with seed = 1"""
    kw = rate_args(fp.p)
    st = dict(kw, max_stretches=fp.max_stretches, guard=fp.guard)
    return [Call("align_seed_pairs_rates", "align_seed_pairs_rates", kw, TRIPLE_FIELDS),
            Call("align_windows_rates", "align_windows_rates", kw, RATE_FIELDS),
            Call("align_windows_rates[seed=1]", "align_windows_rates", dict(kw, seed=True), RATE_FIELDS),
            Call("align_windows_rates_stretches", "align_windows_rates_stretches", st, RATE_STRETCH_FIELDS),
            Call("align_windows_rates_stretches[seed=1]", "align_windows_rates_stretches", dict(st, seed=True), RATE_STRETCH_FIELDS)]


def as_list(seed_table: np.ndarray) -> np.ndarray:
    """a table of the seed call's records (TRIPLE_FIELDS: a, b, rate) as the [n, 3] (rate, a, b) list the align calls take"""
    return np.ascontiguousarray(seed_table.reshape(-1, 3)[:, [2, 0, 1]])


def list_calls(fp: RateFuzzProblem, seed_triples: np.ndarray) -> list:
    """the calls on a list ([n, 3] (rate, a, b)): on the seed call's own output and on the drawn sublist.  A list goes without exclude_same (the
    library refuses the two together); the seed call's output has no self-named triple under it anyway"""
    kw = rate_args(fp.p, exclude_same=False)
    out = []
    for which, triples in (("seeds", seed_triples), ("sublist", fp.triples)):
        out += [Call(f"align_windows_rates[{which}]", "align_windows_rates", dict(kw, triples=triples), RATE_FIELDS),
                Call(f"align_windows_rates_stretches[{which}]", "align_windows_rates_stretches",
                     dict(kw, triples=triples, max_stretches=fp.max_stretches, guard=fp.guard), RATE_STRETCH_FIELDS)]
    return out


def one_rate(p: Problem, r: int) -> Problem:
    """block r as a problem of its own: one rate, exclude_same off - what align_windows_retimed answers at that rate"""
    lo, hi = int(p.a_rate_first[r]), int(p.a_rate_first[r + 1])
    return p._replace(a_hashes=p.a_hashes[lo:hi], a_first=p.a_first[r:r + 1], a_rate_first=np.array([0, hi - lo], np.int64), rates=(p.rates[r],),
                      a_skip=None if p.a_skip is None else p.a_skip[lo:hi], exclude_same=False)


def host_form(vdf, call: Call, capacity: int):
    """the library's plain C++ definition of a call (vdf: the imported package) -> (table, found)"""
    rec, found = getattr(vdf, call.name + "_host")(capacity=capacity, **call.kw)
    return table(rec, call.fields), found
