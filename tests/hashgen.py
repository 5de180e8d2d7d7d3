"""Synthetic hash fixtures: the build's own restatement of the reference's test utilities
(vid_dup_finder_lib/src/video_hashing/video_hash.rs:240-308 `test_util`, and the scenario builders of
vid_dup_finder_lib/tests/test_find_all.rs:14-132) with numpy's PCG64 instead of rand 0.9's StdRng.
Every assertion upstream is structural (group counts and sizes), so the construction - not the
random stream - is what has to match.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

HASH_WORDS = 16
HASH_BITS = 1000


def random_hash(rng: np.random.Generator) -> np.ndarray:
    """1000 fair bits, padding bits 1000..1023 zero (video_hash.rs:293-306)."""
    bits = rng.integers(0, 2, size=1024, dtype=np.uint8)
    bits[HASH_BITS:] = 0
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


def random_hashes(rng: np.random.Generator, n: int) -> np.ndarray:
    words = rng.integers(0, 2**64, size=(n, HASH_WORDS), dtype=np.uint64)
    words[:, 15] &= np.uint64((1 << 40) - 1)  # bits 960..999 live in word 15; 1000..1023 cleared
    return words


def hamming(a: np.ndarray, b: np.ndarray) -> int:
    return int(np.unpackbits((a ^ b).view(np.uint8)).sum())


def hash_with_spatial_distance(h: np.ndarray, target: int, rng: np.random.Generator) -> np.ndarray:
    """A hash at EXACTLY `target` bits from `h`, bits chosen anywhere in the 1024 (padding included).
    Upstream (video_hash.rs:272-291) random-walks single bit flips until the distance first reaches
    `target`; by symmetry the first-hit point is uniform on the sphere of that radius, which is what
    flipping `target` distinct random positions samples directly.  (The walk itself is hopeless in Python
    for radius 600 > the 512-bit equilibrium, which test_find_with_refs needs.)"""
    flips = rng.choice(1024, size=target, replace=False)
    bits = np.unpackbits(h.view(np.uint8), bitorder="little")
    bits[flips] ^= 1
    out = np.packbits(bits, bitorder="little").view(np.uint64).copy()
    assert hamming(h, out) == target
    return out


class HashesWithDistance:
    """test_find_all.rs:14-60"""

    def __init__(self, start_hash, distance, num_hashes, rng):
        self.start_hash = start_hash
        self.members_ = [hash_with_spatial_distance(start_hash, distance, rng) for _ in range(num_hashes)]
        self.distance = distance

    def members(self, rng):
        idx = rng.permutation(len(self.members_))
        return [self.members_[i] for i in idx]


class HashesWithDistanceSet:
    """test_find_all.rs:62-132"""

    def __init__(self, num_groups, hashes_per_group, intergroup_distance, intragroup_distance, rng):
        assert intragroup_distance * 2 < intergroup_distance
        assert (19 * 64) // num_groups > intergroup_distance
        start = random_hash(rng)
        self.groups = []
        cur = 0
        for _ in range(num_groups):
            g_start = hash_with_spatial_distance(start, cur, rng)
            cur += intergroup_distance
            self.groups.append(HashesWithDistance(g_start, intragroup_distance, hashes_per_group, rng))
            hashes_per_group += 10

    def all_members(self, rng):
        allm = [m for g in self.groups for m in g.members(rng)]
        idx = rng.permutation(len(allm))
        return [allm[i] for i in idx]


def planted_set(rng: np.random.Generator, n: int, n_clusters: int, max_copies: int = 4, max_flips: int = 350,
                durations: str = "zero"):
    """Random hashes with planted near-duplicates: some copies land exactly on or over
    the tolerance.  Returns (hashes [n,16] u64, durations [n] u32), unsorted."""
    words = random_hashes(rng, n)
    if durations == "zero":
        dur = np.zeros(n, np.uint32)
    else:
        dur = np.floor(np.exp(rng.uniform(np.log(5), np.log(7200), size=n))).astype(np.uint32)
    src = rng.choice(n, size=min(n_clusters, n), replace=False)
    free = np.setdiff1d(np.arange(n), src)
    rng.shuffle(free)
    pos = 0
    for s in src:
        for _ in range(int(rng.integers(1, max_copies + 1))):
            if pos >= len(free):
                break
            t = free[pos]
            pos += 1
            k = int(rng.integers(0, max_flips + 30))
            flips = rng.choice(1024, size=k, replace=False)
            bits = np.unpackbits(words[s].view(np.uint8), bitorder="little")
            bits[flips] ^= 1
            words[t] = np.packbits(bits, bitorder="little").view(np.uint64)
            if durations != "zero":
                jitter = rng.uniform(0.9, 1.12)
                dur[t] = np.uint32(max(0, int(dur[s] * jitter)))
    return words, dur


def sort_by_duration(words: np.ndarray, dur: np.ndarray):
    """Search::sort with all paths equal: stable by duration."""
    order = np.argsort(dur, kind="stable")
    return words[order], dur[order], order


# ---------------------------------------------------------------------------------------------------------------------
# Structured hashes for the search's prefix test (DESIGN.md 4.3 "Structured pair corpus").
#
# Both search backends rule a pair out after a PREFIX of the 32 packed dwords (u32 dword d = bits 32 d .. 32 d + 31 of the hash,
# little-endian inside the u64 words) and only evaluate the survivors over all 1024 bits.  Everything below is restated from
# the comments and launch tables of csrc/hamming.hip and csrc/api.cpp - nothing is imported from the library - so that a
# change on either side shows as a disagreement.

MFMA_STEPS = (6, 8, 10, 11, 12, 13, 14, 16)  # instantiated early-exit steps of hamming_mfma2_kernel (16 = no test: all 16 k-steps)
VALU_DWORDS = ((6, 14), (10, 22), (12, 26))  # hamming_tile_kernel<R, CHKW>: (largest step that takes it, CHKW); beyond: all 32

# (api.cpp search_core: tolerances up to the first number take the step next to it; the numbers are the largest tolerances that
# still leave unrelated hashes 4 sigma away after 64 (step + 1) bits.)  The GPU tests search on both sides of every change:
AUTO_STEP_EDGES = (180, 239, 297, 327, 357, 387, 417)
AUTO_TOLERANCES = tuple(t for e in AUTO_STEP_EDGES for t in (e, e + 1)) + (0, 1, 31, 120, 350, 448, 511, 512, 600, 1000, 1023, 1024, 5000)
FORCED_STEP_TOLERANCES = tuple((s, t) for s in (6, 8, 10, 11, 12) for t in (0, 120, 350)) + tuple((s, t) for s in (13, 14, 16) for t in (400, 600))


def auto_step(tol: int) -> int:
    """The early-exit step search_core derives from the tolerance: the first k-step st in 6..14 after which unrelated hashes
    (partial distance bits / 2 +- sqrt(bits) / 2 over bits = 64 (st + 1)) are still more than tol apart 4 sigma down; else 16."""
    for st in range(6, 15):
        bits = 64.0 * (st + 1)
        if bits / 2 - 2.0 * np.sqrt(bits) >= tol + 1:
            return st
    return 16


def instantiated_step(backend: str, step: int) -> int:
    """The step of the kernel instance that serves a requested step: the next instantiated one (16 = the full-length test)."""
    return next((s for s in (MFMA_STEPS if backend == "mfma" else (6, 10, 12)) if step <= s), 16)


def tested_dwords(backend: str, step: int):
    """Sorted dwords of the prefix the backend tests when asked for early-exit step `step` (any step: rounded up to the next
    instantiated one, as the launchers do).  Matrix cores: k-step s multiplies dwords s and 16 + s, the prefix is k-steps
    0..step.  VALU: the first 14, 22 or 26 dwords in linear order."""
    if backend == "mfma":
        inst = next((s for s in MFMA_STEPS if step <= s), 16)
        if inst >= 15:
            return tuple(range(32))
        return tuple(sorted([s for s in range(inst + 1)] + [16 + s for s in range(inst + 1)]))
    assert backend == "valu"
    return tuple(range(next((w for s, w in VALU_DWORDS if step <= s), 32)))


FAMILIES = ("zero", "ones", "tail_ones", "prefix_ones", "low_half_ones", "one_bit")


class StructuredPairs(NamedTuple):
    a: np.ndarray          # [n, 16] u64
    b: np.ndarray          # [n, 16] u64
    distance: np.ndarray   # [n] exact Hamming distance of (a[i], b[i]) over all 1024 bits
    family: tuple          # base family of a[i]
    salted: np.ndarray     # [n] bool: the prefix dwords of a[i] carry fair random bits instead of the family's
    placement: tuple       # "in" | "out" | "dword<d>" | "complement": where the differing bits were asked to go
    exact: np.ndarray      # [n] bool: every differing bit is where `placement` says (False: the region was too small and it spilled)


def _pack_bits(bits: np.ndarray) -> np.ndarray:
    return np.packbits(bits.astype(np.uint8), axis=-1, bitorder="little").view(np.uint64).copy()


def structured_pairs(rng: np.random.Generator, tol: int, prefix, reps: int = 1, salted=None) -> StructuredPairs:
    """Pairs whose distance sits exactly on or one over `tol`, on hashes that are nothing like fair coin flips.

    Bases: all zero / all 1024 bits one (padding bits included) / the dwords outside `prefix` ones and the prefix zero / the
    reverse / dwords 0..15 ones / one set bit (what a constant clip hashes to), each plain and "salted" (the prefix dwords
    replaced by fair random bits, drawn per pair: pairs of different bases are then as far apart as unrelated hashes are over
    the prefix).  salted = None: both forms, True / False: only that one.
    Placements of the differing bits, per base: all inside `prefix` at tol and tol + 1; all outside at tol and tol + 1 (prefix
    distance 0); for tol < 32, all inside one dword d, every d, at tol and tol + 1 bits; the complement (1024).  A region
    with too few bits is filled and the rest spills into the other one (`exact` False); distances are capped at 1024.
    `reps` draws of everything random (bit positions, salts, the one set bit)."""
    in_prefix = np.zeros(1024, bool)
    for d in prefix:
        in_prefix[32 * d: 32 * d + 32] = True
    reg_in, reg_out = np.flatnonzero(in_prefix), np.flatnonzero(~in_prefix)

    def base_bits(family):
        if family == "zero":
            return np.zeros(1024, np.uint8)
        if family == "ones":
            return np.ones(1024, np.uint8)
        if family == "tail_ones":
            return (~in_prefix).astype(np.uint8)
        if family == "prefix_ones":
            return in_prefix.astype(np.uint8)
        if family == "low_half_ones":
            return (np.arange(1024) < 512).astype(np.uint8)
        bits = np.zeros(1024, np.uint8)
        bits[int(rng.integers(0, 1024))] = 1
        return bits

    def pick(first, second, k):
        k = min(k, 1024)
        n1 = min(k, len(first))
        idx = rng.choice(first, size=n1, replace=False)
        if k > n1:
            idx = np.concatenate([idx, rng.choice(second, size=k - n1, replace=False)])
        return idx, k == n1

    placements = [("in", tol), ("in", tol + 1), ("out", tol), ("out", tol + 1)]
    if tol < 32:
        placements += [(f"dword{d}", k) for d in range(32) for k in (tol, tol + 1)]
    placements.append(("complement", 1024))
    forms = (False, True) if salted is None else (bool(salted),)
    rows_a, rows_b, dist, fam, salt, plc, exact = [], [], [], [], [], [], []
    for _ in range(reps):
        for family in FAMILIES:
            for s in forms:
                for where, k in placements:
                    a = base_bits(family)
                    if s:
                        a[reg_in] = rng.integers(0, 2, size=len(reg_in), dtype=np.uint8)
                    if where == "in":
                        flips, ok = pick(reg_in, reg_out, k)
                    elif where == "out":
                        flips, ok = pick(reg_out, reg_in, k)
                    elif where == "complement":
                        flips, ok = np.arange(1024), True
                    else:
                        d = int(where[5:])
                        flips, ok = pick(np.arange(32 * d, 32 * d + 32), np.zeros(0, np.int64), k)
                    b = a.copy()
                    b[flips] ^= 1
                    rows_a.append(a); rows_b.append(b); dist.append(len(flips))
                    fam.append(family); salt.append(s); plc.append(where); exact.append(ok)
    a, b = _pack_bits(np.stack(rows_a)), _pack_bits(np.stack(rows_b))
    distance = np.array(dist, np.int64)
    assert all(hamming(a[i], b[i]) == distance[i] for i in range(len(a)))
    return StructuredPairs(a, b, distance, tuple(fam), np.array(salt, bool), tuple(plc), np.array(exact, bool))


def _dword_counts(x: np.ndarray) -> np.ndarray:
    """[n, 16] u64 -> [n, 32] popcounts of the packed dwords"""
    x = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, HASH_WORDS)
    return np.unpackbits(x.view(np.uint8).reshape(len(x), 32, 4), axis=2).sum(axis=2).astype(np.int64)


def all_distances(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """[len(x), len(y)] exact Hamming distances over all 1024 bits (brute force; the tests' sets are ~1000 hashes)"""
    bx = np.unpackbits(np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, HASH_WORDS).view(np.uint8), axis=1).astype(np.float32)
    by = np.unpackbits(np.ascontiguousarray(y, dtype=np.uint64).reshape(-1, HASH_WORDS).view(np.uint8), axis=1).astype(np.float32)
    dot = bx @ by.T  # integers <= 1024: exact in f32
    return (bx.sum(1)[:, None] + by.sum(1)[None, :] - 2 * dot).astype(np.int64)


MUTANTS = ("linear", "strict", "full_pop", ("stale", 7), ("stale", 13), ("stale", 16), "pad_masked", "tol_unclamped")


def prefix_filter_twin(a, b, prefix, tol: int, mutant=None) -> np.ndarray:
    """Numpy twin of the prefix test, pairwise over a[i], b[i]: True = the pair stays a suspect and goes to the exact pass.
    Written in the matrix-core kernel's own form (f32 half-integers): with paK, pbK the popcounts of row and column over the
    prefix dwords and dotK = popcount(a & b) over them,  acc = dotK - paK / 2  >=  (pbK - min(tol, 1024)) / 2,  which is
    (prefix distance <= tol) - the VALU kernel's integer test.  Mutants (each one plausible slip):
      "linear"        popcounts taken over dwords 0 .. len(prefix) - 1 instead of the streamed ones
      "strict"        > for >=
      "full_pop"      popcounts over all 32 dwords
      ("stale", K)    the column popcount left over from an expansion for K k-steps (dwords s, 16 + s for s < K)
      "pad_masked"    bits 1000..1023 cleared before anything is counted
      "tol_unclamped" tol instead of min(tol, 1024)"""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, HASH_WORDS).copy()
    b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, HASH_WORDS).copy()
    if mutant == "pad_masked":
        a[:, 15] &= np.uint64((1 << 40) - 1)
        b[:, 15] &= np.uint64((1 << 40) - 1)
    sel = sorted(prefix)
    pa, pb, dot = _dword_counts(a), _dword_counts(b), _dword_counts(a & b)
    pop_sel = sel
    if mutant == "linear":
        pop_sel = list(range(len(sel)))
    elif mutant == "full_pop":
        pop_sel = list(range(32))
    col_sel = pop_sel
    if isinstance(mutant, tuple) and mutant[0] == "stale":
        col_sel = [s for s in range(mutant[1])] + [16 + s for s in range(mutant[1])]
    tol_f = np.float32(tol if mutant == "tol_unclamped" else min(tol, 1024))
    acc = dot[:, sel].sum(1).astype(np.float32) - np.float32(0.5) * pa[:, pop_sel].sum(1).astype(np.float32)
    thr = np.float32(0.5) * (pb[:, col_sel].sum(1).astype(np.float32) - tol_f)
    return acc > thr if mutant == "strict" else acc >= thr


class SearchCase(NamedTuple):
    cand: np.ndarray       # [n, 16] u64 candidates (self mode: the whole set), shuffled
    refs: np.ndarray       # [m, 16] u64 references, shuffled (self mode: empty)
    cand_of: np.ndarray    # pair i -> candidate index of b[i]
    ref_of: np.ndarray     # pair i -> reference index of a[i] (self mode: candidate index of a[i])
    pairs: StructuredPairs


def refs_case(rng, tol: int, prefix, n_cand: int = 1100, reps=None) -> SearchCase:
    """search_with_references outputs every hit: references = the a's, candidates = the b's plus iid fillers up to n_cand,
    both shuffled - pairs on every wave, row tile and lane group of a 256-row tile, every sub-tile of a 128-column stage, and
    across the padded tails.  All durations are meant to be equal (every reference sees every candidate)."""
    if reps is None:
        reps = 1 if tol < 32 else 13  # 12 bases x (5 | 69) placements per draw: ~800 pairs either way
    sp = structured_pairs(rng, tol, prefix, reps=reps)
    n = len(sp.a)
    cand = np.concatenate([sp.b, random_hashes(rng, max(n_cand - n, 0))])
    cperm, rperm = rng.permutation(len(cand)), rng.permutation(n)
    cand_of, ref_of = np.empty(len(cand), np.int64), np.empty(n, np.int64)
    cand_of[cperm] = np.arange(len(cand))
    ref_of[rperm] = np.arange(n)
    return SearchCase(cand[cperm], sp.a[rperm], cand_of[:n], ref_of, sp)


def self_case(rng, tol: int, prefix, n: int = 1100) -> SearchCase:
    """search() compares groups, and a dense cluster re-absorbs a lost hit: salted pairs only (isolated wherever unrelated
    prefixes are further apart than tol), a's, b's and iid fillers shuffled into one set of n hashes, equal durations."""
    per_draw = 6 * (5 if tol >= 32 else 69)
    sp = structured_pairs(rng, tol, prefix, reps=max(1, (n // 2 - 8) // per_draw), salted=True)
    keep = np.sort(rng.permutation(len(sp.a))[: n // 2])
    sp = StructuredPairs(sp.a[keep], sp.b[keep], sp.distance[keep], tuple(sp.family[i] for i in keep), sp.salted[keep],
                         tuple(sp.placement[i] for i in keep), sp.exact[keep])
    m = len(sp.a)
    allh = np.concatenate([sp.a, sp.b, random_hashes(rng, n - 2 * m)])
    perm = rng.permutation(n)
    # the last two positions hold a pair exactly on the tolerance: a row of the partly padded last row tile with a column of the
    # padded last stage (n = 513: the last row of a full 512-row tile against the tile's one-row remainder)
    on_tol = np.flatnonzero(sp.exact & (sp.distance == min(tol, 1024)) & (np.array(sp.placement) == "in"))
    k = int(on_tol[0] if len(on_tol) else 0)
    for member, pos in ((k, n - 2), (m + k, n - 1)):
        at = int(np.flatnonzero(perm == member)[0])
        perm[[at, pos]] = perm[[pos, at]]
    where = np.empty(n, np.int64)
    where[perm] = np.arange(n)
    return SearchCase(allh[perm], np.zeros((0, HASH_WORDS), np.uint64), where[m: 2 * m], where[:m], sp)


def search_combos():
    """Every (backend, instantiated step, tolerance) the structured GPU tests search at: the automatic step on both sides of
    each of its changes plus the forced-step table.  Sorted, without repeats."""
    out = set()
    for backend in ("mfma", "valu"):
        for tol in AUTO_TOLERANCES:
            out.add((backend, instantiated_step(backend, auto_step(tol)), tol))
        for step, tol in FORCED_STEP_TOLERANCES:
            out.add((backend, instantiated_step(backend, step), tol))
    return sorted(out)


def corpus_rng(tol: int, prefix) -> np.random.Generator:
    """One corpus per (tolerance, prefix), the same in the CPU and the GPU tests."""
    return np.random.default_rng([4242, tol, len(prefix), int(sum(prefix))])
