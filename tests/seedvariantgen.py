"""Shared by the tests of the seeded flipped alignment: a numpy twin of vdf_align_seed_pairs_variants* and of
vdf_align_windows_variants_pairs* built from the existing twins only - candidates: seedgen.seed_twin on the problem with B replaced by
variantgen.variant_twin's set, per variant, with the a < b filter of variantgen.twin in self mode; records: variantgen.twin filtered by triple -
and the problems both the CPU tests of the host forms and the GPU tests of the kernels solve.  Nothing is imported from the library."""
from __future__ import annotations

import functools

import numpy as np

import aligngen
import hashgen
import planegen
import seedgen
import variantgen

ALL = 0b11111110


def seed_twin(vp: variantgen.VariantProblem, mask=None, min_run=None) -> list:
    """-> the candidate triples [(variant, a, b)] in (variant, a, b) order"""
    p = vp.p
    self_mode = p.b_hashes is None
    bh, bf, bs, bz = (p.a_hashes, p.a_first, p.a_skip, vp.a_zero) if self_mode else (p.b_hashes, p.b_first, p.b_skip, vp.b_zero)
    mask = vp.mask if mask is None else mask
    out = []
    for v in variantgen.ALL_VARIANTS:
        if not mask >> v & 1:
            continue
        d = variantgen.variant_twin(bh, bz, bf, v, bs)
        dh, ds = d if bs is not None else (d, None)
        q = p._replace(b_hashes=dh, b_first=bf, b_skip=ds)  # two-set mode on (A, derived B); in self mode the pairs a < b of it
        out += [(v, a, b) for a, b in seedgen.seed_twin(q, min_run) if not self_mode or a < b]
    return out


def records_twin(vp: variantgen.VariantProblem, triples) -> list:
    """variantgen.twin's records of the listed triples (whatever the problem's own mask says)"""
    want = set(map(tuple, triples))
    return [r for r in variantgen.twin(vp._replace(mask=ALL)) if r[:3] in want]


def triples_of(arr) -> list:
    """a structured array of the library's (VIDEO_PAIR_VARIANT_DTYPE) as the twin's tuples"""
    return [(int(r["variant"]), int(r["a"]), int(r["b"])) for r in arr]


def all_triples(vp: variantgen.VariantProblem, mask=None) -> list:
    mask = vp.mask if mask is None else mask
    return [(v, a, b) for v in variantgen.ALL_VARIANTS if mask >> v & 1 for a, b in seedgen.all_pairs(vp.p)]


def call_args(vp: variantgen.VariantProblem, mask=None) -> dict:
    """keyword arguments of align_seed_pairs_variants_host / Engine.align_seed_pairs_variants"""
    kw = variantgen.call_args(vp)
    if mask is not None:
        kw["variant_mask"] = mask
    return kw


def list_args(vp: variantgen.VariantProblem) -> dict:
    """keyword arguments of align_windows_variants_pairs_host / Engine.align_windows_variants_pairs (the list goes third)"""
    kw = variantgen.call_args(vp)
    del kw["variant_mask"]
    return kw


# ---- the class-major rows (include/vdf.h: vdf_window_class_layout_*), written from the header's text ----------------------------------------------
def class_dest(i: int) -> int:
    """bit i < 1024 of a hash -> its position among the 33 x 32 bits of the layout"""
    if i >= 1000:
        return 125 + (i - 1000)
    kt, kx, ky = i // 100, (i // 10) % 10, i % 10
    c, r = (kx & 1) | (ky & 1) << 1 | (kt & 1) << 2, 25 * (kt >> 1) + 5 * (kx >> 1) + (ky >> 1)
    return r if c == 0 else 32 * (5 + 4 * (c - 1)) + r


_DEST = np.array([class_dest(i) for i in range(1024)])


def _class_major(words: np.ndarray) -> np.ndarray:
    """[n, 16] u64 -> [n, 33] u32"""
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")   # [n, 1024]: bit i of the hash
    out = np.zeros((len(words), 33 * 32), np.uint8)
    out[:, _DEST] = bits
    return np.packbits(out, axis=1, bitorder="little").view(np.uint32)


def class_layout_twin(hashes, first, zero=None, skip=None, min_run=1) -> np.ndarray:
    """the seeds (zero None: [n, 36]) or the rows ([n, 72]) of a set as vdf_window_class_layout_* defines them"""
    first = np.asarray(first).astype(np.int64)
    sk = lambda w: 0 if skip is None else int(skip[w] != 0)
    if zero is None:
        ws = [(w, v) for v in range(len(first) - 1) for w in range(first[v], first[v + 1], min_run)]
        out = np.zeros((len(ws), 36), np.uint32)
        if ws:
            idx = np.array([w for w, _ in ws])
            out[:, :33] = _class_major(hashes[idx])
            out[:, 33] = np.unpackbits(np.ascontiguousarray(hashes[idx]).view(np.uint8), axis=1).sum(1)
            out[:, 34] = [sk(w) for w, _ in ws]
            out[:, 35] = [v for _, v in ws]
        return out
    idx = np.arange(first[0], first[-1])
    out = np.zeros((len(idx), 72), np.uint32)
    if len(idx):
        nz = _class_major(~zero[idx])
        out[:, :33] = _class_major(hashes[idx] & ~zero[idx])
        out[:, 36:69] = nz
        live = np.stack([np.unpackbits(np.ascontiguousarray(nz[:, 5 + 4 * (c - 1):9 + 4 * (c - 1)]).view(np.uint8), axis=1).sum(1) for c in range(1, 8)], axis=1)
        out[:, 33] = sum(live[:, c - 1].astype(np.uint32) << np.uint32(8 * (c - 1)) for c in range(1, 5))
        out[:, 34] = sum(live[:, c - 1].astype(np.uint32) << np.uint32(8 * (c - 5)) for c in range(5, 8))
        out[:, 35] = [sk(w) for w in idx]
    return out


def layout_problem(seed=0):
    """arbitrary words - padding bits set, H & Z != 0 - in a set that begins behind row 0, with empty and one-window videos, skip bytes (any
    non-zero value) and 772 rows: not a multiple of 256.  -> hashes, zero, first, skip"""
    rng = np.random.default_rng([83, 20, seed])
    first = np.array([5, 5, 40, 41, 300, 300, 777], np.uint32)
    hashes = rng.integers(0, 2**64, size=(780, 16), dtype=np.uint64)
    zero = rng.integers(0, 2**64, size=(780, 16), dtype=np.uint64) & rng.integers(0, 2**64, size=(780, 16), dtype=np.uint64)
    zero[::7] = 0
    zero[3::11] = np.uint64(2**64 - 1)
    skip = (rng.random(780) < 0.2).astype(np.uint8) * rng.integers(1, 256, size=780).astype(np.uint8)
    return hashes, zero, first, skip


# ---- builders ---------------------------------------------------------------------------------------------------------------------------
def _own(p: aligngen.Problem) -> aligngen.Problem:
    """seedgen's cases are cached and shared: a problem of our own to plant into"""
    c = lambda x: None if x is None else np.array(x, copy=True)
    return p._replace(a_hashes=c(p.a_hashes), b_hashes=c(p.b_hashes), a_skip=c(p.a_skip), b_skip=c(p.b_skip))


def static_planes(rng, hashes: np.ndarray) -> np.ndarray:
    """planes of 900 bits (every coefficient of temporal frequency > 0) on a third of the rows, sparse random planes on the others"""
    z = variantgen.random_planes(rng, hashes, 0.05)
    static = planegen.pack_bits((np.arange(1000) >= 100).astype(np.uint8))
    z[rng.random(len(hashes)) < 0.33] = static
    return z


def with_planes(seed, p: aligngen.Problem, mask: int, density, plants: int = 0) -> variantgen.VariantProblem:
    """variantgen.with_planes on a copy of p (density "static": static_planes), then `plants` stretches planted under variants of the mask: windows
    of a video of A become what the variant set of B shows, with a few bits changed"""
    rng = np.random.default_rng([83, seed])
    p = _own(p)
    self_mode = p.b_hashes is None
    if density == "static":
        bh = p.a_hashes if self_mode else p.b_hashes
        z = static_planes(rng, bh)
        vp = variantgen.VariantProblem(p, z if self_mode else None, None if self_mode else z, mask)
    else:
        vp = variantgen.with_planes(rng, p, mask, density)
    bh, bf, bz = (p.a_hashes, p.a_first, vp.a_zero) if self_mode else (p.b_hashes, p.b_first, vp.b_zero)
    ca, cb = np.diff(p.a_first.astype(np.int64)), np.diff(bf.astype(np.int64))
    live_a, live_b = np.flatnonzero(ca >= 4), np.flatnonzero(cb >= 4)
    variants = [v for v in variantgen.ALL_VARIANTS if mask >> v & 1]
    done = 0
    while done < plants and len(live_a) and len(live_b):
        a, b = int(rng.choice(live_a)), int(rng.choice(live_b))
        if self_mode and a >= b:
            continue
        n = int(rng.integers(1, min(ca[a], cb[b]) + 1))
        variantgen.plant_variant(rng, p.a_hashes, p.a_first, a, int(rng.integers(0, ca[a] - n + 1)), bh, bz, bf, b, int(rng.integers(0, cb[b] - n + 1)), n,
                                 int(rng.choice(variants)), int(rng.integers(0, 30)))
        done += 1
    return vp


def random_problem(rng) -> variantgen.VariantProblem:
    """variantgen.random_problem, then about a third of A's windows made the variant - of the mask or not - of a random window of B with 0 ... 6
    bits changed: at its tolerances of a few bits the planes and the variant decide"""
    vp = variantgen.random_problem(rng)
    p = _own(vp.p)
    self_mode = p.b_hashes is None
    bh, bz = (p.a_hashes, vp.a_zero) if self_mode else (p.b_hashes, vp.b_zero)
    src = bh.copy()
    for k in range(len(p.a_hashes) if len(bh) else 0):
        if rng.random() < 0.33:
            j, v = int(rng.integers(0, len(bh))), int(rng.integers(1, 8))
            p.a_hashes[k] = aligngen.flipped((src[j] ^ planegen.variant_mask(v)) & ~bz[j], int(rng.integers(0, 7)), rng)
    return vp._replace(p=p)  # (self mode, B = A: the planes go with the changed hashes as they are - H & Z != 0 is legal)


def _bits(positions) -> np.ndarray:
    w = np.zeros(16, np.uint64)
    for i in positions:
        w[i // 64] |= np.uint64(1) << np.uint64(i % 64)
    return w


def class_of(i: int) -> int:
    kt, kx, ky = i // 100, (i // 10) % 10, i % 10
    return (kx & 1) | (ky & 1) << 1 | (kt & 1) << 2


PAD = list(range(1000, 1024))


def on_the_tolerance(tol: int = 350) -> variantgen.VariantProblem:
    """One-window videos, pair i = (video i of A, video i of B), even i exactly tol from the variant-v row of b, odd i tol + 1: the deciding bits
    in class 7 (the last streamed), in a class v flips, and among the padding bits 1000 ... 1023 - set in A only, in B only (a B whose padding
    bits survive the derive: Z clear there), in both (they cancel) and in B with Z set there too (the derive clears them) - on rows of B with
    H & Z != 0 throughout.  The variant cycles through 1 ... 7.  `want` of the pair: in, out, in, out, ..."""
    assert tol >= 24, "the padding bits alone are 24 apart"
    rng = np.random.default_rng([83, 7, tol])
    kinds = ["class7", "flipped", "pad_a", "pad_b", "pad_both", "pad_z"]
    n = 2 * len(kinds) * 7
    bh = hashgen.random_hashes(rng, n)
    bz = np.stack([planegen.pack_bits((rng.random(1000) < 0.1).astype(np.uint8)) for _ in range(n)])  # not & ~H: H & Z != 0
    assert (bh & bz).any()
    ah = np.zeros_like(bh)
    i = 0
    for v in variantgen.ALL_VARIANTS:
        m = planegen.variant_mask(v)
        for kind in kinds:
            for over in (0, 1):
                h, z = bh[i].copy(), bz[i].copy()
                if kind in ("pad_b", "pad_both", "pad_z"):
                    h |= _bits(PAD)
                if kind == "pad_z":
                    z |= _bits(PAD)
                bh[i], bz[i] = h, z
                target = (h ^ m) & ~z
                pad_dist = {"class7": 0, "flipped": 0, "pad_a": 24, "pad_b": 24, "pad_both": 0, "pad_z": 24}[kind]
                want_class = {"class7": 7, "flipped": next(c for c in range(1, 8) if bin(v & c).count("1") & 1)}.get(kind)
                a = target.copy()
                if kind in ("pad_a", "pad_both", "pad_z"):
                    a |= _bits(PAD)
                if kind == "pad_b":
                    a &= ~_bits(PAD)
                # the other tol + over - pad_dist differing bits: in the wanted class first (125 of them), then anywhere below 1000
                order = [b for b in range(1000) if class_of(b) == want_class] if want_class is not None else []
                order += [b for b in rng.permutation(1000).tolist() if class_of(b) != want_class]
                a ^= _bits(order[:tol + over - pad_dist])
                ah[i] = a
                assert int(hashgen.all_distances(a[None], target[None])[0, 0]) == tol + over, (v, kind, over)
                i += 1
    first = np.arange(n + 1, dtype=np.uint32)
    return variantgen.VariantProblem(aligngen.Problem(ah, first, bh, first.copy(), tol, 1), None, bz, ALL)


def only_under(v_planted, mask=0b00110010) -> variantgen.VariantProblem:
    """variantgen's planted problem - video 0 of A holds 12 derived windows of video 1 of B under ONE variant - asked for variants 1, 4 and 5:
    planted under 5 (reversed and mirrored) the pair (0, 1) is a candidate under 5 and not under 1 or 4; planted under 1 or under 4, the converse"""
    return variantgen._planted(10 + v_planted, v_planted, mask)


def _tile(name, mask, density, seed, plants=12):
    return lambda: with_planes(seed, seedgen.case(name), mask, density, plants)


BUILDERS = {
    **{f"variant_{n}": (lambda n=n: variantgen.case(n)) for n in variantgen.CASES},
    **{f"variant_{n}_all": (lambda n=n: variantgen.case(n)._replace(mask=ALL)) for n in variantgen.CASES},
    **{f"phases_{m}": _tile(f"phases_{m}", ALL, d, 100 + m, 3) for m, d in ((1, 0.0), (2, 0.05), (3, 0.25), (5, "static"))},
    **{f"phases_self_{m}": _tile(f"phases_self_{m}", ALL, d, 110 + m, 3) for m, d in ((2, 0.25), (3, 0.0))},
    "tile_edges": _tile("tile_edges", ALL, 0.05, 1),
    "tile_edges_dense_planes": _tile("tile_edges", 0b10100100, 0.25, 2),
    "tile_edges_no_planes": _tile("tile_edges", 0b00000010, 0.0, 3),
    "tile_edges_static_planes": _tile("tile_edges", ALL, "static", 4),
    "tile_edges_self": _tile("tile_edges_self", ALL, 0.05, 5),
    "tile_edges_self_static_planes": _tile("tile_edges_self", 0b01101010, "static", 6),
    "tile_edges_tol0": _tile("tile_edges_tol0", ALL, 0.05, 7),
    "tile_edges_all": _tile("tile_edges_all", ALL, 0.25, 8, 0),
    "tile_edges_self_all": _tile("tile_edges_self_all", ALL, 0.05, 9, 0),
    "tile_edges_min_run_1": _tile("tile_edges_min_run_1", ALL, 0.0, 10),
    "tile_edges_min_run_above": _tile("tile_edges_min_run_above", ALL, 0.05, 11),
    "skipped_seeds": _tile("skipped_seeds", ALL, 0.05, 12, 4),
    "skipped_seeds_static_planes": _tile("skipped_seeds", ALL, "static", 13, 4),
    **{f"early_exit_{str(d).replace('.', '')}": _tile("early_exit", ALL, d, 14 + k, 0) for k, d in enumerate((0.0, 0.05, 0.25, "static"))},
    "on_the_tolerance": on_the_tolerance,
    "on_the_tolerance_100": functools.partial(on_the_tolerance, 100),
    "only_under_5": functools.partial(only_under, 5),
    "only_under_1": functools.partial(only_under, 1),
    "only_under_4": functools.partial(only_under, 4),
}


@functools.lru_cache(maxsize=None)
def case(name: str) -> variantgen.VariantProblem:
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def expected(name: str) -> tuple:
    return tuple(seed_twin(case(name)))


@functools.lru_cache(maxsize=None)
def expected_records(name: str) -> tuple:
    """the records of the all-pairs variants call at the case's mask"""
    return tuple(variantgen.twin(case(name)))
