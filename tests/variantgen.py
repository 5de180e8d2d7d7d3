"""Shared by the tests of flipped and reversed stretches: the oracle's window hashes WITH their zero planes, whole videos
flipped, a numpy twin of the variant of a set of window hashes (written from the header's text, nothing imported from the library), and
the align problems of tests/aligngen.py extended with zero planes.  numpy + the CPU oracle only."""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import numpy as np

import aligngen
import hashgen
import planegen
import windowgen

ALL_VARIANTS = tuple(range(1, 8))


def flip_video(frames: np.ndarray, v: int) -> np.ndarray:
    """ALL frames of [n, h, w] flipped by variant v (planegen.flip takes the first 16 only)."""
    f = frames
    if v & 1:
        f = f[:, :, ::-1]
    if v & 2:
        f = f[:, ::-1, :]
    if v & 4:
        f = f[::-1]
    return np.ascontiguousarray(f)


def oracle_windows_planes(frames: np.ndarray, stride: int):
    """(hashes [n_win, 16], zero planes [n_win, 16], exact zeros per window) of one video by the oracle."""
    words, planes, zeros = [], [], []
    for k in range(windowgen.n_windows(len(frames), stride)):
        w, z, n = planegen.oracle_planes(frames[k * stride:k * stride + 16])
        words.append(w)
        planes.append(z)
        zeros.append(n)
    return np.stack(words), np.stack(planes), zeros


def variant_twin(hashes, zero, first, v, skip=None):
    """Row first[i] + j of the result = (H[src] ^ M_v) & ~Z[src], src = first[i] + j without bit 2 of v, first[i] + N - 1 - j with it."""
    out = np.zeros_like(hashes)
    out_skip = None if skip is None else np.zeros_like(skip)
    m = planegen.variant_mask(v)
    for i in range(len(first) - 1):
        lo, hi = int(first[i]), int(first[i + 1])
        for j in range(hi - lo):
            src = hi - 1 - j if v & 4 else lo + j
            out[lo + j] = (hashes[src] ^ m) & ~zero[src]
            if skip is not None:
                out_skip[lo + j] = skip[src]
    return out if skip is None else (out, out_skip)


class VariantProblem(NamedTuple):
    p: aligngen.Problem
    a_zero: Optional[np.ndarray]   # needed in self mode only
    b_zero: Optional[np.ndarray]
    mask: int


def random_planes(rng, hashes: np.ndarray, density: float = 0.05) -> np.ndarray:
    """Zero planes that go with `hashes`: random bits below 1000, none where the hash has a bit (H & Z == 0)."""
    z = np.stack([planegen.pack_bits((rng.random(1000) < density).astype(np.uint8)) for _ in range(len(hashes))] + [np.zeros(16, np.uint64)])[:len(hashes)]
    return z & ~hashes


def with_planes(rng, p: aligngen.Problem, mask: int, density: float = 0.05) -> VariantProblem:
    self_mode = p.b_hashes is None
    return VariantProblem(p, random_planes(rng, p.a_hashes, density) if self_mode else None, None if self_mode else random_planes(rng, p.b_hashes, density), mask)


def twin(vp: VariantProblem):
    """-> [(variant, a, b, offset, start_a, n_windows, dist_sum)] in (variant, a, b) order: aligngen.align_twin on the derived sets"""
    p = vp.p
    self_mode = p.b_hashes is None
    bh, bf, bs, bz = (p.a_hashes, p.a_first, p.a_skip, vp.a_zero) if self_mode else (p.b_hashes, p.b_first, p.b_skip, vp.b_zero)
    out = []
    for v in ALL_VARIANTS:
        if not vp.mask >> v & 1:
            continue
        d = variant_twin(bh, bz, bf, v, bs)
        dh, ds = d if bs is not None else (d, None)
        # in self mode the pairs a < b of A against the DERIVED A: the twin in two-set mode, filtered
        q = p._replace(b_hashes=dh, b_first=bf, b_skip=ds)
        out += [(v,) + r for r in aligngen.align_twin(q) if not self_mode or r[0] < r[1]]
    return out


def records(rec) -> list:
    return [tuple(int(r[k]) for k in ("variant", "a", "b", "offset", "start_a", "n_windows", "dist_sum")) for r in rec]


def plant_variant(rng, vp_hashes_a, af, a, ka, bh, bz, bf, b, kb, n, v, flips=0):
    """Make windows ka .. ka + n of video a of A what the variant-v set of B shows at DERIVED rows kb .. kb + n of video b: a's windows are
    derived from b's (hash, plane) by the formula, then `flips` bits are changed.  With bit 2 of v the source rows of b run backwards."""
    m = planegen.variant_mask(v)
    lo, hi = int(bf[b]), int(bf[b + 1])
    for i in range(n):
        src = hi - 1 - (kb + i) if v & 4 else lo + kb + i
        h = (bh[src] ^ m) & ~bz[src]
        vp_hashes_a[int(af[a]) + ka + i] = aligngen.flipped(h, flips, rng) if flips else h


def _planted(seed, v, mask, ca=(40, 30), cb=(35, 50), tol=350, min_run=2):
    """video 0 of A holds 12 derived windows of video 1 of B under variant v (derived rows 5 ..), video 1 of A a PLAIN copy of video 0 of B"""
    rng = np.random.default_rng([91, seed])
    ah, af = aligngen.videos(rng, ca)
    bh, bf = aligngen.videos(rng, cb)
    bz = random_planes(rng, bh)
    plant_variant(rng, ah, af, 0, 7, bh, bz, bf, 1, 5, 12, v, 3)
    aligngen.plant(rng, ah, af, 1, 2, bh, bf, 0, 4, 10, 0)  # b0[4:14] := a1[2:12]: matches plain, under no variant
    return VariantProblem(aligngen.Problem(ah, af, bh, bf, tol, min_run), None, bz, mask)


def _static(skip: bool):
    """static windows (one hash, plane of 900 bits: every kt > 0 coefficient) on both sides, noise around them; with skip they abstain"""
    rng = np.random.default_rng([91, 20])
    ca, cb = [30, 12], [25, 0, 1]
    ah, af = aligngen.videos(rng, ca)
    bh, bf = aligngen.videos(rng, cb)
    i = np.arange(1000)
    static_plane = planegen.pack_bits((i >= 100).astype(np.uint8))
    sh = hashgen.random_hashes(rng, 1)[0] & ~static_plane
    bz = random_planes(rng, bh)
    a_skip, b_skip = np.zeros(len(ah), np.uint8), np.zeros(len(bh), np.uint8)
    ah[5:15] = sh
    bh[10:18] = sh
    bz[10:18] = static_plane
    a_skip[5:15] = 1
    b_skip[10:18] = 1
    p = aligngen.Problem(ah, af, bh, bf, 350, 1, a_skip if skip else None, b_skip if skip else None)
    return VariantProblem(p, None, bz, 0b10110010)


def _self_mode():
    rng = np.random.default_rng([91, 30])
    counts = [20, 33, 0, 1, 27]
    ah, af = aligngen.videos(rng, counts)
    az = random_planes(rng, ah)
    plant_variant(rng, ah, af, 0, 3, ah, az, af, 1, 10, 9, 5, 2)   # a0 holds reversed + mirrored windows of a1
    plant_variant(rng, ah, af, 4, 0, ah, az, af, 1, 0, 6, 1, 0)    # a4 holds mirrored windows of a1: seen from a = 1, b = 4 through a4's own planes
    plant_variant(rng, ah, af, 1, 25, ah, az, af, 4, 20, 5, 1, 0)  # a1 holds mirrored windows of a4
    return VariantProblem(aligngen.Problem(ah, af, None, None, 350, 2), az, None, 0b00100010)


def _tiny():
    rng = np.random.default_rng([91, 40])
    ah, af = aligngen.videos(rng, [0, 1, 3])
    bh, bf = aligngen.videos(rng, [1, 0, 2])
    bz = random_planes(rng, bh)
    plant_variant(rng, ah, af, 1, 0, bh, bz, bf, 0, 0, 1, 4)
    plant_variant(rng, ah, af, 2, 1, bh, bz, bf, 2, 0, 2, 6)
    return VariantProblem(aligngen.Problem(ah, af, bh, bf, 350, 1), None, bz, 0b11111110)


CASES = {
    "mirrored": lambda: _planted(1, 1, 0b00000010),
    "reversed": lambda: _planted(2, 4, 0b00010000),
    "mirrored_reversed": lambda: _planted(3, 5, 0b00100000),
    "all_variants_order": lambda: _planted(4, 3, 0b11111110, min_run=1),
    "plain_only": lambda: _planted(5, 2, 0b11111010),     # the planted variant (2) is not asked for: only the plain copy is there, and it is invisible
    "static_skipped": lambda: _static(True),
    "static_left_in": lambda: _static(False),
    "self_mode": _self_mode,
    "tiny_videos": _tiny,
}


@functools.lru_cache(maxsize=None)
def case(name: str) -> VariantProblem:
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name: str) -> tuple:
    return tuple(twin(case(name)))


def random_problem(rng) -> VariantProblem:
    """aligngen.random_problem with dense zero planes (a quarter of the bits) and a random mask: at tolerances of a few bits the planes decide"""
    p = aligngen.random_problem(rng)
    return with_planes(rng, p, int(rng.integers(1, 128)) << 1, density=float(rng.choice([0.0, 0.002, 0.25])))


def call_args(vp: VariantProblem) -> dict:
    """keyword arguments of align_windows_variants_host / Engine.align_windows_variants"""
    p = vp.p
    return dict(a_hashes=p.a_hashes, a_first=p.a_first, a_zero=vp.a_zero, b_hashes=p.b_hashes, b_first=p.b_first, b_zero=vp.b_zero, tol_int=p.tol,
                min_run=p.min_run, variant_mask=vp.mask, a_skip=p.a_skip, b_skip=p.b_skip)
