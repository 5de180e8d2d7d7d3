"""Shared by the zero-plane / flipped-hash tests: clip content with exact zero coefficients, the flips themselves, and
the oracle's side of every comparison - the hash, the zero plane (coefs == 0.0, packed like a hash) and the hash of the actually flipped
frames.  numpy + the CPU oracle only.

variant v: bit 0 = mirror along W, bit 1 = flip along H, bit 2 = reverse the 16 frames used."""
from __future__ import annotations

import numpy as np

import framegen
from oracle import vdf_oracle as orc

KINDS = framegen.KINDS + ("static", "constant", "x_symmetric")  # 7: a prime, so that the clips a persistent workgroup takes in turn differ in kind
HOST_KINDS = ("noise", "static", "constant", "x_symmetric", "t_symmetric", "blocks4")


def clip(kind: str, rng: np.random.Generator, h: int, w: int) -> np.ndarray:
    """One [16, h, w] u8 clip.  static: one noise frame 16 times (every kt > 0 coefficient is 0.0: 900 zeros); constant: one grey level (999);
    x_symmetric: every row its own mirror image (kx odd: 500); t_symmetric: frame t == frame 15 - t (kt odd: 500); blocks4: 4 x 4 cells of 0 / 255;
    noise: iid (none)."""
    if kind in framegen.KINDS:
        return framegen.clips(kind, rng, 1, h, w)[0]
    if kind == "noise":
        return rng.integers(0, 256, size=(16, h, w), dtype=np.uint8)
    if kind == "static":
        return np.repeat(rng.integers(0, 256, size=(1, h, w), dtype=np.uint8), 16, axis=0)
    if kind == "constant":
        return np.full((16, h, w), int(rng.integers(1, 255)), np.uint8)
    if kind == "x_symmetric":
        half = rng.integers(0, 256, size=(16, h, (w + 1) // 2), dtype=np.uint8)
        return np.ascontiguousarray(np.concatenate([half, half[:, :, ::-1][:, :, w % 2:]], axis=2))
    if kind == "t_symmetric":
        half = rng.integers(0, 256, size=(8, h, w), dtype=np.uint8)
        return np.ascontiguousarray(np.concatenate([half, half[::-1]], axis=0))
    if kind == "blocks4":
        cells = rng.integers(0, 2, size=(16, (h + 3) // 4, (w + 3) // 4), dtype=np.uint8) * 255
        return np.ascontiguousarray(np.repeat(np.repeat(cells, 4, axis=1), 4, axis=2)[:, :h, :w])
    raise ValueError(kind)


def flip(frames: np.ndarray, v: int) -> np.ndarray:
    """The first 16 frames of [n >= 16, h, w], flipped by variant v."""
    f = frames[:16]
    if v & 1:
        f = f[:, :, ::-1]
    if v & 2:
        f = f[:, ::-1, :]
    if v & 4:
        f = f[::-1]
    return np.ascontiguousarray(f)


def pack_bits(bits1000: np.ndarray) -> np.ndarray:
    b = np.zeros(1024, np.uint8)
    b[:1000] = bits1000
    return np.packbits(b, bitorder="little").view(np.uint64).copy()


def oracle_planes(frames: np.ndarray):
    """(hash [16] u64, zero plane [16] u64, number of exact zeros) of one clip by the oracle."""
    rc, words, coefs = orc.hash_clip(np.ascontiguousarray(frames), want_coefs=True)
    assert rc == 0
    z = coefs == 0.0
    return words, pack_bits(z), int(z.sum())


def oracle_variant(frames: np.ndarray, v: int) -> np.ndarray:
    """The oracle's hash of the actually flipped frames."""
    rc, words, _ = orc.hash_clip(flip(frames, v))
    assert rc == 0
    return words


def variant_mask(v: int) -> np.ndarray:
    """M_v of the issue's formula, written out independently of the library: [16] u64."""
    i = np.arange(1000)
    kt, kx, ky = i // 100, (i // 10) % 10, i % 10
    return pack_bits((((v & 1) * kx + ((v >> 1) & 1) * ky + ((v >> 2) & 1) * kt) & 1).astype(np.uint8))
