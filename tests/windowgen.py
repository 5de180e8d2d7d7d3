"""Shared by the window-hash tests: videos whose windows hold exact zero coefficients, and the oracle's hash of every window.
numpy + the CPU oracle only."""
from __future__ import annotations

import numpy as np

import planegen
from oracle import vdf_oracle as orc

STATIC, CONSTANT = 17, 16  # frames: a static stretch of 17 holds two windows that are entirely static, a constant one of 16 holds one


def video(rng: np.random.Generator, n_frames: int, h: int, w: int, lead: int = 5) -> np.ndarray:
    """[n_frames, h, w] u8 from tests/planegen.py pieces concatenated in time: `lead` frames of noise, a static stretch (one noise frame
    repeated: a window inside it has 900 exact zeros), a constant stretch (999), then noise again - cut off at n_frames.  Windows that
    straddle a boundary have few zeros or none."""
    parts = []
    if lead:
        parts.append(rng.integers(0, 256, size=(lead, h, w), dtype=np.uint8))
    parts.append(np.repeat(planegen.clip("static", rng, h, w)[:1], STATIC, axis=0))
    parts.append(np.repeat(planegen.clip("constant", rng, h, w)[:1], CONSTANT, axis=0))
    rest = n_frames - sum(len(p) for p in parts)
    if rest > 0:
        parts.append(rng.integers(0, 256, size=(rest, h, w), dtype=np.uint8))
    return np.ascontiguousarray(np.concatenate(parts)[:n_frames])


def n_windows(n_frames: int, stride: int) -> int:
    return (n_frames - 16) // stride + 1


def oracle_windows(frames: np.ndarray, stride: int):
    """(hashes [n_win, 16] u64, exact zeros per window) of one video: oracle.hash_clip of each window's 16 frames."""
    words, zeros = [], []
    for k in range(n_windows(len(frames), stride)):
        rc, w, coefs = orc.hash_clip(np.ascontiguousarray(frames[k * stride:k * stride + 16]), want_coefs=True)
        assert rc == 0
        words.append(w)
        zeros.append(int((coefs == 0.0).sum()))
    return np.stack(words), zeros
