"""Shared by the retimed-window tests: the oracle's retimed windows of a video, a small corpus of videos and copies of them at another
frame rate, and a brute-force twin of api.align_retimed written from its definition.  numpy + the CPU oracle only."""
from __future__ import annotations

import math

import numpy as np

from oracle import vdf_oracle as orc

RATES = [(6, 5), (5, 4), (3, 2), (31, 16), (2, 1)]


def taps(rate) -> np.ndarray:
    return np.array([(i * rate[0]) // rate[1] for i in range(16)])


def span(rate) -> int:
    return (15 * rate[0]) // rate[1] + 1


def n_windows(n_frames: int, stride: int, rate) -> int:
    return 0 if n_frames < span(rate) else (n_frames - span(rate)) // stride + 1


def oracle_windows(frames: np.ndarray, rate, stride: int = 1):
    """(hashes [n_win, 16] u64, don't-care counts [n_win]) of one video [F, h, w]: oracle.hash_clip of the 16 frames k * stride + tap(i) gathered into a stack."""
    t = taps(rate)
    words, dc = [], []
    for k in range(n_windows(len(frames), stride, rate)):
        rc, w, coefs = orc.hash_clip(np.ascontiguousarray(frames[k * stride + t]), want_coefs=True)
        assert rc == 0
        words.append(w)
        dc.append(int((np.abs(coefs) < 1e-6).sum()))
    return np.stack(words).reshape(-1, 16), np.array(dc, np.uint32)


def corpus(rate, seed: int):
    """Six videos of noise frames at 16 x 16: (A, B), A = two sources, B = four files at den / num of the sources' frames, B[j] = A[c + (j * num) // den]:
    B0 an excerpt of A0 from c = 0, B1 an excerpt of A1 from c = 7, B2 an excerpt of A0 from c = 13, ten frames of noise, then a shorter excerpt of A1
    from c = 0 (two excerpts in one file), B3 unrelated.  Every excerpt stays inside its source at every rate up to 2 / 1, and starts in its file at a
    multiple of 10 frames - of every den in use - so that the windows of B at multiples of den hold exactly the taps of a window of A."""
    num, den = rate
    rng = np.random.default_rng(seed)
    noise = lambda n: rng.integers(0, 256, size=(n, 16, 16), dtype=np.uint8)
    a0, a1 = noise(100), noise(90)
    cut = lambda a, c, n: a[c + (np.arange(n) * num) // den]
    b = [cut(a0, 0, 40), cut(a1, 7, 36), np.concatenate([cut(a0, 13, 30), noise(10), cut(a1, 0, 24)]), noise(40)]
    return [a0, a1], [np.ascontiguousarray(x) for x in b]


EXCERPTS = {(0, 0): (0, 0, 40), (1, 1): (7, 0, 36), (0, 2): (13, 0, 30), (1, 2): (0, 40, 24)}  # (a, b) -> (c, first frame in b, frames of b)


def _dist(wa: np.ndarray, wb: np.ndarray) -> np.ndarray:
    """[Na, Nb] hamming distances of two sets of hashes."""
    x = wa[:, None, :] ^ wb[None, :, :]
    return np.unpackbits(x.view(np.uint8), axis=2).sum(axis=2).astype(np.int64)


def align_retimed_twin(words_a, words_b, rate, tol_int: int, min_run: int = 1):
    """api.align_retimed by brute force, from its definition: words_a[a] = the retimed windows of video a at stride 1 ([Na, 16] u64), words_b[b] = the plain
    windows of video b at stride 1.  Every pair, every phase p, every start: the cells (ka + num m, kb + den m) with ka = p (mod num), kb a multiple of den;
    a run = a maximal stretch of consecutive cells within tol; per phase the best run by n (tol + 1) - dist_sum (ties: the smaller kb / den - (ka - p) / num, then
    the smaller ka - vdf_align_windows' rule on the sub-sampled windows), over the phases the best of those (ties: the smaller first_frame_a, then
    first_frame_b).  -> [(a, b, num, den, first_frame_a, first_frame_b, n_frames_a, n_frames_b, n_windows, mean_distance)] in (a, b) order."""
    num, den = rate
    g = math.gcd(num, den)
    num, den = num // g, den // g
    sp = (15 * num) // den + 1
    tol = min(tol_int, 1024)
    out = []
    for a, wa in enumerate(words_a):
        for b, wb in enumerate(words_b):
            if not len(wa) or not len(wb):
                continue
            d = _dist(wa, wb)
            best = None
            for p in range(num):
                na, nb = len(range(p, len(wa), num)), len(range(0, len(wb), den))
                phase_best = None
                for off in range(-(na - 1), nb):  # the diagonals of the sub-sampled matrix
                    i = max(0, -off)
                    while i < na and i + off < nb:
                        if d[p + num * i, den * (i + off)] > tol:
                            i += 1
                            continue
                        i0, ds = i, 0
                        while i < na and i + off < nb and d[p + num * i, den * (i + off)] <= tol:
                            ds += int(d[p + num * i, den * (i + off)])
                            i += 1
                        n = i - i0
                        if n >= min_run:
                            key = (-(n * (tol + 1) - ds), off, i0)
                            if phase_best is None or key < phase_best[0]:
                                phase_best = (key, n, ds)
                if phase_best is not None:
                    (neg_score, off, i0), n, ds = phase_best
                    key = (neg_score, p + num * i0, den * (i0 + off))
                    if best is None or key < best[0]:
                        best = (key, n, ds)
            if best is not None:
                (_, fa, fb), n, ds = best
                out.append((a, b, num, den, fa, fb, (n - 1) * num + sp, (n - 1) * den + 16, n, ds / n))
    return out
