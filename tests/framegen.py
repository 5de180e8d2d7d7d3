"""Frame CONTENT for the hash tests: seeded, numpy only (the companion of hashgen.py, which makes hashes).

Both resize passes end in clip8((acc + 2^(p-1)) >> p).  Frames of iid uniform noise - what almost every hash test fills its frames with -
all but never reach that clamp from 64 x 64 up: the first pass already averages four or more pixels per tap (one value in 32 768 past a
clamp at 64 x 64, none from 96 x 160 up), and at 270 x 480 the second pass sees operands within [74, 182] and the thumbnails stay within
[117, 137] (the figures are at the end of this text).  A kernel whose clamp, re-centring XOR (u8 -> i8 operands) or pack were wrong for negative or > 255 accumulators passes every
test on such frames.  The classes below are the content that reaches them:

  blocks_noise   per FRAME 15 random cuts per axis, every cell of the 16 x 16 grid 0 or 255, +-6 noise: hard edges about one output pixel
                 apart, both clamps fire in both passes, new rectangles every frame (the temporal DCT axis is live)
  dark_sparse    black (0..3) with isolated white pixels and short horizontal white runs: the negative lobes dominate, the low clamp fires
                 in both passes and most of the thumbnail sits on 0
  bright_sparse  255 - dark_sparse: the high clamp
  ramp_noise     a 0 -> 255 gradient, +-2 noise that tapers to nothing where the ramp reaches 0 and 255, its direction one of 32 at random
                 per clip and turning by 11.25 degrees per frame (one frame of every clip runs exactly along the vertical, where the first
                 pass leaves whole rows of 0 and of 255): no value is clamped, and the second pass's operands cover the whole u8 range,
                 0 and 255 included - the low-frequency regime real hashes live in

Density of the sparse classes (settled on so that at least 3 % of the second pass's values pass their clamp at every size the tests use):
isolated pixels 0.4 % of the frame; runs of 2 ... max(3, w / 8) pixels, ceil(48 * h / (h + 64)) ... twice as many per frame, each repeated on
1 ... max(1, h / 24) consecutive rows - so a frame holds a few dozen marks of about an output pixel's footprint whatever its size (isolated
pixels alone average out: at 300 x 2000 a tap window holds 750 pixels).

resize_twin() restates the fixed-point resize on oracle.np_lanczos3_coeffs (as one exact f64 matrix product per pass), records what reaches
each clamp and can run three mutants - the clamp of one side replaced by a wrap to the low byte, or the second pass fed with operands that
kept the re-centring XOR - for tests/test_hash_content_corpus.py, which shows on the CPU that this corpus sees each of them.

Measured by that test (pytest -s; 2 clips per class; per pass the share of values below 0 / above 255 before the clamp; hash bits of 1000
changed per clip by the mutants no_low_clamp / no_high_clamp / no_recentre, the smallest over the clips), over the sizes 36 x 48 ... 300 x 2000
(rows x columns) of the GPU tests:

  class          pass 1 < 0     pass 1 > 255   pass 1 range   pass 2 < 0     pass 2 > 255   pass 2 range   pass-2 operands   bits changed: low / high / recentre
  blocks_noise   14.1 - 16.3 %  13.8 - 16.5 %  [-45, 299]     7.9 - 9.9 %    7.8 - 9.9 %    [-45, 300]     0 .. 255          264 - 312 / 260 - 307 / 553 - 609
  dark_sparse     7.7 - 12.6 %   1.0 - 2.0 %   [-45, 297]    13.3 - 17.2 %   0 %            [-37, 263]     0 .. 255          407 - 495 / 122 - 161 / 499 - 578
  bright_sparse   1.0 - 2.1 %    7.5 - 12.1 %  [-41, 300]     0 %           13.0 - 17.8 %   [-19, 293]     0 .. 255          125 - 165 / 403 - 504 / 516 - 579
  ramp_noise      0 %            0 %           [0, 255]       0 %            0 %            [4, 251]       0 .. 255          0 / 0 / 456 - 514
  (smallest - largest over the 31 sizes; the test prints every size's row)

iid 0..255 noise, for comparison (test_iid_noise_stays_clear_of_both_clamps prints it; 2 clips): 64 x 64 one first-pass value of 32 768
clamped, range [2, 261], second pass none, [59, 186]; 96 x 160 none, [44, 214] and [96, 157]; 270 x 480 none, [74, 182] and [117, 137].
"""
from __future__ import annotations

import numpy as np

from oracle import vdf_oracle as orc

KINDS = ("blocks_noise", "dark_sparse", "bright_sparse", "ramp_noise")
MUTANTS = ("no_low_clamp", "no_high_clamp", "no_recentre")


def _blocks_frame(rng, h, w):
    def cuts(n):
        k = min(15, n - 1)
        return np.sort(rng.choice(np.arange(1, n), size=k, replace=False)) if k > 0 else np.zeros(0, np.int64)

    ys, xs = cuts(h), cuts(w)
    cells = rng.integers(0, 2, size=(len(ys) + 1, len(xs) + 1), dtype=np.int64) * 255
    rows = np.searchsorted(ys, np.arange(h), side="right")
    cols = np.searchsorted(xs, np.arange(w), side="right")
    img = cells[rows][:, cols] + rng.integers(-6, 7, size=(h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def _dark_frame(rng, h, w):
    img = rng.integers(0, 4, size=(h, w), dtype=np.uint8)
    img[rng.random((h, w)) < 0.004] = 255
    base = -(-48 * h // (h + 64))
    for _ in range(int(rng.integers(base, 2 * base + 1))):
        n = int(rng.integers(2, max(3, w // 8) + 1))
        m = int(rng.integers(1, max(1, h // 24) + 1))
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        img[y:y + m, x:x + n] = rng.integers(252, 256, size=img[y:y + m, x:x + n].shape, dtype=np.uint8)
    return img


def _ramp_clip(rng, h, w):
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    u /= max(w - 1, 1)
    v /= max(h - 1, 1)
    th0 = int(rng.integers(0, 32)) * np.pi / 16  # one of 32 directions: one frame of every clip runs exactly top to bottom (or bottom to top)
    out = np.empty((16, h, w), np.uint8)
    for f in range(16):
        c, s = np.cos(th0 + f * np.pi / 16), np.sin(th0 + f * np.pi / 16)
        t = u * c + v * s
        lo, hi = min(c, 0.0) + min(s, 0.0), max(c, 0.0) + max(s, 0.0)
        base = np.floor((t - lo) / (hi - lo) * 255.0 + 0.5)
        amp = np.minimum(2, np.minimum(base, 255 - base))  # the noise tapers to nothing at both ends: 0 and 255 are reached, and not by clipping
        out[f] = (base + np.rint(rng.uniform(-1, 1, size=(h, w)) * amp)).astype(np.uint8)
    return out


def clips(kind: str, rng: np.random.Generator, n: int, h: int, w: int) -> np.ndarray:
    """n clips of 16 frames of one content class -> uint8 [n, 16, h, w]."""
    out = np.empty((n, 16, h, w), np.uint8)
    for c in range(n):
        if kind == "ramp_noise":
            out[c] = _ramp_clip(rng, h, w)
            continue
        for f in range(16):
            if kind == "blocks_noise":
                out[c, f] = _blocks_frame(rng, h, w)
            elif kind == "dark_sparse":
                out[c, f] = _dark_frame(rng, h, w)
            elif kind == "bright_sparse":
                out[c, f] = 255 - _dark_frame(rng, h, w)
            else:
                raise ValueError(kind)
    return out


def interleaved(rng: np.random.Generator, n_per_kind: int, h: int, w: int):
    """One batch that interleaves clips of all classes (clip i is of class KINDS[i % 4]) -> (uint8 [4 * n_per_kind, 16, h, w], class names)."""
    per = [clips(k, rng, n_per_kind, h, w) for k in KINDS]
    out = np.empty((len(KINDS) * n_per_kind, 16, h, w), np.uint8)
    for i in range(len(KINDS)):
        out[i::len(KINDS)] = per[i]
    return out, [KINDS[i % len(KINDS)] for i in range(len(out))]


def _dense(in_size):
    """The oracle twin's fixed-point coefficients as a dense [in_size, 16] f64 matrix (exact: |q| < 2^15) and their precision."""
    p, _, st, sz, q = orc.np_lanczos3_coeffs(in_size)
    m = np.zeros((in_size, orc.DCT_SIZE))
    for o in range(orc.DCT_SIZE):
        m[st[o]: st[o] + sz[o], o] = q[o, : sz[o]]
    return p, m


def _record(stats, name, v, operands=None):
    if stats is None:
        return
    s = stats.setdefault(name, {"n": 0, "below": 0, "above": 0, "min": None, "max": None, "op_min": None, "op_max": None})
    s["n"] += v.size
    s["below"] += int((v < 0).sum())
    s["above"] += int((v > 255).sum())
    s["min"] = int(v.min()) if s["min"] is None else min(s["min"], int(v.min()))
    s["max"] = int(v.max()) if s["max"] is None else max(s["max"], int(v.max()))
    if operands is not None:
        s["op_min"] = int(operands.min()) if s["op_min"] is None else min(s["op_min"], int(operands.min()))
        s["op_max"] = int(operands.max()) if s["op_max"] is None else max(s["op_max"], int(operands.max()))


def _finish(v, mutate):
    lo = v & 255 if mutate == "no_low_clamp" else 0
    hi = v & 255 if mutate == "no_high_clamp" else 255
    return np.where(v < 0, lo, np.where(v > 255, hi, v))


def resize_twin(frame: np.ndarray, mutate=None, stats=None) -> np.ndarray:
    """[..., h, w] u8 -> [..., 16, 16] u8 thumbnails: horizontal pass, then vertical, each (2^(p-1) + sum) >> p clamped to 0..255 - sums of at
    most 2^35, exact in f64.  stats (a dict, accumulated over calls): per pass ("pass1" horizontal, "pass2" vertical) the number of values
    before the clamp, how many were below 0 / above 255, their range, and the range of the pass's operands.
    mutate: None, or one of MUTANTS - "no_low_clamp" / "no_high_clamp" wrap values past that clamp to their low byte instead, "no_recentre"
    feeds the second pass with operands ^ 0x80 (read as unsigned): what a kernel computes that turns its u8 operands into i8 by that XOR
    and forgets the 128 * 2^p that undoes it."""
    assert mutate is None or mutate in MUTANTS
    x = np.asarray(frame).astype(np.int64)
    h, w = x.shape[-2:]
    if (h, w) == (orc.DCT_SIZE, orc.DCT_SIZE):
        return x.astype(np.uint8)
    if w != orc.DCT_SIZE:
        p, m = _dense(w)
        v = ((1 << (p - 1)) + np.rint(x.astype(np.float64) @ m).astype(np.int64)) >> p
        _record(stats, "pass1", v, x)
        x = _finish(v, mutate)
    if h != orc.DCT_SIZE:
        p, m = _dense(h)
        ops = x ^ 0x80 if mutate == "no_recentre" else x
        v = ((1 << (p - 1)) + np.rint(np.swapaxes(ops, -1, -2).astype(np.float64) @ m).astype(np.int64)) >> p
        v = np.swapaxes(v, -1, -2)
        _record(stats, "pass2", v, x)
        x = _finish(v, mutate)
    return x.astype(np.uint8)
