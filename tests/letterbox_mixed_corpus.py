"""The seeded corpus of letterboxed clips of different frame sizes that the mixed letterbox tests share (tests/test_hash_mixed_letterbox_corpus.py proves on
the CPU, by the oracle alone, that it is not vacuous; tests/test_gpu_hash_mixed_letterbox.py and tests/test_gpu_hash_queue_mixed_letterbox.py run it on the GPU).
Expected boxes, words and don't-care counts come from the oracle (orc.hash_clip_letterbox, pinned by the reference's own KATs in tests/test_oracle_letterbox.py),
are computed once per session and are not to be modified by a test.

Sizes (w x h) sit on the edges of the three hash parts (small: w <= 256 and h <= 128; lines: w < 192; whole lines: w >= 192) and of the three detect classes
(column batch 8 / 16 / 32 for h < 256 / < 512 / >= 512).  Content is tests/test_gpu_letterbox.py::_letterboxed without its uniform-frame rule (a uniform frame 0
makes the whole clip's box zero): smoothed picture, bars of a random base 0..39 with noise 0..5, bar depth up to 0.3 of the axis.  The special clips are added
one by one below."""
import numpy as np

from oracle import vdf_oracle as orc

SIZES = [(17, 33), (64, 64), (65, 64), (160, 90), (256, 128), (257, 128), (191, 130), (192, 130), (200, 300), (320, 240), (640, 512), (641, 361), (1920, 1080)]
SEED = 2025
_CACHE = {}

KAT_3X3 = [[255] * 9, [0] * 9, [127, 127, 127, 127, 0, 127, 127, 127, 127], [120, 130, 120, 130, 0, 130, 120, 130, 120], [0, 0, 0, 0, 127, 0, 0, 0, 0],
           [127, 0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 200, 0, 0, 120, 0, 0, 100], [0, 0, 0, 0, 127, 0, 0, 0, 127]]  # video_frames_gray.rs:216-443
KAT_6X5 = [0, 0, 0, 0, 0, 0, 255, 255, 255, 0, 0, 255, 255, 255, 0, 0, 255, 255, 255, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]  # :444-459 -> (1, 1, 1, 2)


def hash_part(w, h):
    """Which mixed hash kernel reads a FRAME of this size (csrc/resize_dispatch.cpp: mixed_part_of)."""
    if w <= 256 and (h + 63) // 64 <= 2:
        return "small"
    return "lines" if w < 192 else "wide"


def detect_class(h):
    """The column batch of the side walk (csrc/resize_dispatch.h: letterbox_column_batch)."""
    return 32 if h >= 512 else 16 if h >= 256 else 8


def _picture(rng, h, w):
    frames = rng.integers(40, 220, size=(16, h, w), dtype=np.uint8)
    return (frames // 4 + 60).astype(np.uint8) + rng.integers(0, 60, size=(16, 1, 1), dtype=np.uint8)


def letterboxed(rng, h, w, max_bar=0.3, bars=None):
    """One [16, h, w] clip: _letterboxed's picture and bars; bars = (l, r, t, b) to fix them."""
    frames = _picture(rng, h, w)
    if bars is None:
        l, r = (int(rng.integers(0, int(w * max_bar))) for _ in range(2))
        t, b = (int(rng.integers(0, int(h * max_bar))) for _ in range(2))
    else:
        l, r, t, b = bars
    base = int(rng.integers(0, 40))
    noise = lambda shape: (base + rng.integers(0, 6, size=shape)).astype(np.uint8)  # noqa: E731
    if t: frames[:, :t, :] = noise((16, t, w))        # noqa: E701
    if b: frames[:, h - b:, :] = noise((16, b, w))    # noqa: E701
    if l: frames[:, :, :l] = noise((16, h, l))        # noqa: E701
    if r: frames[:, :, w - r:] = noise((16, h, r))    # noqa: E701
    return frames


def build():
    """[(name, clip [16, h, w])]: the size list, then the special clips."""
    rng = np.random.default_rng(SEED)
    clips = []
    for w, h in SIZES:
        for k in range(3 if w * h <= 320 * 240 else 2 if w * h <= 10**6 else 1):
            clips.append((f"{w}x{h}#{k}", letterboxed(rng, h, w)))
    # one clip per hash part whose frame 8 has a top bar two rows narrower: the union takes the minimum
    for w, h in ((160, 90), (191, 130), (320, 240)):
        t = h // 5
        c = letterboxed(rng, h, w, bars=(w // 9, w // 7, t, h // 8))
        c[8, t - 2:t, :] = rng.integers(100, 200, size=(2, w), dtype=np.uint8)
        clips.append((f"narrower-top {w}x{h}", c))
    # frame 0 uniform: converging edges -> that frame says "no crop", so the clip's box is all zero
    c = letterboxed(rng, 64, 64, bars=(5, 6, 7, 8))
    c[0] = 17
    clips.append(("uniform frame 0", c))
    clips.append(("noise", rng.integers(0, 256, size=(16, 64, 65), dtype=np.uint8)))
    # a bar whose outermost accepted strip (the row next to the picture) has one pixel outside +-16: 191 of 192 pixels stay inside, still > 90 %
    c = letterboxed(rng, 130, 192, bars=(0, 0, 20, 0))
    c[:, 19, 100] = 255
    clips.append(("blemished bar", c))
    for i, px in enumerate(KAT_3X3):
        clips.append((f"kat 3x3 #{i}", np.tile(np.array(px, np.uint8).reshape(1, 3, 3), (16, 1, 1))))
    clips.append(("kat 6x5", np.tile(np.array(KAT_6X5, np.uint8).reshape(1, 6, 5), (16, 1, 1))))
    return clips


def corpus():
    """(names, clips, boxes [n, 4] u32, words [n, 16] u64, don't-care counts [n] u32) - the last three by the oracle; cached, read-only."""
    if "corpus" not in _CACHE:
        named = build()
        boxes, words, dcs = [], [], []
        for name, c in named:
            rc, w, coefs, crop = orc.hash_clip_letterbox(c, want_coefs=True)
            assert rc == 0, (name, rc)
            assert crop == orc.cropdetect_letterbox(c), name
            boxes.append(crop)
            words.append(w)
            dcs.append(int((np.abs(coefs) < 1e-6).sum()))
        out = ([n for n, _ in named], [c for _, c in named], np.array(boxes, np.uint32), np.stack(words), np.array(dcs, np.uint32))
        for a in out[1] + list(out[2:]):
            a.setflags(write=False)
        _CACHE["corpus"] = out
    return _CACHE["corpus"]
