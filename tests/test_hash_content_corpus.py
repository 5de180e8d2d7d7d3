"""The content corpus of tests/framegen.py can see a wrong clamp or a wrong re-centring - shown with the reference alone, on the CPU.

tests/test_gpu_hash_saturating.py hashes this corpus on every kernel route and compares with the oracle.  That comparison is only worth
what the content is: on iid noise a resize without its low clamp, or without its high clamp, gives the same hashes (from
64 x 64 up next to no value reaches either).  Here, for every size that file uses:

  * framegen.resize_twin (no mutant) equals the C oracle's resize and oracle.np_resize_frame pixel for pixel on every class - the three
    restatements had been compared on content that never saturates only;
  * blocks_noise: at least 5 % of the first pass's values fall below 0 before the clamp and 5 % above 255, 3 % each way in the second pass,
    and each mutant of the twin (no low clamp, no high clamp, no re-centring of the second pass's operands) changes at least 100 of the
    1000 hash bits of every clip;
  * dark_sparse / bright_sparse: at least 3 % of the second pass's values past the low / high clamp, 100 bits from that side's mutant;
  * ramp_noise: no value clamped in either pass, second-pass operands that span at least 0..250 (the ramp's noise tapers off at its ends,
    so 0 is reached without a clamp), 100 bits from no_recentre.

The floors are far under what is measured (pytest -s prints the table; framegen.py's docstring keeps a copy)."""
import numpy as np
import pytest

import framegen
from oracle import vdf_oracle as orc
from test_gpu_hash_saturating import corpus_sizes

SIZES = corpus_sizes()
N_CLIPS = 2  # per class (the numpy hash and np_resize_frame are slow from 1100 columns up)


def _bits(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:1000]


def _pct(stats, name, side):
    return 100.0 * stats[name][side] / stats[name]["n"] if name in stats else 0.0


@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_corpus_reaches_both_clamps_and_sees_every_mutant(h, w):
    for kind in framegen.KINDS:
        frames = framegen.clips(kind, np.random.default_rng([h, w, framegen.KINDS.index(kind)]), N_CLIPS, h, w)
        assert frames.shape == (N_CLIPS, 16, h, w) and frames.dtype == np.uint8
        stats = {}
        thumbs = framegen.resize_twin(frames, None, stats)
        for c in range(N_CLIPS):
            for f in range(16):
                assert np.array_equal(thumbs[c, f], orc.resize_frame(frames[c, f])), (kind, c, f, "twin != C oracle")
                assert np.array_equal(thumbs[c, f], orc.np_resize_frame(frames[c, f])), (kind, c, f, "twin != numpy oracle")
        base = [_bits(orc.np_hash_frames16(t)) for t in thumbs]
        assert all(np.array_equal(b, _bits(orc.hash_clip(fr)[1])) for b, fr in zip(base, frames))
        changed = {}
        for mutant in framegen.MUTANTS:
            mt = framegen.resize_twin(frames, mutant)
            changed[mutant] = min(int((_bits(orc.np_hash_frames16(t)) != b).sum()) for t, b in zip(mt, base))
        p1, p2 = stats["pass1"], stats["pass2"]
        print(f"{h:4d} x {w:4d} {kind:13s} pass 1 {_pct(stats, 'pass1', 'below'):5.1f} % < 0 {_pct(stats, 'pass1', 'above'):5.1f} % > 255 [{p1['min']}, {p1['max']}]"
              f"  pass 2 {_pct(stats, 'pass2', 'below'):5.1f} % < 0 {_pct(stats, 'pass2', 'above'):5.1f} % > 255 [{p2['min']}, {p2['max']}] operands {p2['op_min']}..{p2['op_max']}"
              f"  bits {changed['no_low_clamp']} / {changed['no_high_clamp']} / {changed['no_recentre']}")
        if kind == "blocks_noise":
            assert _pct(stats, "pass1", "below") >= 5 and _pct(stats, "pass1", "above") >= 5
            assert _pct(stats, "pass2", "below") >= 3 and _pct(stats, "pass2", "above") >= 3
            assert all(changed[m] >= 100 for m in framegen.MUTANTS), changed
        elif kind == "dark_sparse":
            assert _pct(stats, "pass2", "below") >= 3 and changed["no_low_clamp"] >= 100, changed
        elif kind == "bright_sparse":
            assert _pct(stats, "pass2", "above") >= 3 and changed["no_high_clamp"] >= 100, changed
        else:
            assert p1["below"] == p1["above"] == p2["below"] == p2["above"] == 0
            assert p2["op_min"] <= 0 and p2["op_max"] >= 250, (p2["op_min"], p2["op_max"])
            assert changed["no_recentre"] >= 100, changed


def test_iid_noise_stays_clear_of_both_clamps():
    """What the corpus is for: on the frames the other hash tests use, the first pass clamps fewer than one value in 10 000 (64 x 64, its
    four-pixel taps: one value of 32 768 here; none from 96 x 160 up), the second pass none, and its values stay within 128 +- 90."""
    for h, w in [(64, 64), (96, 160), (270, 480)]:
        frames = np.random.default_rng([h, w]).integers(0, 256, size=(2, 16, h, w), dtype=np.uint8)
        stats = {}
        framegen.resize_twin(frames, None, stats)
        p1, p2 = stats["pass1"], stats["pass2"]
        print(f"{h:4d} x {w:4d} iid 0..255    pass 1 clamped {p1['below'] + p1['above']} of {p1['n']} [{p1['min']}, {p1['max']}]  pass 2 clamped {p2['below'] + p2['above']} [{p2['min']}, {p2['max']}]")
        assert (p1["below"] + p1["above"]) * 10000 <= p1["n"] and p2["below"] == p2["above"] == 0, stats
        assert 38 <= p2["min"] and p2["max"] <= 218, stats
