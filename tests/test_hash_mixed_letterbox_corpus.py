"""The corpus of the mixed letterbox GPU tests (tests/letterbox_mixed_corpus.py) is not vacuous - shown by the oracle alone, without a GPU: most clips have a
box, every edge is exercised, every hash part and every detect class sees side bars and top / bottom bars, the special clips do what they are there for."""
import numpy as np

import letterbox_mixed_corpus as lc


def test_corpus_has_the_documented_sizes_and_counts():
    names, clips, boxes, words, dcs = lc.corpus()
    by_size = {}
    for n, c in zip(names, clips):
        assert c.dtype == np.uint8 and c.shape[0] == 16
        if "#" in n and "x" in n and not n.startswith("kat"):
            by_size[(c.shape[2], c.shape[1])] = by_size.get((c.shape[2], c.shape[1]), 0) + 1
    assert by_size == {s: (3 if s[0] * s[1] <= 320 * 240 else 2 if s[0] * s[1] <= 10**6 else 1) for s in lc.SIZES}
    assert sum(by_size.values()) == 35 and len(names) == len(set(names)) == len(boxes) == len(words) == len(dcs)
    assert {lc.hash_part(w, h) for w, h in lc.SIZES} == {"small", "lines", "wide"} and {lc.detect_class(h) for _, h in lc.SIZES} == {8, 16, 32}


def test_most_clips_have_a_box_and_every_edge_is_exercised():
    names, clips, boxes, _, _ = lc.corpus()
    n = len(clips)
    boxed = (boxes != 0).any(axis=1)
    print("boxed", int(boxed.sum()), "of", n, "edges non-zero", (boxes != 0).sum(axis=0))
    assert boxed.sum() >= 0.8 * n
    assert ((boxes != 0).sum(axis=0) >= 0.6 * n).all()
    # every box leaves pixels
    for c, b in zip(clips, boxes):
        assert int(b[0]) + int(b[1]) < c.shape[2] and int(b[2]) + int(b[3]) < c.shape[1]


def test_every_hash_part_and_detect_class_sees_side_bars_and_row_bars():
    _, clips, boxes, _, _ = lc.corpus()
    side, rows = {}, {}
    for c, b in zip(clips, boxes):
        h, w = c.shape[1:]
        for key in (lc.hash_part(w, h), lc.detect_class(h)):
            side[key] = side.get(key, 0) + int(b[0] != 0 or b[1] != 0)
            rows[key] = rows.get(key, 0) + int(b[2] != 0 or b[3] != 0)
    for key in ("small", "lines", "wide", 8, 16, 32):
        assert side.get(key, 0) >= 1 and rows.get(key, 0) >= 1, key


def test_special_clips_do_what_they_are_there_for():
    from oracle import vdf_oracle as orc

    names, clips, boxes, _, _ = lc.corpus()
    at = {n: i for i, n in enumerate(names)}
    assert tuple(boxes[at["kat 6x5"]]) == (1, 1, 1, 2)  # video_frames_gray.rs:444-459
    assert tuple(boxes[at["kat 3x3 #0"]]) == (0, 0, 0, 0) and tuple(boxes[at["kat 3x3 #2"]]) == (1, 1, 1, 1)
    assert tuple(boxes[at["uniform frame 0"]]) == (0, 0, 0, 0) and orc.letterbox_crop(clips[at["uniform frame 0"]][8]) == (5, 6, 7, 8)
    assert tuple(boxes[at["noise"]]) == (0, 0, 0, 0)
    parts = set()
    for n in names:
        if n.startswith("narrower-top"):
            c = clips[at[n]]
            t0, t8 = orc.letterbox_crop(c[0])[2], orc.letterbox_crop(c[8])[2]
            assert t8 == t0 - 2 and boxes[at[n]][2] == t8, (n, t0, t8)  # the union takes the minimum
            parts.add(lc.hash_part(c.shape[2], c.shape[1]))
    assert parts == {"small", "lines", "wide"}
    c = clips[at["blemished bar"]]
    assert abs(int(c[0, 19, 100]) - int(np.bincount(c[0, 19]).argmax())) > 16 and tuple(boxes[at["blemished bar"]]) == (0, 0, 20, 0)
