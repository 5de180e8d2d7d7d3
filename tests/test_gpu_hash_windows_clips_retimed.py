"""vdf_hash_windows_clips_u8_retimed* (csrc/dct_hash.hip: dct_hash_windows_mixed_retimed_kernel behind resize_mfma_mixed_kernel): the RETIMED
windows of videos of different frame sizes and lengths from one call, in the layout the retimed align calls read.  The yardsticks are the uniform retimed call
(Engine.hash_windows_retimed) on each video alone - on a contiguous cropped copy where the video has a box - and the oracle on each window's gathered frames
(tests/retimedgen.py): whole words and don't-care counts, equality, nothing masked.  The library and its yardsticks are made once per (rate, stride) and shared.
The library (W x H x F): 16 x 16 x 31 (exactly the span of 2/1: one window), 16 x 16 x 40, 32 x 32 x 33, 64 x 48 x 47, 96 x 96 x 65 (boxed), 200 x 120 x 32 (the
wide-line resize part, boxed), 640 x 360 x 40 - placed in one buffer in shuffled order, with padded frame strides and gaps."""
import numpy as np
import pytest

import retimedgen
import windowgen

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16, 31), (16, 16, 40), (32, 32, 33), (64, 48, 47), (96, 96, 65), (200, 120, 32), (640, 360, 40)]  # w, h, frames
BOXES = {4: (9, 5, 0, 11), 5: (3, 14, 7, 2)}  # left, right, top, bottom: one video on each side of the 192-column split
RATES = [(6, 5), (3, 2), (2, 1)]
STRIDES = [1, 7, 33]
SENTINEL_ROWS = 8
_CACHE = {}


@pytest.fixture(scope="module")
def eng():
    import vid_dup_finder_lib_amd as vdf

    e = vdf.Engine(0)
    yield e
    e.close()


def _library():
    if "library" not in _CACHE:
        rng = np.random.default_rng(418)
        vids = [windowgen.video(rng, f, h, w, lead=(0, 5, 3)[i % 3]) for i, (w, h, f) in enumerate(SHAPES)]
        crops = np.zeros((len(vids), 4), np.uint32)
        for i, box in BOXES.items():
            crops[i] = box
        cropped = [np.ascontiguousarray(v[:, t:v.shape[1] - b, l:v.shape[2] - r]) for v, (l, r, t, b) in zip(vids, crops)]
        for v in vids + cropped:
            v.setflags(write=False)
        _CACHE["library"] = (vids, crops, cropped)
    return _CACHE["library"]


def _pack(videos, crops=None, order=None, tail=0):
    """One buffer filled with 0xAA: the videos PLACED in `order` (the records stay in the videos' order), gaps between them, offsets that are no multiple of 4,
    frame strides padded by 0 and by 3 bytes in turn."""
    from vid_dup_finder_lib_amd.engine import CLIP_DTYPE

    recs = np.zeros(len(videos), CLIP_DTYPE)
    at = 1
    for i in (range(len(videos)) if order is None else order):
        f, h, w = videos[i].shape
        fs = w * h + (3 if i % 2 else 0)
        at += 5 * (i % 3)
        while at % 4 == 0:
            at += 1
        recs[i]["offset"], recs[i]["frame_stride"], recs[i]["w"], recs[i]["h"] = at, fs, w, h
        at += (f - 1) * fs + w * h
    if crops is not None:
        recs["crop"] = np.asarray(crops, np.uint32).reshape(len(videos), 4)
    buf = np.full(at + tail, 0xAA, np.uint8)
    for r, v in zip(recs, videos):
        fb = v.shape[1] * v.shape[2]
        for f in range(v.shape[0]):
            o = int(r["offset"]) + f * int(r["frame_stride"])
            buf[o:o + fb] = v[f].reshape(-1)
    return buf, recs, np.array([v.shape[0] for v in videos], np.uint32)


def _device_call(eng, buf, recs, n_frames, stride, rate, rows, want_dc=True, raw=False):
    """-> (words [rows, 16], don't-care [rows]); the outputs hold SENTINEL_ROWS more rows than the call may write, filled with a sentinel that must survive."""
    import torch

    d_buf = torch.empty(len(buf), dtype=torch.uint8, device="cuda")  # exactly buf_bytes
    d_buf.copy_(torch.from_numpy(buf))
    d_out = torch.full(((rows + SENTINEL_ROWS) * 16,), -1, dtype=torch.int64, device="cuda")
    d_dc = torch.full((rows + SENTINEL_ROWS,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    try:
        if raw:  # (what the python mirror would refuse: straight to the C ABI)
            nf = np.ascontiguousarray(n_frames, np.uint32)
            eng._check(eng.lib.vdf_hash_windows_clips_u8_retimed_device(eng.ctx, d_buf.data_ptr(), len(buf), recs.ctypes.data if len(recs) else None,
                                                                        nf.ctypes.data if len(recs) else None, len(recs), stride, rate[0], rate[1], d_out.data_ptr(),
                                                                        d_dc.data_ptr(), None))
        else:
            eng.hash_windows_clips_retimed_device(d_buf.data_ptr(), len(buf), recs, n_frames, stride, rate, d_out.data_ptr(), d_dc.data_ptr() if want_dc else 0)
    finally:
        torch.cuda.synchronize()
        out = d_out.cpu().numpy().view(np.uint64).reshape(-1, 16)
        dc = d_dc.cpu().numpy().view(np.uint32)
        _CACHE["last_outputs"] = (out, dc)
    assert (out[rows:] == np.uint64(2**64 - 1)).all() and (dc[rows:] == 2**32 - 1).all(), "a row outside [0, first[n]) was written"
    if not want_dc:
        assert (dc == 2**32 - 1).all()
    return out[:rows], dc[:rows]


def _yardsticks(eng, rate, stride):
    """The uniform retimed call and the oracle on every video alone (the cropped copy where boxed), concatenated in the videos' order; once per (rate, stride)."""
    k = ("want", rate, stride)
    if k not in _CACHE:
        _, _, cropped = _library()
        uni = [eng.hash_windows_retimed(v[None], rate, stride, want_dontcare=True) for v in cropped]
        orc = [retimedgen.oracle_windows(v, rate, stride) for v in cropped]
        _CACHE[k] = (np.concatenate([u[0][0] for u in uni]), np.concatenate([u[1][0] for u in uni]), np.concatenate([o[0] for o in orc]),
                     np.concatenate([o[1] for o in orc]))
    return _CACHE[k]


def _same_rows(got, want, first, what):
    for i in range(len(first) - 1):
        a, b = int(first[i]), int(first[i + 1])
        bad = np.argwhere((got[a:b] != want[a:b]).reshape(b - a, -1).any(axis=1)).reshape(-1)
        assert len(bad) == 0, f"{what}: video {i}, windows {bad[:8].tolist()} differ"


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("rate", RATES)
def test_parity_of_the_device_form_with_the_uniform_call_and_the_oracle(eng, rate, stride):
    import vid_dup_finder_lib_amd as vdf

    vids, crops, _ = _library()
    order = np.random.default_rng(5).permutation(len(vids))
    buf, recs, nf = _pack(vids, crops, order=order, tail=77)
    assert (recs["offset"] % 4 != 0).all() and {int(r["frame_stride"]) - int(r["w"]) * int(r["h"]) for r in recs} == {0, 3}
    assert not np.array_equal(np.argsort(recs["offset"]), np.arange(len(vids)))  # shuffled in the buffer
    first = vdf.hash_windows_first_retimed(nf, rate, stride)
    assert first.tolist() == np.concatenate([[0], np.cumsum([retimedgen.n_windows(int(f), stride, rate) for f in nf])]).tolist()
    if rate == (2, 1):
        assert first[1] - first[0] == 1  # a video of exactly `span` frames gives one window
    rows = int(first[-1])
    uni, uni_dc, orc, orc_dc = _yardsticks(eng, rate, stride)
    assert len(uni) == len(orc) == rows
    got, dc = _device_call(eng, buf, recs, nf, stride, rate, rows)
    _same_rows(got, uni, first, f"rate {rate} stride {stride}: words against the uniform retimed call's")
    _same_rows(dc, uni_dc, first, "don't-care counts against the uniform retimed call's")
    _same_rows(got, orc, first, f"rate {rate} stride {stride}: words against the oracle's on the gathered frames")
    _same_rows(dc, orc_dc, first, "don't-care counts against the oracle's")
    got_n, _ = _device_call(eng, buf, recs, nf, stride, rate, rows, want_dc=False)  # the don't-care pointer null
    assert np.array_equal(got_n, got)
    _CACHE["device", rate, stride] = (got, dc)


@pytest.mark.parametrize("rate,stride", [((6, 5), 1), ((2, 1), 7)])
def test_host_form_equals_device_form(eng, rate, stride):
    import vid_dup_finder_lib_amd as vdf

    vids, crops, _ = _library()
    buf, recs, nf = _pack(vids, crops, order=np.random.default_rng(5).permutation(len(vids)), tail=0)
    first = vdf.hash_windows_first_retimed(nf, rate, stride)
    rows = int(first[-1])
    got, dc = _CACHE.get(("device", rate, stride)) or _device_call(eng, buf, recs, nf, stride, rate, rows)
    out = np.full((rows + 1, 16), 0xFFFFFFFFFFFFFFFF, np.uint64)
    out_dc = np.full(rows + 1, 0xFFFFFFFF, np.uint32)
    eng._check(eng.lib.vdf_hash_windows_clips_u8_retimed(eng.ctx, buf.ctypes.data, buf.size, recs.ctypes.data, nf.ctypes.data, len(recs), stride, rate[0], rate[1],
                                                         out.ctypes.data, out_dc.ctypes.data))
    assert np.array_equal(out[:rows], got) and np.array_equal(out_dc[:rows], dc) and (out[rows] == np.uint64(2**64 - 1)).all() and out_dc[rows] == 2**32 - 1
    words, first_l, dc_l = eng.hash_windows_clips_retimed(vids, rate, stride, crops=crops, want_dontcare=True)  # packed on 64-byte boundaries: the same words
    assert np.array_equal(words, got) and np.array_equal(dc_l, dc) and first_l.tolist() == first.tolist()
    assert eng.hash_windows_clips_retimed([], rate, stride)[0].shape == (0, 16)  # n_videos == 0


@pytest.mark.parametrize("rate", [(6, 5), (2, 1)])
def test_a_thousand_videos_of_exactly_span_frames_one_segment_each(eng, rate):
    """seg_first holds 1000 single-segment entries: every workgroup's binary search ends on another video, and every row is written once."""
    from vid_dup_finder_lib_amd.engine import CLIP_DTYPE

    span = retimedgen.span(rate)
    rng = np.random.default_rng(span)
    frames = rng.integers(0, 256, size=(1000, span, 16, 16), dtype=np.uint8)
    want, want_dc = eng.hash_windows_retimed(frames, rate, 1, want_dontcare=True)
    assert want.shape == (1000, 1, 16)
    recs = np.zeros(1000, CLIP_DTYPE)
    recs["frame_stride"], recs["w"], recs["h"] = 256, 16, 16
    gaps = rng.integers(0, 3, size=1000) * 4  # irregular offsets: not the uniform route
    recs["offset"] = (np.arange(1000) * span * 256 + np.cumsum(gaps)).astype(np.uint64)
    buf = np.full(int(recs["offset"][-1]) + span * 256, 0xAA, np.uint8)
    for i in range(1000):
        buf[int(recs["offset"][i]):int(recs["offset"][i]) + span * 256] = frames[i].reshape(-1)
    got, dc = _device_call(eng, buf, recs, np.full(1000, span, np.uint32), 1, rate, 1000)
    bad = np.argwhere((got != want[:, 0]).any(axis=1)).reshape(-1)
    assert len(bad) == 0, f"videos {bad[:8].tolist()} differ from the uniform retimed call's"
    assert np.array_equal(dc, want_dc[:, 0])


@pytest.mark.parametrize("w,h,nf", [(64, 48, 40), (16, 16, 33)])
def test_a_uniform_library_takes_the_uniform_retimed_route(eng, w, h, nf):
    from vid_dup_finder_lib_amd.engine import CLIP_DTYPE

    rng = np.random.default_rng(w + nf)
    frames = np.stack([windowgen.video(rng, nf, h, w, lead=(0, 5, 3)[c % 3]) for c in range(5)])
    step = nf * w * h + 12  # padded between the videos: still one step
    buf = np.full(5 * step, 0xAA, np.uint8)
    for c in range(5):
        buf[c * step:c * step + nf * w * h] = frames[c].reshape(-1)
    recs = np.zeros(5, CLIP_DTYPE)
    recs["offset"], recs["frame_stride"], recs["w"], recs["h"] = np.arange(5, dtype=np.uint64) * np.uint64(step), w * h, w, h
    for rate, stride in (((6, 5), 1), ((2, 1), 5)):
        want, want_dc = eng.hash_windows_retimed(frames, rate, stride, want_dontcare=True)  # (the same kernels: clip_stride only moves the clips)
        got, dc = _device_call(eng, buf, recs, np.full(5, nf, np.uint32), stride, rate, want.shape[0] * want.shape[1])
        assert np.array_equal(got, want.reshape(-1, 16)) and np.array_equal(dc, want_dc.reshape(-1))


@pytest.mark.parametrize("rate", [(1, 1), (25, 24)])
def test_plain_tap_rates_are_the_plain_mixed_call_word_for_word(eng, rate):
    import torch

    import vid_dup_finder_lib_amd as vdf

    vids, crops, _ = _library()
    buf, recs, nf = _pack(vids, crops, order=np.random.default_rng(5).permutation(len(vids)), tail=3)
    for stride in (1, 7):
        first = vdf.hash_windows_first(nf, stride)
        assert vdf.hash_windows_first_retimed(nf, rate, stride).tolist() == first.tolist()
        rows = int(first[-1])
        got, dc = _device_call(eng, buf, recs, nf, stride, rate, rows)
        d_buf = torch.from_numpy(buf).cuda()
        d_out = torch.zeros(rows * 16, dtype=torch.int64, device="cuda")
        d_dc = torch.zeros(rows, dtype=torch.int32, device="cuda")
        eng.hash_windows_clips_device(d_buf.data_ptr(), len(buf), recs, nf, stride, d_out.data_ptr(), d_dc.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(got, d_out.cpu().numpy().view(np.uint64).reshape(-1, 16)) and np.array_equal(dc, d_dc.cpu().numpy().view(np.uint32))


def test_errors_come_in_the_stated_order_and_launch_nothing(eng):
    import vid_dup_finder_lib_amd as vdf

    vids, crops, _ = _library()
    vids, crops = vids[:4], crops[:4]  # 31, 40, 33 and 47 frames
    buf, recs, nf = _pack(vids, crops)
    rows = int(vdf.hash_windows_first_retimed(nf, (6, 5), 1)[-1])

    def refused(code, video, text, rate, r=recs, f=nf, stride=1, nbytes=None):
        with pytest.raises(vdf.VdfError) as ei:
            _device_call(eng, buf if nbytes is None else buf[:nbytes], r, f, stride, rate, rows, raw=True)
        assert ei.value.code == code and text in str(ei.value), (ei.value, code, text)
        if video is not None:
            assert f"video {video}" in str(ei.value), ei.value
        out, dc = _CACHE["last_outputs"]
        assert (out == np.uint64(2**64 - 1)).all() and (dc == 2**32 - 1).all(), "a rejected call wrote to its outputs"

    last = int(np.argmax(recs["offset"]))
    f15 = nf.copy(); f15[2] = 15
    # the plain mixed call's checks first, in their order, each with a bad rate AND a too-short video behind it
    refused(-1, 2, "fewer than 16", (5, 2), f=f15, stride=0, nbytes=10)
    refused(-5, last, "past the end", (5, 2), nbytes=len(buf) - 1)
    refused(-5, None, "window_stride", (5, 2), stride=0)
    # then the rate, in front of the too-short video (31, 33 and 40 frames are below nothing at 5/2: it is no rate)
    for bad in ((5, 2), (4, 5), (1, 0), (0, 0), (65536, 65536)):
        refused(-5, None, "rate", bad)
    # then the first video shorter than the span: 31 frames at 31/16 (span 30) pass, at 2/1 all four pass, a 30-frame video does not
    f30 = nf.copy(); f30[1] = 30; f30[3] = 29
    refused(-1, 1, "spans", (2, 1), f=f30)
    refused(-1, 3, "spans", (31, 16), f=f30)
    # n_videos == 0: VDF_OK, nothing launched
    got, _ = _device_call(eng, buf, recs[:0], nf[:0], 1, (6, 5), 0, raw=True)
    assert got.shape == (0, 16)
    # the context goes on: the same videos, valid
    _, _, cropped = _library()
    want = np.concatenate([eng.hash_windows_retimed(v[None], (6, 5), 1)[0] for v in cropped[:4]])
    got, _ = _device_call(eng, buf, recs, nf, 1, (6, 5), rows)
    assert np.array_equal(got, want)


def test_a_multi_gpu_context_is_refused(eng):
    import vid_dup_finder_lib_amd as vdf

    multi = vdf.Engine(devices=[0, 0])
    try:
        vids, crops, _ = _library()
        buf, recs, nf = _pack(vids[:2], crops[:2])
        with pytest.raises(vdf.VdfError) as ei:
            _device_call(multi, buf, recs, nf, 1, (6, 5), 4)
        assert ei.value.code == -5 and "single-device" in str(ei.value)
        out, dc = _CACHE["last_outputs"]
        assert (out == np.uint64(2**64 - 1)).all() and (dc == 2**32 - 1).all()
    finally:
        multi.close()


def _planted(rate, seed):
    """Six noise videos of three frame sizes, and three files that hold B[j] = A[c + (j * num) // den] of videos 0, 2 and 4 from c = 0, 7 and 13."""
    num, den = rate
    rng = np.random.default_rng(seed)
    sizes = [(16, 16), (32, 24), (64, 48)]
    a = [rng.integers(0, 256, size=(f, sizes[i % 3][1], sizes[i % 3][0]), dtype=np.uint8) for i, f in enumerate((100, 90, 110, 80, 95, 85))]
    cut = lambda v, c, n: np.ascontiguousarray(v[c + (np.arange(n) * num) // den])
    return a, [cut(a[0], 0, 40), cut(a[2], 7, 36), cut(a[4], 13, 30)], {(0, 0): (0, 40), (2, 1): (7, 36), (4, 2): (13, 30)}


@pytest.mark.parametrize("rate", [(6, 5), (2, 1)])
def test_end_to_end_the_planted_copies_are_found_from_one_call(eng, rate):
    import vid_dup_finder_lib_amd as vdf

    a, b, planted = _planted(rate, 18)
    pa, pb = [f"/a/{i}.mp4" for i in range(len(a))], [f"/b/{i}.mp4" for i in range(len(b))]
    wa = vdf.hash_frame_windows(a, pa, [len(v) for v in a], engine=eng, rate=rate, one_call=True)
    wa_each = vdf.hash_frame_windows(a, pa, [len(v) for v in a], engine=eng, rate=rate)
    assert [len(w) for w in wa] == [retimedgen.n_windows(len(v), 1, rate) for v in a]
    for x, y in zip(wa, wa_each):
        assert len(x) == len(y) and all(np.array_equal(p.hash, q.hash) and p.src_path() == q.src_path() for p, q in zip(x, y))
    wb = vdf.hash_frame_windows(b, pb, [len(v) for v in b], engine=eng)
    got = vdf.align_retimed(wa, wb, rate, tolerance=0.2, min_run=2, engine=eng, native=True)
    assert got == vdf.align_retimed(wa_each, wb, rate, tolerance=0.2, min_run=2, engine=eng, native=True)
    assert sorted((g.a, g.b) for g in got) == sorted(planted), got
    for g in got:
        c, n = planted[g.a, g.b]
        assert (g.first_frame_a, g.first_frame_b, g.mean_distance, g.n_windows) == (c, 0, 0.0, len(range(0, n - 15, rate[1]))), g
        assert g.path_a == pa[g.a] and g.path_b == pb[g.b]


def test_end_to_end_letterbox_boxes_are_detected_then_read_in_place(eng):
    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(19)
    vids = []
    for (w, h), (bar_l, bar_t), f in (((64, 48), (4, 0), 40), ((96, 64), (0, 4), 33), ((200, 120), (4, 4), 47)):
        v = rng.integers(40, 256, size=(f, h, w), dtype=np.uint8)
        v[:, :bar_t] = 16; v[:, h - bar_t:] = 16
        v[:, :, :bar_l] = 16; v[:, :, w - bar_l:] = 16
        vids.append(v)
    paths, durs = [f"/v/{i}.mp4" for i in range(len(vids))], [7, 8, 9]
    boxes = vdf.cropdetect_letterbox(vids, engine=eng)
    assert [(b.left, b.right, b.top, b.bottom) for b in boxes] == [(4, 4, 0, 0), (0, 0, 4, 4), (4, 4, 4, 4)], boxes
    for rate in ((6, 5), (2, 1)):
        auto = vdf.hash_frame_windows(vids, paths, durs, stride=2, engine=eng, rate=rate, one_call=True, letterbox=True)
        by_hand = vdf.hash_frame_windows(vids, paths, durs, stride=2, engine=eng, rate=rate, one_call=True, crops=boxes)
        bare = vdf.hash_frame_windows(vids, paths, durs, stride=2, engine=eng, rate=rate, one_call=True)
        assert any(not np.array_equal(p.hash, q.hash) for p, q in zip(auto[0], bare[0]))  # the bars are not hashed
        for i, (v, c) in enumerate(zip(vids, boxes)):
            cut = np.ascontiguousarray(v[:, c.top:v.shape[1] - c.bottom, c.left:v.shape[2] - c.right])
            want = eng.hash_windows_retimed(cut[None], rate, 2)[0]
            assert len(auto[i]) == len(want) == retimedgen.n_windows(len(v), 2, rate)
            assert np.array_equal(np.stack([x.hash for x in auto[i]]), want), f"video {i} at {rate}: words differ from the uniform retimed call's on the cropped copy"
            assert all(np.array_equal(x.hash, y.hash) for x, y in zip(auto[i], by_hand[i]))
