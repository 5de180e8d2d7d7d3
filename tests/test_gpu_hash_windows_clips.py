"""vdf_hash_windows_clips_u8* (csrc/dct_hash.hip: dct_hash_windows_mixed_kernel behind resize_mfma_mixed_kernel): the hash of every 16-frame
window of videos of DIFFERENT frame sizes and lengths from one call, in the layout the align calls read.  The yardstick is the uniform call
(Engine.hash_windows[_planes]) on each video alone - whole words, don't-care counts and zero planes, equality, nothing masked - and the oracle on a sample of
windows.  The library of 12 videos and the uniform call's answers per stride are made once and shared by the tests.
The sizes (W x H): 16 x 16 and 33 x 17 (the small class, which the mixed windows route sends through the whole-line kernels), 64 x 48, 191 x 40 and 192 x 40
(both sides of the cut between the line and the wide-line resize kernel), 300 x 130 (an odd-ish width on the wide side, more than one row block)."""
import numpy as np
import pytest

import windowgen
from oracle import vdf_oracle as orc

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (33, 17), (64, 48), (191, 40), (192, 40), (300, 130)]  # w x h
FRAME_COUNTS = [16, 17, 31, 32, 33, 47, 48, 49, 65, 80]
STRIDES = [1, 3, 16, 17, 40]
_CACHE = {}


@pytest.fixture(scope="module")
def eng():
    import vid_dup_finder_lib_amd as vdf

    e = vdf.Engine(0)
    yield e
    e.close()


def _library():
    """12 videos: every size twice, frame counts drawn from FRAME_COUNTS, in shuffled order; read-only."""
    if "library" not in _CACHE:
        rng = np.random.default_rng(415)
        counts = list(rng.permutation(FRAME_COUNTS)) + [80, 16]
        vids = [windowgen.video(rng, int(counts[i]), h, w, lead=(0, 5, 3)[i % 3]) for i, (w, h) in enumerate(SIZES + SIZES)]
        vids = [vids[i] for i in rng.permutation(len(vids))]
        for v in vids:
            v.setflags(write=False)
        assert {v.shape[0] for v in vids} == set(FRAME_COUNTS) and len({v.shape[1:] for v in vids}) == len(SIZES)
        _CACHE["library"] = vids
    return _CACHE["library"]


def _uniform(eng, key, videos, stride, planes=False):
    """The uniform call on each video alone: (words, don't-care counts[, planes]) concatenated in the videos' order; once per key."""
    k = (key, stride, planes)
    if k not in _CACHE:
        parts = [eng.hash_windows_planes(v[None], stride, want_dontcare=True) if planes else eng.hash_windows(v[None], stride, want_dontcare=True) for v in videos]
        cat = lambda j: np.concatenate([p[j][0] for p in parts])
        _CACHE[k] = (cat(0), cat(2), cat(1)) if planes else (cat(0), cat(1))
    return _CACHE[k]


def _pack(videos, crops=None, tail=0, first_offset=1):
    """One buffer, filled with 0xAA between the videos: offsets that are no multiple of 4, frame strides padded by 0 and by 3 bytes in turn."""
    from vid_dup_finder_lib_amd.engine import CLIP_DTYPE

    recs = np.zeros(len(videos), CLIP_DTYPE)
    at = first_offset
    for i, v in enumerate(videos):
        f, h, w = v.shape
        fs = w * h + (3 if i % 2 else 0)
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


def _device_call(eng, buf, recs, n_frames, stride, planes=False, rows=None):
    """-> (words [rows, 16], don't-care [rows][, planes [rows, 16]]), the outputs filled with a sentinel first."""
    import torch

    import vid_dup_finder_lib_amd as vdf

    if rows is None:
        rows = int(vdf.hash_windows_first(n_frames, stride)[-1])
    d_buf = torch.empty(len(buf), dtype=torch.uint8, device="cuda")  # exactly buf_bytes
    d_buf.copy_(torch.from_numpy(buf))
    d_out = torch.full((max(rows, 1) * 16,), -1, dtype=torch.int64, device="cuda")
    d_zero = torch.full((max(rows, 1) * 16,), -1, dtype=torch.int64, device="cuda")
    d_dc = torch.full((max(rows, 1),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    try:
        if stride == 0:  # (the python mirror refuses it before the library sees it: straight to the C ABI)
            nf = np.ascontiguousarray(n_frames, np.uint32)
            args = (eng.ctx, d_buf.data_ptr(), len(buf), recs.ctypes.data, nf.ctypes.data, len(recs), 0, d_out.data_ptr(), d_dc.data_ptr())
            eng._check(eng.lib.vdf_hash_windows_clips_u8_planes_device(*args, d_zero.data_ptr(), None) if planes else eng.lib.vdf_hash_windows_clips_u8_device(*args, None))
        elif planes:
            eng.hash_windows_clips_planes_device(d_buf.data_ptr(), len(buf), recs, n_frames, stride, d_out.data_ptr(), d_zero.data_ptr(), d_dc.data_ptr())
        else:
            eng.hash_windows_clips_device(d_buf.data_ptr(), len(buf), recs, n_frames, stride, d_out.data_ptr(), d_dc.data_ptr())
    finally:
        torch.cuda.synchronize()
        _CACHE["last_outputs"] = (d_out.cpu().numpy(), d_zero.cpu().numpy(), d_dc.cpu().numpy())
    u64 = lambda t: t.cpu().numpy().view(np.uint64).reshape(-1, 16)[:rows]
    dc = d_dc.cpu().numpy().view(np.uint32)[:rows]
    return (u64(d_out), dc, u64(d_zero)) if planes else (u64(d_out), dc)


def _same_rows(got, want, first, what):
    for i in range(len(first) - 1):
        a, b = int(first[i]), int(first[i + 1])
        bad = np.argwhere((got[a:b] != want[a:b]).reshape(b - a, -1).any(axis=1)).reshape(-1)
        assert len(bad) == 0, f"{what}: video {i}, windows {bad[:8].tolist()} differ from the uniform call's"


@pytest.mark.parametrize("stride", STRIDES)
def test_05_geometry_twelve_videos_in_one_call(eng, stride):
    import vid_dup_finder_lib_amd as vdf

    vids = _library()
    want, want_dc = _uniform(eng, "library", vids, stride)
    buf, recs, nf = _pack(vids, tail=77)
    assert (recs["offset"] % 4 != 0).all() and {int(r["frame_stride"]) - int(r["w"]) * int(r["h"]) for r in recs} == {0, 3}
    first = vdf.hash_windows_first(nf, stride)
    assert first.tolist() == np.concatenate([[0], np.cumsum([windowgen.n_windows(int(f), stride) for f in nf])]).tolist() and first[-1] == len(want)
    got, dc = _device_call(eng, buf, recs, nf, stride)
    _same_rows(got, want, first, f"stride {stride}")
    _same_rows(dc, want_dc, first, f"stride {stride} don't-care counts")
    # the oracle on a sample: the first and the last window of every video
    for i, v in enumerate(vids):
        for k in {0, int(first[i + 1] - first[i]) - 1}:
            rc, words, coefs = orc.hash_clip(np.ascontiguousarray(v[k * stride:k * stride + 16]), want_coefs=True)
            assert rc == 0 and np.array_equal(got[int(first[i]) + k], words), f"video {i} {v.shape} window {k}: words differ from the oracle's"
            assert dc[int(first[i]) + k] == int((np.abs(coefs) < 1e-6).sum())


@pytest.mark.parametrize("size", [(192, 40), (64, 48)])
def test_06_last_video_ends_on_the_buffers_last_byte(eng, size):
    """The careful loaders of both resize parts: the last video's last frame ends on the last byte of a buffer allocated to exactly buf_bytes, and the words
    are the ones it has with slack behind it (and the uniform call's)."""
    import vid_dup_finder_lib_amd as vdf

    vids = _library()
    last = next(v for v in vids if v.shape[1:] == (size[1], size[0]))
    company = next(v for v in vids if v.shape[1:] == (17, 33))
    pair = [company, last]
    for stride in (1, 17):
        want, want_dc = _uniform(eng, ("end", size), pair, stride)
        first = vdf.hash_windows_first([len(v) for v in pair], stride)
        buf, recs, nf = _pack(pair, tail=0)
        assert int(recs[1]["offset"]) + (len(last) - 1) * int(recs[1]["frame_stride"]) + size[0] * size[1] == len(buf)
        got, dc = _device_call(eng, buf, recs, nf, stride)
        slack, recs2, _ = _pack(pair, tail=4096)
        got2, dc2 = _device_call(eng, slack, recs2, nf, stride)
        assert np.array_equal(got, got2) and np.array_equal(dc, dc2), "the result depends on what lies behind the buffer's last video"
        _same_rows(got, want, first, f"last video {size} stride {stride}")
        _same_rows(dc, want_dc, first, "don't-care counts")


def _boxes(videos):
    out = []
    for i, v in enumerate(videos):
        _, h, w = v.shape
        l, r = ((w // 7, w // 9 + 1), (0, 0), (w // 5, 0))[i % 3]
        t, b = ((0, 0), (h // 8, h // 6 + 1), (1, h // 4))[i % 3]
        out.append((l, r, t, b))
    return np.array(out, np.uint32)


def test_07_crop_boxes_are_read_in_place(eng):
    import vid_dup_finder_lib_amd as vdf

    vids = [v for v in _library() if v.shape[1:] != (16, 16)][:8]
    crops = _boxes(vids)
    cropped = [np.ascontiguousarray(v[:, t:v.shape[1] - b, l:v.shape[2] - r]) for v, (l, r, t, b) in zip(vids, crops)]
    stride = 3
    want, want_dc = _uniform(eng, "cropped", cropped, stride)
    buf, recs, nf = _pack(vids, crops=crops, tail=5)
    first = vdf.hash_windows_first(nf, stride)
    got, dc = _device_call(eng, buf, recs, nf, stride)
    _same_rows(got, want, first, "boxes")
    _same_rows(dc, want_dc, first, "boxes, don't-care counts")
    got_l, first_l = eng.hash_windows_clips(vids, stride, crops=crops)
    assert np.array_equal(got_l, want) and first_l.tolist() == first.tolist()


def test_07_letterbox_on_a_list_is_detect_then_boxes(eng):
    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(7)
    vids = []
    for (w, h), (bar_l, bar_t), f in (((64, 48), (6, 0), 33), ((192, 40), (0, 5), 40), ((300, 130), (20, 9), 20), ((33, 17), (0, 0), 17)):
        v = rng.integers(40, 256, size=(f, h, w), dtype=np.uint8)
        v[:, :bar_t] = 16; v[:, h - bar_t:] = 16
        v[:, :, :bar_l] = 16; v[:, :, w - bar_l:] = 16
        vids.append(v)
    paths, durs = [f"/v/{i}.mp4" for i in range(len(vids))], list(range(10, 10 + len(vids)))
    boxes = vdf.cropdetect_letterbox(vids, engine=eng)
    assert [(b.left, b.top) for b in boxes][:3] == [(6, 0), (0, 5), (20, 9)], boxes
    auto = vdf.hash_frame_windows(vids, paths, durs, stride=2, engine=eng, letterbox=True)
    by_hand = vdf.hash_frame_windows(vids, paths, durs, stride=2, engine=eng, crops=boxes)
    plain = vdf.hash_frame_windows(vids, paths, durs, stride=2, engine=eng)
    assert [len(a) for a in auto] == [windowgen.n_windows(len(v), 2) for v in vids]
    for i in range(len(vids)):
        assert all(np.array_equal(a.hash, b.hash) for a, b in zip(auto[i], by_hand[i])), i
        assert auto[i][0].src_path() == paths[i]
    assert any(not np.array_equal(a.hash, p.hash) for a, p in zip(auto[0], plain[0]))  # the bars are not hashed
    # ... and the boxed words are the uniform call's on the cropped copy
    c = boxes[2]
    cut = np.ascontiguousarray(vids[2][:, c.top:130 - c.bottom, c.left:300 - c.right])
    want = eng.hash_windows(cut[None], 2)[0]
    assert np.array_equal(np.stack([a.hash for a in auto[2]]), want)


@pytest.mark.parametrize("stride", [1, 17])
def test_08_planes(eng, stride):
    import vid_dup_finder_lib_amd as vdf

    vids = _library()
    want, want_dc, want_zero = _uniform(eng, "library", vids, stride, planes=True)
    plain, plain_dc = _uniform(eng, "library", vids, stride)
    assert np.array_equal(want, plain) and np.array_equal(want_dc, plain_dc)
    buf, recs, nf = _pack(vids, tail=9)
    first = vdf.hash_windows_first(nf, stride)
    got, dc, zero = _device_call(eng, buf, recs, nf, stride, planes=True)
    got_p, dc_p = _device_call(eng, buf, recs, nf, stride)
    assert np.array_equal(got, got_p) and np.array_equal(dc, dc_p), "hashes and don't-care counts of the planes form are not the plain form's"
    _same_rows(got, want, first, "planes form, words")
    _same_rows(zero, want_zero, first, "planes")
    assert (got & zero == 0).all() and (zero != 0).any()
    # through the list mirror, and on to VideoHash.zero
    w_l, z_l, f_l, dc_l = eng.hash_windows_clips_planes(vids, stride, want_dontcare=True)
    assert np.array_equal(w_l, want) and np.array_equal(z_l, want_zero) and np.array_equal(dc_l, want_dc) and f_l.tolist() == first.tolist()


def test_09_host_form_equals_device_form(eng):
    vids = _library()
    stride = 3
    buf, recs, nf = _pack(vids, tail=0)
    got, dc = _device_call(eng, buf, recs, nf, stride)
    out = np.full((len(got), 16), 0xFFFFFFFFFFFFFFFF, np.uint64)
    out_dc = np.full(len(got), 0xFFFFFFFF, np.uint32)
    eng._check(eng.lib.vdf_hash_windows_clips_u8(eng.ctx, buf.ctypes.data, buf.size, recs.ctypes.data, nf.ctypes.data, len(recs), stride, out.ctypes.data,
                                                 out_dc.ctypes.data))
    assert np.array_equal(out, got) and np.array_equal(out_dc, dc)
    words, first, dc_l = eng.hash_windows_clips(vids, stride, want_dontcare=True)  # packed on 64-byte boundaries: the same words
    assert np.array_equal(words, got) and np.array_equal(dc_l, dc)
    assert eng.hash_windows_clips([], stride)[0].shape == (0, 16)  # n_videos == 0


def test_10_end_to_end_align_finds_the_resized_excerpt(eng):
    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(10)
    coarse = rng.integers(0, 256, size=(80, 6, 8), dtype=np.uint8)
    a = np.kron(coarse, np.ones((1, 8, 8), np.uint8))                   # 80 frames of 64 x 48
    b = np.kron(coarse[20:60], np.ones((1, 16, 16), np.uint8))          # frames 20 .. 59 of it at 128 x 96
    c = rng.integers(0, 256, size=(33, 17, 33), dtype=np.uint8)
    for stride in (1, 4):
        wins = vdf.hash_frame_windows([a, b, c], ["/a.mp4", "/b.mp4", "/c.mp4"], [80, 40, 33], stride=stride, engine=eng)
        assert [len(w) for w in wins] == [windowgen.n_windows(f, stride) for f in (80, 40, 33)]
        got = vdf.align(wins, tolerance=0.2, min_run=2, stride=stride, engine=eng)
        assert [(g.a, g.b, g.offset_frames, g.first_frame_a, g.first_frame_b, g.n_windows) for g in got] == [(0, 1, -20, 20, 0, len(wins[1]))], got
        assert got[0].path_b == "/b.mp4" and got[0].n_frames == (len(wins[1]) - 1) * stride + 16


def test_11_errors_in_order_leave_the_outputs_untouched(eng):
    import vid_dup_finder_lib_amd as vdf

    vids = [v for v in _library() if v.shape[1:] in ((48, 64), (40, 192), (17, 33))][:3]
    buf, recs, nf = _pack(vids, tail=0)
    rows = int(vdf.hash_windows_first(nf, 1)[-1])

    def refused(code, video, r=recs, f=nf, stride=1, nbytes=None, planes=False, null=None):
        b = buf if nbytes is None else buf[:nbytes]
        with pytest.raises(vdf.VdfError) as ei:
            if null == "clips":
                eng._check(eng.lib.vdf_hash_windows_clips_u8_device(eng.ctx, 1, len(b), None, f.ctypes.data, len(f), stride, 1, None, None))
            elif null == "out":
                eng._check(eng.lib.vdf_hash_windows_clips_u8_device(eng.ctx, 1, len(b), r.ctypes.data, f.ctypes.data, len(f), stride, None, None, None))
            elif null == "zero":
                eng._check(eng.lib.vdf_hash_windows_clips_u8_planes_device(eng.ctx, 1, len(b), r.ctypes.data, f.ctypes.data, len(f), stride, 1, None, None, None))
            else:
                _device_call(eng, b, r, f, stride, planes=planes, rows=rows)
        assert ei.value.code == code, (ei.value, code)
        if video is not None:
            assert f"video {video}" in str(ei.value), ei.value
        if null is None:
            out, zero, dc = _CACHE["last_outputs"]
            assert (out == -1).all() and (zero == -1).all() and (dc == -1).all(), "a rejected call wrote to its outputs"

    # every call below carries ALL the later errors of the list as well: the earliest is the one reported
    all_bad = recs.copy()
    all_bad[2]["crop"] = (20, 20, 0, 0)           # 4: 33 - 40 columns
    all_bad[1]["frame_stride"] = int(all_bad[1]["w"]) * int(all_bad[1]["h"]) - 1   # 3
    all_bad[0]["h"] = 0                           # 2
    f_bad = nf.copy()
    f_bad[1] = 15                                 # 1
    for planes in (False, True):
        refused(-1, 1, r=all_bad, f=f_bad, stride=0, nbytes=10, planes=planes)    # 1 VDF_E_NOT_ENOUGH_FRAMES
        refused(-2, 0, r=all_bad, stride=0, nbytes=10, planes=planes)             # 2 VDF_E_BAD_DIMS: a zero dimension
        r = all_bad.copy(); r[0]["h"] = recs[0]["h"]
        refused(-5, 1, r=r, stride=0, nbytes=10, planes=planes)                   # 3 frame_stride < w * h
        r[1]["frame_stride"] = recs[1]["frame_stride"]
        refused(-5, 2, r=r, stride=0, nbytes=10, planes=planes)                   # 4 a box that leaves no pixels
        refused(-5, 0, stride=0, nbytes=10, planes=planes)                        # 5 the video reaches past the buffer
        refused(-5, 2, stride=0, nbytes=len(buf) - 1, planes=planes)              #   ... by one byte of its LAST frame (frame 15 would fit)
        r = recs.copy(); r[1]["offset"] = 2**63; r[1]["frame_stride"] = 2**63
        refused(-5, 1, r=r, stride=0, planes=planes)                              #   ... in 128 bits
        refused(-5, None, stride=0, planes=planes)                                # 6 window_stride == 0
    refused(-5, None, null="clips")                                               # 9 null pointers
    refused(-5, None, null="out")
    refused(-5, None, null="zero")
    f = nf.copy(); f[1] = 2**32 - 10                                              # 7 (with a buffer that large claimed: nothing is read)
    with pytest.raises(vdf.VdfError) as ei:
        eng._check(eng.lib.vdf_hash_windows_clips_u8_device(eng.ctx, 1, 2**63, recs.ctypes.data, f.ctypes.data, 3, 1, 1, None, None))
    assert ei.value.code == -5 and "video 1" in str(ei.value) and "2^32" in str(ei.value)
    big = np.zeros(3, recs.dtype); big["w"] = big["h"] = 1; big["frame_stride"] = 1     # 8: 3 x (2^31 - 15) windows
    f = np.full(3, 2**31, np.uint32)
    with pytest.raises(vdf.VdfError) as ei:
        eng._check(eng.lib.vdf_hash_windows_clips_u8_device(eng.ctx, 1, 2**63, big.ctypes.data, f.ctypes.data, 3, 1, 1, None, None))
    assert ei.value.code == -5 and "2^32 windows" in str(ei.value)
    # a rejected call launched nothing, and the context goes on: the same videos, valid
    want, want_dc = _uniform(eng, "errors", vids, 1)
    got, dc = _device_call(eng, buf, recs, nf, 1)
    assert np.array_equal(got, want) and np.array_equal(dc, want_dc)


def test_11_multi_gpu_context_is_refused_last(eng):
    import vid_dup_finder_lib_amd as vdf

    multi = vdf.Engine(devices=[0, 0])
    try:
        vids = _library()[:2]
        buf, recs, nf = _pack(vids)
        with pytest.raises(vdf.VdfError) as ei:
            _device_call(multi, buf, recs, nf, 1)
        assert ei.value.code == -5 and "single-device" in str(ei.value)
        out, zero, dc = _CACHE["last_outputs"]
        assert (out == -1).all() and (dc == -1).all()
        with pytest.raises(vdf.VdfError) as ei:
            _device_call(multi, buf, recs, nf, 0, rows=4)
        assert "window_stride" in str(ei.value)  # an argument error comes first
    finally:
        multi.close()


@pytest.mark.parametrize("w,h,nf", [(64, 48, 40), (16, 16, 33)])
def test_12_uniform_input_gives_the_uniform_calls_words(eng, w, h, nf):
    from vid_dup_finder_lib_amd.engine import CLIP_DTYPE

    rng = np.random.default_rng(w + nf)
    frames = np.stack([windowgen.video(rng, nf, h, w, lead=(0, 5, 3)[c % 3]) for c in range(7)])
    for stride in (1, 5):
        want, want_dc = eng.hash_windows(frames, stride, want_dontcare=True)
        recs = np.zeros(7, CLIP_DTYPE)
        recs["offset"], recs["frame_stride"], recs["w"], recs["h"] = np.arange(7, dtype=np.uint64) * np.uint64(nf * w * h), w * h, w, h
        got, dc = _device_call(eng, frames.reshape(-1), recs, np.full(7, nf, np.uint32), stride)
        assert np.array_equal(got, want.reshape(-1, 16)) and np.array_equal(dc, want_dc.reshape(-1))
        got_l, first = eng.hash_windows_clips(list(frames), stride)  # (64-byte packing keeps one step here: also the uniform route)
        assert np.array_equal(got_l, want.reshape(-1, 16)) and first.tolist() == (np.arange(8) * want.shape[1]).tolist()
