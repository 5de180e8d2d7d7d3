"""Cropdetect::Letterbox on clips of different frame sizes in one call (vdf_cropdetect_letterbox_clips_device, vdf_hash_clips_u8_letterbox[_device];
csrc/cropdetect.hip: cropdetect_mixed_kernel, cropdetect_sides_mixed_kernel) against the CPU oracle, clip by clip: the boxes equal, the hash words equal WHOLE
(no bit masked, padding bits zero), the don't-care count equal.  The corpus is tests/letterbox_mixed_corpus.py (shown not to be vacuous, on the CPU, by
tests/test_hash_mixed_letterbox_corpus.py); it is packed as tests/test_gpu_hash_mixed.py::_pack does - odd offsets, a padded frame_stride on every third clip, a
device buffer of exactly buf_bytes."""
import numpy as np
import pytest

import letterbox_mixed_corpus as lc
from test_gpu_hash_mixed import _bits, _pack as _pack_aa

pytestmark = pytest.mark.gpu

_CACHE = {}


def _pack(clips, seed, tail=0, even=False, fill=0xAA):
    """_pack of the mixed hash tests, with the gaps (and the tail) filled with `fill`."""
    buf, recs = _pack_aa(clips, seed, tail=tail, even=even)
    if fill != 0xAA:
        buf = np.full(len(buf), fill, np.uint8)
        for r, c in zip(recs, clips):
            fb = int(r["w"]) * int(r["h"])
            for f in range(16):
                o = int(r["offset"]) + f * int(r["frame_stride"])
                buf[o:o + fb] = c[f].reshape(-1)
    return buf, recs


def _to_device(buf):
    import torch

    d_buf = torch.empty(len(buf), dtype=torch.uint8, device="cuda")  # exactly buf_bytes
    d_buf.copy_(torch.from_numpy(buf))
    return d_buf


def _detect_call(engine, buf, recs, frames_per_clip=16):
    import torch

    d_buf = _to_device(buf)
    d_crops = torch.full((max(len(recs), 1) * 4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    engine.cropdetect_letterbox_clips_device(d_buf.data_ptr(), len(buf), recs, d_crops.data_ptr(), frames_per_clip=frames_per_clip)
    torch.cuda.synchronize()
    return d_crops.cpu().numpy().view(np.uint32).reshape(-1, 4)[:len(recs)]


def _device_call(engine, buf, recs, frames_per_clip=16):
    import torch

    d_buf = _to_device(buf)
    d_out = torch.full((len(recs) * 16,), -1, dtype=torch.int64, device="cuda")
    d_dc = torch.full((len(recs),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    crops = engine.hash_clips_letterbox_device(d_buf.data_ptr(), len(buf), recs, d_out.data_ptr(), d_dc.data_ptr(), frames_per_clip=frames_per_clip)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint64).reshape(len(recs), 16), crops, d_dc.cpu().numpy().view(np.uint32)


def _host_call(engine, buf, recs, frames_per_clip=16):
    out = np.zeros((len(recs), 16), np.uint64)
    crops = np.zeros((len(recs), 4), np.uint32)
    dc = np.zeros(len(recs), np.uint32)
    engine._check(engine.lib.vdf_hash_clips_u8_letterbox(engine.ctx, buf.ctypes.data, buf.size, recs.ctypes.data, len(recs), frames_per_clip, out.ctypes.data,
                                                         crops.ctypes.data, dc.ctypes.data))
    return out, crops, dc


def _same(got, crops, dc, want, want_crops, want_dc, what="", names=None):
    for i in range(len(want)):
        name = names[i] if names else i
        assert tuple(crops[i]) == tuple(want_crops[i]), f"{what} clip {name}: box {tuple(crops[i])}, oracle {tuple(want_crops[i])}"
    for i in range(len(want)):
        name = names[i] if names else i
        assert np.array_equal(got[i], want[i]), f"{what} clip {name}: {int((_bits(got[i:i + 1]) != _bits(want[i:i + 1])).sum())} hash bits differ"
    assert (_bits(got)[:, 1000:] == 0).all(), "padding bits"
    assert np.array_equal(dc, want_dc), f"{what} don't-care counts {dc} vs {want_dc}"


def _corpus_on_device(engine):
    """The whole corpus through vdf_hash_clips_u8_letterbox_device, once per engine: tests 2 and 4 read it."""
    key = ("device", engine.backend)
    if key not in _CACHE:
        _, clips, _, _, _ = lc.corpus()
        buf, recs = _pack(clips, 1, tail=333)
        assert (recs["offset"] % 2 == 1).all() and (recs["frame_stride"] > recs["w"].astype(np.uint64) * recs["h"]).sum() >= len(clips) // 3
        _CACHE[key] = _device_call(engine, buf, recs)
    return _CACHE[key]


@pytest.mark.parametrize("fill", [0xAA, 0x00])
def test_1_detect_only_whole_corpus_in_one_call(engine, fill):
    """Gaps of 0xAA and of 0x00 (the colour of a black bar): a load that leaves its frame would move a box in one of the two."""
    names, clips, boxes, _, _ = lc.corpus()
    buf, recs = _pack(clips, 1, tail=333, fill=fill)
    got = _detect_call(engine, buf, recs)
    for i, n in enumerate(names):
        assert tuple(got[i]) == tuple(boxes[i]), f"fill {fill:#x} clip {n}: box {tuple(got[i])}, oracle {tuple(boxes[i])}"


def test_2_detect_crop_hash_in_one_device_call(engine):
    names, _, boxes, words, dcs = lc.corpus()
    got, crops, dc = _corpus_on_device(engine)
    _same(got, crops, dc, words, boxes, dcs, "device", names)


def test_3_same_through_the_other_entries(engine):
    import vid_dup_finder_lib_amd as vdf

    names, clips, boxes, words, dcs = lc.corpus()
    buf, recs = _pack(clips, 2, tail=0)
    _same(*_host_call(engine, buf, recs), words, boxes, dcs, "host", names)
    got, crops, dc = engine.hash_clips_letterbox(clips, want_dontcare=True)
    _same(got, crops, dc, words, boxes, dcs, "Engine.hash_clips_letterbox", names)
    pick = [i for i, c in enumerate(clips) if c.shape[1] * c.shape[2] <= 320 * 240][::3]
    vhs = vdf.gen_hashes([clips[i] for i in pick], ["p"] * len(pick), [1] * len(pick), engine=engine)  # default cropdetect: Letterbox
    assert all(np.array_equal(v.hash, words[i]) for v, i in zip(vhs, pick))
    cr = vdf.cropdetect_letterbox([clips[i] for i in pick], engine=engine)
    assert cr == [vdf.Crop.from_abi((clips[i].shape[2], clips[i].shape[1]), boxes[i]) for i in pick]


def test_4_every_clip_alone_on_the_established_route(engine):
    """Engine.hash_frames_letterbox (the uniform letterbox call) on each corpus clip alone gives the box and the words of the mixed call."""
    names, clips, _, _, _ = lc.corpus()
    got, crops, dc = _corpus_on_device(engine)
    for i, c in enumerate(clips):
        one, one_crop, one_dc = engine.hash_frames_letterbox(c[None], want_dontcare=True)
        assert tuple(one_crop[0]) == tuple(crops[i]), (names[i], one_crop[0], crops[i])
        assert np.array_equal(one[0], got[i]) and one_dc[0] == dc[i], names[i]


@pytest.mark.parametrize("size", [(7, 5), (96, 96), (191, 130), (320, 240)])
def test_5_last_clip_ends_on_the_buffers_last_byte(engine, size):
    """A clip of each hash part (and 7 x 5) as the LAST thing of a buffer allocated to exactly buf_bytes, behind a 65 x 64 clip, at odd and even offsets: the box
    and the words it has mid-buffer, which are the oracle's."""
    from oracle import vdf_oracle as orc

    rng = np.random.default_rng(size[0] * 1000 + size[1])
    w, h = size
    last = lc.letterboxed(rng, h, w, bars=(w // 6, w // 5, h // 5, h // 4))
    company = lc.letterboxed(rng, 64, 65)
    filler = lc.letterboxed(rng, 33, 17)
    want = []
    for c in (company, last):
        rc, words, coefs, crop = orc.hash_clip_letterbox(c, want_coefs=True)
        assert rc == 0
        want.append((words, crop, int((np.abs(coefs) < 1e-6).sum())))
    words, boxes, dcs = np.stack([x[0] for x in want]), np.array([x[1] for x in want], np.uint32), np.array([x[2] for x in want], np.uint32)
    assert boxes[1].all()  # four bars
    mid_buf, mid_recs = _pack([company, last, filler], 5, tail=777)
    mid = _device_call(engine, mid_buf, mid_recs)
    _same(mid[0][:2], mid[1][:2], mid[2][:2], words, boxes, dcs, "mid-buffer")
    for even in (False, True):
        buf, recs = _pack([company, last], 3, tail=0, even=even)
        assert int(recs[1]["offset"]) + 15 * int(recs[1]["frame_stride"]) + w * h == len(buf) and int(recs[1]["offset"]) % 2 == (0 if even else 1)
        assert tuple(_detect_call(engine, buf, recs)[1]) == tuple(boxes[1])
        _same(*_device_call(engine, buf, recs), words, boxes, dcs, "last clip")


@pytest.mark.parametrize("n,w,h", [(300, 64, 64), (33, 160, 90)])
def test_6_uniform_batches_are_the_uniform_letterbox_call(engine, n, w, h):
    from test_gpu_letterbox import _letterboxed
    from vid_dup_finder_lib_amd.engine import CLIP_DTYPE

    frames = _letterboxed(np.random.default_rng(n), n, h, w)
    want, want_crops, want_dc = engine.hash_frames_letterbox(frames, want_dontcare=True)
    assert (want_crops != 0).any(axis=1).sum() >= n // 2
    recs = np.zeros(n, CLIP_DTYPE)
    recs["offset"], recs["frame_stride"], recs["w"], recs["h"] = np.arange(n, dtype=np.uint64) * np.uint64(16 * w * h), w * h, w, h
    buf = frames.reshape(-1)
    _same(*_device_call(engine, buf, recs), want, want_crops, want_dc, "uniform device")
    _same(*_host_call(engine, buf, recs), want, want_crops, want_dc, "uniform host")
    assert np.array_equal(_detect_call(engine, buf, recs), want_crops)
    got, crops, dc = engine.hash_clips_letterbox(list(frames), want_dontcare=True)
    _same(got, crops, dc, want, want_crops, want_dc, "uniform list")


def test_7_aligned_probes_give_the_boxes_of_unaligned_ones(engine):
    """640 x 512 and 1920 x 1080 clips with clean 128-column side bars: at a 128-byte aligned offset the side walk probes whole aligned windows, one byte further it
    cannot.  The same boxes, the oracle's."""
    from oracle import vdf_oracle as orc
    from vid_dup_finder_lib_amd.engine import CLIP_DTYPE

    rng = np.random.default_rng(7)
    clips = []
    for w, h in ((640, 512), (1920, 1080)):
        c = lc._picture(rng, h, w)
        c[:, :, :128] = 16
        c[:, :, w - 128:] = 16
        clips.append(c)
    want = np.array([orc.cropdetect_letterbox(c) for c in clips], np.uint32)
    assert [tuple(x) for x in want] == [(128, 128, 0, 0)] * 2
    got = []
    for shift in (0, 1):
        recs = np.zeros(2, CLIP_DTYPE)
        at = shift
        for i, c in enumerate(clips):
            h, w = c.shape[1:]
            recs[i]["offset"], recs[i]["frame_stride"], recs[i]["w"], recs[i]["h"] = at, w * h, w, h
            at = (at + 16 * w * h + 127) // 128 * 128 + shift
        assert (recs["offset"] % 128 == shift).all()
        buf = np.full(int(recs[1]["offset"]) + 16 * 1920 * 1080, 0xAA, np.uint8)
        for r, c in zip(recs, clips):
            buf[int(r["offset"]):int(r["offset"]) + c.size] = c.reshape(-1)
        got.append(_detect_call(engine, buf, recs))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], want), (got, want)


def test_8_every_error_has_its_code_names_its_clip_and_leaves_the_context_usable(engine):
    import vid_dup_finder_lib_amd as vdf

    names, clips, boxes, words, dcs = lc.corpus()
    pick = [next(k for k, c in enumerate(clips) if c.shape[1:] == (hh, ww)) for ww, hh in ((64, 64), (320, 240), (17, 33))]
    buf, recs = _pack([clips[k] for k in pick], 7, tail=0)

    def refused(call, r, code, clip, frames_per_clip=16, nbytes=None, eng=None):
        b = buf if nbytes is None else buf[:nbytes]
        with pytest.raises(vdf.VdfError) as ei:
            call(eng or engine, b, r, frames_per_clip)
        assert ei.value.code == code, (ei.value, code)
        if clip is not None:
            assert f"clip {clip}" in str(ei.value), ei.value

    for call in (_detect_call, _device_call, _host_call):
        refused(call, recs, -1, None, frames_per_clip=15)                    # VDF_E_NOT_ENOUGH_FRAMES
        r = recs.copy(); r[1]["h"] = 0
        refused(call, r, -2, 1)                                              # VDF_E_BAD_DIMS: a zero dimension
        r = recs.copy(); r[2]["frame_stride"] = 17 * 33 - 1
        refused(call, r, -5, 2)                                              # VDF_E_INVAL: frame_stride < w * h
        refused(call, recs, -5, 2, nbytes=len(buf) - 1)                      # a clip past the buffer
        r = recs.copy(); r[1]["crop"] = (0, 0, 3, 0)
        refused(call, r, -5, 1)                                              # a caller-supplied box
        with pytest.raises(vdf.VdfError, match="caller-supplied crop box in a letterbox call"):
            call(engine, buf, r, 16)
        r[2]["frame_stride"] = 1                                             # ... comes after the other errors
        refused(call, r, -5, 2)
        with pytest.raises(vdf.VdfError, match="frame_stride smaller than a frame"):
            call(engine, buf, r, 16)
    multi = vdf.Engine(devices=[0, 0])
    try:
        for call in (_detect_call, _device_call, _host_call):
            refused(call, recs, -5, None, eng=multi)                         # a multi-GPU context
    finally:
        multi.close()
    # the rejected calls launched nothing, and the context goes on: the whole corpus
    cbuf, crecs = _pack(clips, 8, tail=1)
    _same(*_device_call(engine, cbuf, crecs), words, boxes, dcs, "after the errors", names)
    empty = crecs[:0]
    assert len(_detect_call(engine, cbuf, empty)) == 0 and len(_device_call(engine, cbuf, empty)[0]) == 0 and len(_host_call(engine, cbuf, empty)[0]) == 0  # n_clips == 0


def test_10_a_context_gives_back_every_byte():
    import gc

    import torch

    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    names, clips, boxes, words, dcs = lc.corpus()
    buf, recs = _pack(clips, 1, tail=333)
    gc.collect()
    before = (lib.vdf_live_device_bytes(), lib.vdf_live_pinned_bytes())
    eng = vdf.Engine(0)
    eng.backend = "fresh"
    try:
        got = _device_call(eng, buf, recs)
        during = (lib.vdf_live_device_bytes(), lib.vdf_live_pinned_bytes())
    finally:
        eng.close()
    torch.cuda.synchronize()
    _same(*got, words, boxes, dcs, "fresh context", names)
    assert during[0] > before[0] and during[1] > before[1]
    assert (lib.vdf_live_device_bytes(), lib.vdf_live_pinned_bytes()) == before
