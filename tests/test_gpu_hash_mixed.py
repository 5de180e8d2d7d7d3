"""Clips of different frame sizes in one call (vdf_hash_clips_u8[_device]; csrc/dct_hash.hip: resize_dct_hash_mixed_small_kernel, resize_mfma_mixed_kernel) against
the CPU oracle, clip by clip.  The rule is tests/test_gpu_hash_parity.py's: whole hash words, no bit masked, padding bits zero, and the don't-care COUNT equal to
the oracle's.  The sizes sit on the edges of the three kernel parts (small: w <= 256 and h <= 128; lines: w < 192; whole lines: w >= 192); with random content
every one of them has 0 don't-care coefficients except 1 x 1 (990 exact zeros), so the whole-word comparison means something for all of them.
The oracle's words are computed once per session and shared by the tests."""
import numpy as np
import pytest

from oracle import vdf_oracle as orc

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 5), (16, 16), (17, 33), (64, 64), (65, 64), (96, 96), (160, 90), (256, 128), (256, 129), (257, 128), (191, 130), (192, 130), (320, 240),
         (641, 361), (1280, 720), (1920, 1080)]  # w x h
SMALL_SIZES = [s for s in SIZES if s[0] <= 256 and s[1] <= 128]
_CACHE = {}


def _bits(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little").reshape(len(words), 1024)


def _oracle(clip):
    """(words [16], don't-care count) of one [16, h, w] clip."""
    words, coefs = orc.hash_clips_with_coefs(clip[None])
    return words[0], int((np.abs(coefs[0]) < 1e-6).sum())


def _corpus():
    """The size list: two random clips per size up to 320 x 240 and one above, plus Gaussian-smoothed content for 64 x 64 and 641 x 361; with the oracle's words."""
    if "corpus" not in _CACHE:
        from scipy.ndimage import gaussian_filter

        rng = np.random.default_rng(2024)
        clips = []
        for w, h in SIZES:
            for _ in range(2 if w * h <= 320 * 240 else 1):
                clips.append(rng.integers(0, 256, size=(16, h, w), dtype=np.uint8))
        for w, h in ((64, 64), (641, 361)):
            s = gaussian_filter(rng.standard_normal((16, h, w)), sigma=(2.0, 6.0, 6.0))
            clips.append(((s - s.min()) / (s.max() - s.min()) * 255.0).astype(np.uint8))
        order = rng.permutation(len(clips))
        clips = [clips[i] for i in order]
        want = [_oracle(c) for c in clips]
        for c, (_, dc) in zip(clips, want):
            assert dc == (990 if c.shape[1:] == (1, 1) else 0) or c.shape[1:] in ((64, 64), (361, 641)), (c.shape, dc)
        _CACHE["corpus"] = (clips, np.stack([w for w, _ in want]), np.array([d for _, d in want], np.uint32))
    return _CACHE["corpus"]


def _pack(clips, seed, crops=None, tail=0, even=False):
    """One buffer with irregular gaps (odd offsets unless `even`), frame_stride > w * h on every third clip; `tail` bytes behind the last clip.  Gaps are filled
    with 0xAA: bytes a load may run into must not matter."""
    from vid_dup_finder_lib_amd.engine import CLIP_DTYPE

    rng = np.random.default_rng(seed)
    recs = np.zeros(len(clips), CLIP_DTYPE)
    at = 0 if even else 1
    for i, c in enumerate(clips):
        h, w = c.shape[1:]
        fs = w * h + (int(rng.integers(1, 200)) if i % 3 == 1 else 0)
        recs[i]["offset"], recs[i]["frame_stride"], recs[i]["w"], recs[i]["h"] = at, fs, w, h
        at += 15 * fs + w * h
        if i + 1 < len(clips):
            at += 64 * int(rng.integers(0, 3)) if even else 2 * int(rng.integers(0, 100)) + (at + 1) % 2  # the next offset is odd
    if crops is not None:
        recs["crop"] = crops
    buf = np.full(at + tail, 0xAA, np.uint8)
    for r, c in zip(recs, clips):
        fb = int(r["w"]) * int(r["h"])
        for f in range(16):
            o = int(r["offset"]) + f * int(r["frame_stride"])
            buf[o:o + fb] = c[f].reshape(-1)
    return buf, recs


def _device_call(engine, buf, recs, frames_per_clip=16):
    import torch

    d_buf = torch.empty(len(buf), dtype=torch.uint8, device="cuda")  # exactly buf_bytes
    d_buf.copy_(torch.from_numpy(buf))
    d_out = torch.full((len(recs) * 16,), -1, dtype=torch.int64, device="cuda")
    d_dc = torch.full((len(recs),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    engine.hash_clips_device(d_buf.data_ptr(), len(buf), recs, d_out.data_ptr(), d_dc.data_ptr(), frames_per_clip=frames_per_clip)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint64).reshape(len(recs), 16), d_dc.cpu().numpy().view(np.uint32)


def _host_call(engine, buf, recs, frames_per_clip=16):
    out = np.zeros((len(recs), 16), np.uint64)
    dc = np.zeros(len(recs), np.uint32)
    engine._check(engine.lib.vdf_hash_clips_u8(engine.ctx, buf.ctypes.data, buf.size, recs.ctypes.data, len(recs), frames_per_clip, out.ctypes.data, dc.ctypes.data))
    return out, dc


def _same(got, dc, want, want_dc, what=""):
    for i in range(len(want)):
        assert np.array_equal(got[i], want[i]), f"{what} clip {i}: {int((_bits(got[i:i + 1]) != _bits(want[i:i + 1])).sum())} hash bits differ"
    assert (_bits(got)[:, 1000:] == 0).all(), "padding bits"
    assert np.array_equal(dc, want_dc), f"{what} don't-care counts {dc} vs {want_dc}"


def test_1_whole_size_list_in_one_device_call(engine):
    clips, want, want_dc = _corpus()
    buf, recs = _pack(clips, 1, tail=333)
    assert (recs["offset"] % 2 == 1).all() and (recs["frame_stride"] > recs["w"].astype(np.uint64) * recs["h"]).sum() >= len(clips) // 3
    got, dc = _device_call(engine, buf, recs)
    _same(got, dc, want, want_dc, "device")


def test_2_host_entry_gives_the_same_words(engine):
    clips, want, want_dc = _corpus()
    buf, recs = _pack(clips, 2, tail=0)
    got, dc = _host_call(engine, buf, recs)
    _same(got, dc, want, want_dc, "host")
    # ... and Engine.hash_clips / hash_frame_stacks on the list of stacks
    import vid_dup_finder_lib_amd as vdf

    got2, dc2 = engine.hash_clips(clips, want_dontcare=True)
    _same(got2, dc2, want, want_dc, "Engine.hash_clips")
    vhs = vdf.hash_frame_stacks(clips[:5], ["a"] * 5, [1] * 5, engine=engine)
    assert all(np.array_equal(v.hash, want[i]) for i, v in enumerate(vhs))


@pytest.mark.parametrize("size", [(7, 5), (96, 96), (191, 130), (320, 240)])
def test_3_last_clip_ends_on_the_buffers_last_byte(engine, size):
    """The careful loader: a clip of each part as the LAST thing of a buffer allocated to exactly buf_bytes hashes to the words it has mid-buffer (test 1)."""
    clips, want, want_dc = _corpus()
    i = next(k for k, c in enumerate(clips) if c.shape[1:] == (size[1], size[0]))
    j = next(k for k, c in enumerate(clips) if c.shape[1:] == (64, 65))  # company of another size: the call is not the uniform one
    for even in (False, True):
        buf, recs = _pack([clips[j], clips[i]], 3, tail=0, even=even)
        assert int(recs[1]["offset"]) + 15 * int(recs[1]["frame_stride"]) + size[0] * size[1] == len(buf)
        got, dc = _device_call(engine, buf, recs)
        _same(got, dc, want[[j, i]], want_dc[[j, i]], "last clip")


@pytest.mark.parametrize("n,w,h", [(300, 64, 64), (33, 160, 90)])
def test_4_uniform_batches_are_the_uniform_call(engine, n, w, h):
    from vid_dup_finder_lib_amd.engine import CLIP_DTYPE

    rng = np.random.default_rng(n)
    frames = rng.integers(0, 256, size=(n, 16, h, w), dtype=np.uint8)
    want, want_dc = engine.hash_frames(frames, want_dontcare=True)
    recs = np.zeros(n, CLIP_DTYPE)
    recs["offset"], recs["frame_stride"], recs["w"], recs["h"] = np.arange(n, dtype=np.uint64) * np.uint64(16 * w * h), w * h, w, h
    buf = frames.reshape(-1)
    _same(*_device_call(engine, buf, recs), want, want_dc, "uniform device")
    _same(*_host_call(engine, buf, recs), want, want_dc, "uniform host")
    got, dc = engine.hash_clips(list(frames), want_dontcare=True)
    _same(got, dc, want, want_dc, "uniform list")


def test_5_crop_boxes(engine):
    """Six clips of three sizes (one per kernel part) with top / bottom bars, side bars and both equal the oracle's hash of the cropped copies."""
    rng = np.random.default_rng(5)
    clips, crops, want = [], [], []
    for (w, h), kinds in (((96, 96), ("rows", "both")), ((191, 130), ("sides", "both")), ((320, 240), ("rows", "sides"))):
        for kind in kinds:
            c = rng.integers(0, 256, size=(16, h, w), dtype=np.uint8)
            l, r = (w // 7, w // 9 + 1) if kind in ("sides", "both") else (0, 0)
            t, b = (h // 8, h // 6 + 1) if kind in ("rows", "both") else (0, 0)
            clips.append(c)
            crops.append((l, r, t, b))
            want.append(_oracle(np.ascontiguousarray(c[:, t:h - b, l:w - r])))
    crops = np.array(crops, np.uint32)
    want_words, want_dc = np.stack([w for w, _ in want]), np.array([d for _, d in want], np.uint32)
    buf, recs = _pack(clips, 5, crops=crops, tail=17)
    _same(*_device_call(engine, buf, recs), want_words, want_dc, "cropped device")
    _same(*_host_call(engine, buf, recs), want_words, want_dc, "cropped host")
    got, dc = engine.hash_clips(clips, crops=crops, want_dontcare=True)
    _same(got, dc, want_words, want_dc, "cropped list")


def test_6_300_small_clips_land_at_their_own_position(engine):
    rng = np.random.default_rng(6)
    clips = [rng.integers(0, 256, size=(16, h, w), dtype=np.uint8) for w, h in (SMALL_SIZES[i % len(SMALL_SIZES)] for i in range(300))]
    got, dc = engine.hash_clips(clips, want_dontcare=True)
    buf, recs = _pack(clips, 6, tail=5)
    got_d, dc_d = _device_call(engine, buf, recs)
    assert np.array_equal(got, got_d) and np.array_equal(dc, dc_d)
    for i in (0, 17, 299):
        one, one_dc = engine.hash_clips([clips[i]], want_dontcare=True)
        assert np.array_equal(got[i], one[0]) and dc[i] == one_dc[0], i
        w, wdc = _oracle(clips[i])
        assert np.array_equal(got[i], w) and dc[i] == wdc, i
    assert len({g.tobytes() for g in got}) >= 300 - 300 // len(SMALL_SIZES)  # (the 1 x 1 clips differ in one bit at most)


def test_7_every_error_has_its_code_names_its_clip_and_leaves_the_context_usable(engine):
    import vid_dup_finder_lib_amd as vdf

    clips, want, want_dc = _corpus()
    pick = [next(k for k, c in enumerate(clips) if c.shape[1:] == (hh, ww)) for ww, hh in ((64, 64), (320, 240), (17, 33))]
    buf, recs = _pack([clips[k] for k in pick], 7, tail=0)

    def refused(r, code, clip, frames_per_clip=16, nbytes=None, host=False):
        b = buf if nbytes is None else buf[:nbytes]
        with pytest.raises(vdf.VdfError) as ei:
            (_host_call if host else _device_call)(engine, b, r, frames_per_clip)
        assert ei.value.code == code, (ei.value, code)
        if clip is not None:
            assert f"clip {clip}" in str(ei.value), ei.value

    for host in (False, True):
        refused(recs, -1, None, frames_per_clip=15, host=host)              # VDF_E_NOT_ENOUGH_FRAMES
        r = recs.copy(); r[1]["w"] = 0
        refused(r, -2, 1, host=host)                                         # VDF_E_BAD_DIMS
        r = recs.copy(); r[2]["frame_stride"] = 17 * 33 - 1
        refused(r, -5, 2, host=host)                                         # VDF_E_INVAL: frame_stride < w * h
        r = recs.copy(); r[0]["crop"] = (40, 24, 0, 0)
        refused(r, -5, 0, host=host)                                         # a box that leaves no pixels
        refused(recs, -5, 2, nbytes=len(buf) - 1, host=host)                 # offset + 15 * frame_stride + w * h > buf_bytes
        r = recs.copy(); r[1]["offset"] = 2**63
        refused(r, -5, 1, host=host)
        # a rejected call launched nothing, and the context goes on: the same clips, valid
        got, dc = (_host_call if host else _device_call)(engine, buf, recs)
        _same(got, dc, want[pick], want_dc[pick], "after the errors")
