"""vdf_hash_windows_u8[_device] (csrc/dct_hash.hip: dct_hash_windows_kernel): the hash of EVERY 16-frame window of a clip from one read of its
frames, held word for word - nothing masked - against both yardsticks that existed before it:
  - oracle.hash_clip of each window's 16 frames;
  - the plain call (hash_frames_device) on the same buffer with clip_stride = stride * frame_stride: hashes and don't-care counts equal.
The videos (tests/windowgen.py) are tests/planegen.py pieces concatenated in time - noise, a static stretch of 17 frames, a constant stretch, noise - so some
windows are entirely static (900 exact zeros), some entirely constant (999) and some straddle a boundary.
Cases: the window geometry at 16 x 16 (the smallest input that runs the whole kernel), one clip longer than twice the planner's segment so that windows
straddle segments, 300 clips of seven kinds (300 workgroups: more than the CUs, but all resident at once at three per CU - neighbours of different kinds, not turns
through one LDS; a workgroup's own windows take turns through its ballot words in every case above), one row per resize route the call
can take - packed, and at an odd base address with padded strides - the host form, locate(), and the error codes in their order."""
import os
import re

import numpy as np
import pytest

import windowgen
from test_gpu_hash_planes import ROWS  # one row per resize route: sizes and knobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG_FRAMES = 16 * int(re.search(r"kWindowSegChunks = (\d+);", open(os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc", "windows_plan.h")).read()).group(1))
GEOMETRY = [(16, 1), (17, 1), (31, 1), (32, 1), (33, 1), (48, 3), (40, 7), (50, 16), (60, 17), (100, 40), (2 * SEG_FRAMES + 1, 1)]
_CACHE = {}


def _engine(env, monkeypatch):
    """A fresh context under env (the knobs are read once, when the context is made)."""
    import vid_dup_finder_lib_amd as vdf

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return vdf.Engine(0)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _videos(key, n, n_frames, h, w, leads):
    """(videos [n, F, h, w], per stride {stride: (oracle hashes [n, n_win, 16], exact zeros per window)}) - made once per key, left unchanged."""
    if key not in _CACHE:
        rng = np.random.default_rng(n_frames * 7919 + h * 4099 + w)
        v = np.stack([windowgen.video(rng, n_frames, h, w, lead=leads[c % len(leads)]) for c in range(n)])
        v.setflags(write=False)
        _CACHE[key] = (v, {})
    return _CACHE[key]


def _oracle(key, stride):
    v, by_stride = _CACHE[key]
    if stride not in by_stride:
        per = [windowgen.oracle_windows(c, stride) for c in v]
        by_stride[stride] = (np.stack([p[0] for p in per]), [p[1] for p in per])
    return by_stride[stride]


def _run(eng, videos, stride, base=0, frame_pad=0, clip_pad=0):
    """The windows call and, clip by clip, the plain call at clip_stride = stride * frame_stride on the same device buffer -> (hashes, dontcare) of each."""
    import torch

    n, nf, h, w = videos.shape
    fs = w * h + frame_pad
    cs = nf * fs + clip_pad
    n_win = windowgen.n_windows(nf, stride)
    host = np.full(base + n * cs, 0xAA, np.uint8)  # ends at the last frame's last byte plus its padding: no load of a kernel can leave it
    for c in range(n):
        for f in range(nf):
            o = base + c * cs + f * fs
            host[o:o + w * h] = videos[c, f].reshape(-1)
    d = torch.from_numpy(host).cuda()
    outs = [torch.full((n, n_win, 16), -1, dtype=torch.int64, device="cuda") for _ in range(2)]
    dcs = [torch.full((n, n_win), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    eng.hash_windows_device(d.data_ptr() + base, n, nf, w, h, stride, outs[0].data_ptr(), d_dontcare=dcs[0].data_ptr(), frame_stride=fs, clip_stride=cs)
    for c in range(n):
        eng.hash_frames_device(d.data_ptr() + base + c * cs, n_win, 16, w, h, outs[1][c].data_ptr(), d_dontcare=dcs[1][c].data_ptr(), frame_stride=fs,
                               clip_stride=stride * fs)
    torch.cuda.synchronize()
    return _u64(outs[0]), dcs[0].cpu().numpy(), _u64(outs[1]), dcs[1].cpu().numpy()


def _check(eng, key, stride, **pads):
    videos = _CACHE[key][0]
    want, zeros = _oracle(key, stride)
    got, dc, plain, plain_dc = _run(eng, videos, stride, **pads)
    print(f"{key} stride {stride} {pads}: {want.shape[0]} x {want.shape[1]} windows, exact zeros of clip 0's windows {zeros[0]}")
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, f"windows (clip, k) {bad[:8].tolist()} ... differ from the oracle's"
    bad = np.argwhere((got != plain).any(axis=2))
    assert len(bad) == 0, f"windows (clip, k) {bad[:8].tolist()} ... differ from the plain call's"
    assert np.array_equal(dc, plain_dc), f"dontcare differs from the plain call's at {np.argwhere(dc != plain_dc)[:8].tolist()}"
    return zeros


@pytest.mark.parametrize("n_frames,stride", GEOMETRY, ids=[f"F{f}_s{s}" for f, s in GEOMETRY])
def test_window_geometry_at_16x16(n_frames, stride, monkeypatch):
    key = ("geometry", n_frames)
    _videos(key, 1, n_frames, 16, 16, leads=(5,))
    eng = _engine({}, monkeypatch)
    try:
        zeros = _check(eng, key, stride)[0]
        if n_frames == 2 * SEG_FRAMES + 1:  # windows on both sides of a segment boundary, and every kind of window
            assert len(zeros) > SEG_FRAMES + 1 and 900 in zeros and 999 in zeros and 0 in zeros
    finally:
        eng.close()


def test_many_clips_of_different_kinds_in_one_call(monkeypatch):
    key = ("many", 20)
    _videos(key, 300, 20, 16, 16, leads=(0, 1, 2, 3, 5, 8, 13))  # seven kinds of clip: windows static, straddling and noisy in turn
    eng = _engine({}, monkeypatch)
    try:
        zeros = _check(eng, key, 2)
        assert any(900 in z for z in zeros) and any(0 in z for z in zeros)
    finally:
        eng.close()


@pytest.mark.parametrize("layout", ["packed", "odd_base_padded"])
@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_every_resize_route_feeds_the_windows_kernel(row, layout, monkeypatch):
    """ROWS of tests/test_gpu_hash_planes.py: the direct row reads the caller's frames, the three fused-class sizes must arrive at an unfused route here.
    Which route each run of each row reaches is pinned on the CPU by tests/test_hash_windows_routes.py (same rows, layouts, frame and clip counts)."""
    route, h, w, env, _kinds = row
    pads = dict(base=0, frame_pad=0, clip_pad=0) if layout == "packed" else dict(base=1, frame_pad=3, clip_pad=5)
    one, two = ("route1", route), ("route2", route)
    _videos(one, 1, 33, h, w, leads=(0,))      # static 0..16, constant 17..32: windows 0 and 1 static, 17 constant, the rest straddle
    _videos(two, 2, 35, h, w, leads=(0, 5))
    eng = _engine(env, monkeypatch)
    try:
        zeros = _check(eng, one, 1, **pads)[0]
        assert zeros[0] == 900 and zeros[1] == 900 and zeros[17] == 999 and zeros[9] not in (900, 999)  # (window 9 straddles the two stretches)
        _check(eng, two, 5, **pads)
    finally:
        eng.close()


def test_host_form_equals_the_device_form(monkeypatch):
    key = ("host", 35)
    videos = _videos(key, 2, 35, 36, 48, leads=(0, 5))[0]
    eng = _engine({}, monkeypatch)
    try:
        got, dc = eng.hash_windows(videos, 5, want_dontcare=True)
        dev, dev_dc, _, _ = _run(eng, videos, 5)
        assert got.shape == (2, 4, 16) and np.array_equal(got, dev) and np.array_equal(dc, dev_dc)
        assert np.array_equal(got, _oracle(key, 5)[0])
    finally:
        eng.close()


def test_locate_finds_a_clip_cut_out_of_a_longer_video(monkeypatch):
    import vid_dup_finder_lib_amd as vdf
    from oracle import vdf_oracle as orc

    rng = np.random.default_rng(23)
    videos = rng.integers(0, 256, size=(3, 48, 32, 32), dtype=np.uint8)
    eng = _engine({}, monkeypatch)
    try:
        windows = vdf.hash_frame_windows(videos, ["a", "b", "c"], [60, 70, 80], stride=1, engine=eng)
        assert [len(w) for w in windows] == [33, 33, 33] and windows[2][4].src_path() == "c" and windows[1][0].duration() == 70
        needle = vdf.hash_frame_stacks(np.ascontiguousarray(videos[2:3, 23:39]), ["needle"], [1], engine=eng)[0]  # the plain hash of frames 23 .. 38 of video 2
        assert vdf.locate([needle], windows, 0.0, stride=1, engine=eng) == [[(2, 23, 0)]]
        # the default tolerance: what the oracle's reference search gives on the oracle's window hashes with zero durations
        want_words = np.concatenate([windowgen.oracle_windows(v, 1)[0] for v in videos])
        rc, needle_words, _ = orc.hash_clip(videos[2, 23:39])
        assert rc == 0 and np.array_equal(needle.hash, needle_words)
        zeros = np.zeros(len(want_words), np.uint32)
        res = orc.search_refs_sorted(want_words, zeros, needle_words[None], np.zeros(1, np.uint32), orc.tolerance_int(vdf.DEFAULT_SEARCH_TOLERANCE))
        want = sorted((m // 33, m % 33, orc.hamming(needle_words, want_words[m])) for r, ms in res for m in ms)
        got = vdf.locate([needle], windows, vdf.DEFAULT_SEARCH_TOLERANCE, stride=1, engine=eng)
        assert got == [want] and (2, 23, 0) in want
    finally:
        eng.close()


def test_error_codes_in_their_order_with_nothing_launched(monkeypatch):
    import torch

    import vid_dup_finder_lib_amd as vdf

    eng = _engine({}, monkeypatch)
    multi = None
    try:
        d = torch.zeros(64 * 256, dtype=torch.uint8, device="cuda")
        out = torch.zeros((64, 16), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        live = eng.lib.vdf_live_device_bytes()
        call = eng.lib.vdf_hash_windows_u8_device
        p, o = d.data_ptr(), out.data_ptr()
        # each line breaks one more rule than the one it reports: the earlier check wins
        assert call(eng.ctx, None, 1, 15, 0, 16, 1, 4096, 0, None, None, None) == -1      # frames_per_clip < 16 (and a zero dimension, ...)
        assert call(eng.ctx, None, 1, 16, 0, 16, 1, 4096, 0, None, None, None) == -2      # a zero dimension (and frame_stride < w * h, ...)
        assert call(eng.ctx, None, 1, 16, 16, 16, 255, 4096, 0, None, None, None) == -5   # frame_stride < w * h
        assert "frame_stride" in eng.lib.vdf_last_error(eng.ctx).decode()
        assert call(eng.ctx, None, 1, 16, 16, 16, 256, 4096, 0, None, None, None) == -5   # window_stride == 0
        assert "window_stride" in eng.lib.vdf_last_error(eng.ctx).decode()
        assert call(eng.ctx, None, 2**32 // 17 + 1, 32, 16, 16, 256, 0, 1, None, None, None) == -5  # n_clips * n_win >= 2^32 (17 windows per clip)
        assert "2^32" in eng.lib.vdf_last_error(eng.ctx).decode()
        assert call(eng.ctx, None, 0, 32, 16, 16, 256, 0, 1, None, None, None) == 0       # no clips: nothing to do, even with null pointers
        assert call(eng.ctx, None, 1, 32, 16, 16, 256, 0, 1, o, None, None) == -5         # a null pointer
        assert call(eng.ctx, p, 1, 32, 16, 16, 256, 0, 1, None, None, None) == -5
        assert "null" in eng.lib.vdf_last_error(eng.ctx).decode()
        torch.cuda.synchronize()
        assert eng.lib.vdf_live_device_bytes() == live  # nothing was allocated, so nothing was launched
        multi = vdf.Engine(devices=[0, 0])
        live = eng.lib.vdf_live_device_bytes()
        assert call(multi.ctx, None, 1, 32, 16, 16, 256, 0, 1, None, None, None) == -5 and "null" in multi.lib.vdf_last_error(multi.ctx).decode()
        assert call(multi.ctx, p, 1, 32, 16, 16, 256, 0, 1, o, None, None) == -5          # a multi-GPU context: the last check
        assert "single-device" in multi.lib.vdf_last_error(multi.ctx).decode()
        with pytest.raises(vdf.VdfError) as ei:
            multi.hash_windows(np.zeros((1, 20, 16, 16), np.uint8))
        assert ei.value.code == -5
        with pytest.raises(vdf.NotEnoughFrames):
            vdf.hash_frame_windows(np.zeros((1, 15, 16, 16), np.uint8), ["a"], [1], engine=eng)
        torch.cuda.synchronize()
        assert eng.lib.vdf_live_device_bytes() == live  # nothing was allocated, so nothing was launched
    finally:
        eng.close()
        if multi is not None:
            multi.close()
