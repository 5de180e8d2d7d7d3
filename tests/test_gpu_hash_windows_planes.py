"""vdf_hash_windows_u8_planes[_device] (csrc/dct_hash.hip: dct_hash_windows_kernel<DWORDS, true>): the zero plane of every
16-frame window beside its hash.  Per case
  - hashes and don't-care counts equal the plain windows call's (hash_windows_device) on the same buffer, bit for bit;
  - the planes equal the oracle's `coefs == 0.0` planes of each window's 16 frames;
  - the planes equal vdf_hash_frames_u8_planes_device's at clip_stride = stride * frame_stride;
  - H & Z == 0;
  - the output buffers are pre-filled with -1 and carry 64 guard words behind them, which stay -1.
Cases as tests/test_gpu_hash_windows.py: its GEOMETRY at 16 x 16 (windows across a segment boundary among them), 300 clips of seven kinds, one
row per resize route packed and at an odd base with padded strides, the host form, the error codes in their order."""
import numpy as np
import pytest

import planegen
import windowgen
from test_gpu_hash_planes import ROWS
from test_gpu_hash_windows import GEOMETRY, SEG_FRAMES, _engine

pytestmark = pytest.mark.gpu

GUARD = 64
_CACHE = {}


def _videos(key, n, n_frames, h, w, leads):
    """(videos, {stride: oracle planes [n, n_win, 16]}) - made once per key, left unchanged"""
    if key not in _CACHE:
        rng = np.random.default_rng(n_frames * 7919 + h * 4099 + w + 1)
        v = np.stack([windowgen.video(rng, n_frames, h, w, lead=leads[c % len(leads)]) for c in range(n)])
        v.setflags(write=False)
        _CACHE[key] = (v, {})
    return _CACHE[key][0]


def _oracle_planes(key, stride):
    v, by_stride = _CACHE[key]
    if stride not in by_stride:
        n_win = windowgen.n_windows(v.shape[1], stride)
        by_stride[stride] = np.stack([np.stack([planegen.oracle_planes(c[k * stride:k * stride + 16])[1] for k in range(n_win)]) for c in v])
    return by_stride[stride]


def _guarded(n_words, dtype):
    import torch

    return torch.full((n_words + GUARD,), -1, dtype=dtype, device="cuda")


def _run(eng, videos, stride, base=0, frame_pad=0, clip_pad=0):
    """-> planes call (hashes, zero, dontcare), plain windows call (hashes, dontcare), plain planes call at clip_stride = stride * frame_stride (zero)"""
    import torch

    n, nf, h, w = videos.shape
    fs = w * h + frame_pad
    cs = nf * fs + clip_pad
    n_win = windowgen.n_windows(nf, stride)
    host = np.full(base + n * cs, 0xAA, np.uint8)
    for c in range(n):
        for f in range(nf):
            o = base + c * cs + f * fs
            host[o:o + w * h] = videos[c, f].reshape(-1)
    d = torch.from_numpy(host).cuda()
    nw = n * n_win
    out, zero, plain, clip_out, clip_zero = (_guarded(nw * 16, torch.int64) for _ in range(5))
    dc, plain_dc = (_guarded(nw, torch.int32) for _ in range(2))
    torch.cuda.synchronize()
    p = d.data_ptr() + base
    eng.hash_windows_planes_device(p, n, nf, w, h, stride, out.data_ptr(), zero.data_ptr(), d_dontcare=dc.data_ptr(), frame_stride=fs, clip_stride=cs)
    eng.hash_windows_device(p, n, nf, w, h, stride, plain.data_ptr(), d_dontcare=plain_dc.data_ptr(), frame_stride=fs, clip_stride=cs)
    for c in range(n):
        eng.hash_frames_planes_device(p + c * cs, n_win, 16, w, h, clip_out.data_ptr() + c * n_win * 128, clip_zero.data_ptr() + c * n_win * 128,
                                      frame_stride=fs, clip_stride=stride * fs)
    torch.cuda.synchronize()
    for name, t, words in (("hashes", out, nw * 16), ("planes", zero, nw * 16), ("don't-care counts", dc, nw)):
        assert bool((t[words:] == -1).all()), f"the guard words behind the {name} were written"

    def u64(t):
        return t[:nw * 16].cpu().numpy().view(np.uint64).reshape(n, n_win, 16)
    return (u64(out), u64(zero), dc[:nw].cpu().numpy().reshape(n, n_win)), (u64(plain), plain_dc[:nw].cpu().numpy().reshape(n, n_win)), u64(clip_zero)


def _check(eng, key, stride, **pads):
    videos = _CACHE[key][0]
    (got, zero, dc), (plain, plain_dc), clip_zero = _run(eng, videos, stride, **pads)
    want = _oracle_planes(key, stride)
    zeros = [[int(np.unpackbits(z.view(np.uint8)).sum()) for z in c] for c in want]
    print(f"{key} stride {stride} {pads}: {want.shape[0]} x {want.shape[1]} windows, exact zeros of clip 0's windows {zeros[0]}")
    assert np.array_equal(got, plain), f"hashes differ from the plain windows call's at {np.argwhere((got != plain).any(axis=2))[:8].tolist()}"
    assert np.array_equal(dc, plain_dc), f"don't-care counts differ from the plain windows call's at {np.argwhere(dc != plain_dc)[:8].tolist()}"
    assert np.array_equal(zero, want), f"planes differ from the oracle's at (clip, k) {np.argwhere((zero != want).any(axis=2))[:8].tolist()}"
    assert np.array_equal(zero, clip_zero), f"planes differ from the plain planes call's at {np.argwhere((zero != clip_zero).any(axis=2))[:8].tolist()}"
    assert not np.any(got & zero)
    return zeros


@pytest.mark.parametrize("n_frames,stride", GEOMETRY, ids=[f"F{f}_s{s}" for f, s in GEOMETRY])
def test_window_geometry_at_16x16(n_frames, stride, monkeypatch):
    key = ("geometry", n_frames)
    _videos(key, 1, n_frames, 16, 16, leads=(5,))
    eng = _engine({}, monkeypatch)
    try:
        zeros = _check(eng, key, stride)[0]
        if n_frames == 2 * SEG_FRAMES + 1:
            assert len(zeros) > SEG_FRAMES + 1 and 900 in zeros and 999 in zeros and 0 in zeros
    finally:
        eng.close()


def test_many_clips_of_different_kinds_in_one_call(monkeypatch):
    key = ("many", 20)
    _videos(key, 300, 20, 16, 16, leads=(0, 1, 2, 3, 5, 8, 13))
    eng = _engine({}, monkeypatch)
    try:
        zeros = _check(eng, key, 2)
        assert any(900 in z for z in zeros) and any(0 in z for z in zeros)
    finally:
        eng.close()


@pytest.mark.parametrize("layout", ["packed", "odd_base_padded"])
@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_every_resize_route_feeds_the_planes_form(row, layout, monkeypatch):
    route, h, w, env, _kinds = row
    pads = dict(base=0, frame_pad=0, clip_pad=0) if layout == "packed" else dict(base=1, frame_pad=3, clip_pad=5)
    one, two = ("route1", route), ("route2", route)
    _videos(one, 1, 33, h, w, leads=(0,))
    _videos(two, 2, 35, h, w, leads=(0, 5))
    eng = _engine(env, monkeypatch)
    try:
        zeros = _check(eng, one, 1, **pads)[0]
        assert zeros[0] == 900 and zeros[1] == 900 and zeros[17] == 999 and zeros[9] not in (900, 999)
        _check(eng, two, 5, **pads)
    finally:
        eng.close()


def test_host_form_equals_the_device_form(monkeypatch):
    import vid_dup_finder_lib_amd as vdf

    key = ("host", 35)
    videos = _videos(key, 2, 35, 36, 48, leads=(0, 5))
    eng = _engine({}, monkeypatch)
    try:
        got, zero, dc = eng.hash_windows_planes(videos, 5, want_dontcare=True)
        (dev, dev_zero, dev_dc), _, _ = _run(eng, videos, 5)
        assert got.shape == (2, 4, 16) and np.array_equal(got, dev) and np.array_equal(zero, dev_zero) and np.array_equal(dc, dev_dc)
        assert np.array_equal(zero, _oracle_planes(key, 5))
        windows = vdf.hash_frame_windows(videos, ["a", "b"], [1, 2], stride=5, engine=eng, zero_plane=True)
        assert all(np.array_equal(windows[c][k].hash, got[c, k]) and np.array_equal(windows[c][k].zero, zero[c, k]) for c in range(2) for k in range(4))
        assert vdf.hash_frame_windows(videos, ["a", "b"], [1, 2], stride=5, engine=eng)[0][0].zero is None
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
        zero = torch.zeros((64, 16), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        live = eng.lib.vdf_live_device_bytes()
        call = eng.lib.vdf_hash_windows_u8_planes_device
        p, o, z = d.data_ptr(), out.data_ptr(), zero.data_ptr()
        # the plain windows call's checks in its order; each line breaks one more rule than the one it reports
        assert call(eng.ctx, None, 1, 15, 0, 16, 1, 4096, 0, None, None, None, None) == -1      # frames_per_clip < 16
        assert call(eng.ctx, None, 1, 16, 0, 16, 1, 4096, 0, None, None, None, None) == -2      # a zero dimension
        assert call(eng.ctx, None, 1, 16, 16, 16, 255, 4096, 0, None, None, None, None) == -5   # frame_stride < w * h
        assert "frame_stride" in eng.lib.vdf_last_error(eng.ctx).decode()
        assert call(eng.ctx, None, 1, 16, 16, 16, 256, 4096, 0, None, None, None, None) == -5   # window_stride == 0
        assert "window_stride" in eng.lib.vdf_last_error(eng.ctx).decode()
        assert call(eng.ctx, None, 2**32 // 17 + 1, 32, 16, 16, 256, 0, 1, None, None, None, None) == -5
        assert "2^32" in eng.lib.vdf_last_error(eng.ctx).decode()
        assert call(eng.ctx, None, 0, 32, 16, 16, 256, 0, 1, None, None, None, None) == 0       # no clips
        for args in ((None, o, z), (p, None, z), (p, o, None)):                                 # a null out_zero is among the null pointers
            assert call(eng.ctx, args[0], 1, 32, 16, 16, 256, 0, 1, args[1], None, args[2], None) == -5
            assert "null" in eng.lib.vdf_last_error(eng.ctx).decode()
        torch.cuda.synchronize()
        assert eng.lib.vdf_live_device_bytes() == live  # nothing was allocated, so nothing was launched
        multi = vdf.Engine(devices=[0, 0])
        live = eng.lib.vdf_live_device_bytes()
        assert call(multi.ctx, p, 1, 32, 16, 16, 256, 0, 1, o, None, None, None) == -5 and "null" in multi.lib.vdf_last_error(multi.ctx).decode()
        assert call(multi.ctx, p, 1, 32, 16, 16, 256, 0, 1, o, None, z, None) == -5             # a multi-GPU context: the last check
        assert "single-device" in multi.lib.vdf_last_error(multi.ctx).decode()
        with pytest.raises(vdf.VdfError) as ei:
            multi.hash_windows_planes(np.zeros((1, 20, 16, 16), np.uint8))
        assert ei.value.code == -5
        with pytest.raises(vdf.NotEnoughFrames):
            vdf.hash_frame_windows(np.zeros((1, 15, 16, 16), np.uint8), ["a"], [1], engine=eng, zero_plane=True)
        torch.cuda.synchronize()
        assert eng.lib.vdf_live_device_bytes() == live
    finally:
        eng.close()
        if multi is not None:
            multi.close()
