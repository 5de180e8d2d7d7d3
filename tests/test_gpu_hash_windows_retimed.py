"""vdf_hash_windows_u8_retimed[_device] (csrc/dct_hash.hip: dct_hash_windows_retimed_kernel) on the GPU: the hash of every retimed window -
the 16 frames k * stride + (i * num) // den - held word for word, don't-care counts and window count included, against oracle.hash_clip of those frames
gathered into a stack.
  - 16 x 16 read in place, on dword boundaries and at an odd base with odd strides (the byte-read form);
  - 64 x 64, 160 x 90, 300 x 200 and 640 x 360: one size per class of resize route (pinned on the CPU by tests/test_hash_windows_retimed_bindings.py);
  - 3 clips per call; F in {span, span + 1, 47, 48, 49, 64, 65, 100} (40 at 640 x 360) x strides 1, 3, 16, 17, 40 x rates 6/5, 5/4, 3/2, 31/16, 2/1;
  - rates 1/1 and 25/24 equal Engine.hash_windows word for word; the device form on a torch buffer; the host form; n_clips == 0; the error codes;
  - end to end: the corpus of tests/test_align_retimed_host.py hashed on the GPU by hash_frame_windows(rate=...) and aligned by align_retimed(engine, seed=True).
A size's clips are made once, 100 frames long (tests/windowgen.py: noise, a static and a constant stretch - exact zeros and their signs), and every F is
the call on their first F frames at clip_stride = 100 frames; the oracle resizes every frame once (16 x 16 input is copied by the resize) and one window
per size is also hashed by the oracle from the full-size frames."""
import numpy as np
import pytest

import retimedgen
import windowgen
from oracle import vdf_oracle as orc

pytestmark = pytest.mark.gpu

RATES = retimedgen.RATES
STRIDES = (1, 3, 16, 17, 40)
LONG = 100
_CACHE = {}


@pytest.fixture(scope="module")
def eng():
    import vid_dup_finder_lib_amd as vdf

    e = vdf.Engine(0)
    yield e
    e.close()


def _frames_of(span, long):
    return sorted({f for f in (span, span + 1, 47, 48, 49, 64, 65, 100) if span <= f <= long})


def _clips(h, w, long=LONG, n=3):
    """(videos [n, long, h, w], their frames resized by the oracle [n, long, 16, 16], {rate: (words, dontcare) per clip at stride 1}) - made once, left unchanged."""
    key = (h, w, long)
    if key not in _CACHE:
        rng = np.random.default_rng(h * 4099 + w)
        v = np.stack([windowgen.video(rng, long, h, w, lead=(5, 0, 3)[c % 3]) for c in range(n)])
        small = v if (h, w) == (16, 16) else np.stack([np.stack([orc.resize_frame(f) for f in c]) for c in v])
        v.setflags(write=False)
        _CACHE[key] = (v, small, {})
    return _CACHE[key]


def _oracle(h, w, rate, long=LONG):
    v, small, by_rate = _clips(h, w, long)
    if rate not in by_rate:
        by_rate[rate] = [retimedgen.oracle_windows(c, rate) for c in small]
        if (h, w) != (16, 16):  # the shortcut through the resized frames, tied to the reference on the full-size frames
            k = min(2, len(by_rate[rate][1][0]) - 1)
            rc, words, _ = orc.hash_clip(np.ascontiguousarray(v[1, k + retimedgen.taps(rate)]))
            assert rc == 0 and np.array_equal(words, by_rate[rate][1][0][k])
    return by_rate[rate]


def _device_buffer(videos, base=0, frame_pad=0, clip_pad=0):
    """The clips on the device at frame_stride = w h + frame_pad, clip_stride = frames * frame_stride + clip_pad, from byte `base` of the buffer, which ends
    with the last clip: (tensor, frame_stride, clip_stride)."""
    import torch

    n, nf, h, w = videos.shape
    fs = w * h + frame_pad
    cs = nf * fs + clip_pad
    host = np.full(base + n * cs, 0xAA, np.uint8)
    for c in range(n):
        rows = host[base + c * cs:base + c * cs + nf * fs].reshape(nf, fs)
        rows[:, :w * h] = videos[c].reshape(nf, -1)
    return torch.from_numpy(host).cuda(), fs, cs


def _call(eng, d, base, n, f, h, w, fs, cs, stride, rate):
    import torch

    n_win = int(eng.lib.vdf_hash_window_count_retimed(f, stride, rate[0], rate[1]))
    assert n_win == retimedgen.n_windows(f, stride, rate)
    out = torch.full((n, n_win, 16), -1, dtype=torch.int64, device="cuda")
    dc = torch.full((n, n_win), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.hash_windows_retimed_device(d.data_ptr() + base, n, f, w, h, stride, rate, out.data_ptr(), d_dontcare=dc.data_ptr(), frame_stride=fs, clip_stride=cs)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64), dc.cpu().numpy().view(np.uint32)


def _check(eng, h, w, d, base, fs, cs, rates, long=LONG, frames=None, strides=STRIDES):
    calls = 0
    for rate in rates:
        table = _oracle(h, w, rate, long)
        span = retimedgen.span(rate)
        for f in frames or _frames_of(span, long):
            for stride in strides:
                got, dc = _call(eng, d, base, len(table), f, h, w, fs, cs, stride, rate)
                for c, (words, counts) in enumerate(table):
                    want, want_dc = words[0:f - span + 1:stride], counts[0:f - span + 1:stride]
                    assert got.shape[1] == len(want), (rate, f, stride)
                    bad = np.argwhere((got[c] != want).any(axis=1)).reshape(-1)
                    assert len(bad) == 0, f"{h} x {w} rate {rate} F {f} stride {stride} clip {c}: windows {bad[:8].tolist()} differ from the oracle's"
                    assert np.array_equal(dc[c], want_dc), f"{h} x {w} rate {rate} F {f} stride {stride} clip {c}: don't-care counts"
                calls += 1
    return calls


@pytest.mark.parametrize("rate", RATES, ids=[f"{n}_{d}" for n, d in RATES])
def test_16x16_read_in_place_on_dword_boundaries(eng, rate):
    v = _clips(16, 16)[0]
    d, fs, cs = _device_buffer(v)
    assert _check(eng, 16, 16, d, 0, fs, cs, [rate]) == 8 * 5
    zeros = np.concatenate([counts for _, counts in _oracle(16, 16, rate)])
    # no retimed window fits into the static stretch of 17 frames (span >= 19), but among the windows that reach into the static and constant stretches
    # some have 400 coefficients that are exact zeros, of either sign; the noisy ones have none
    assert (zeros >= 400).any() and (zeros == 0).any()


@pytest.mark.parametrize("rate", RATES, ids=[f"{n}_{d}" for n, d in RATES])
def test_16x16_read_by_bytes_at_an_odd_base_and_odd_strides(eng, rate):
    v = _clips(16, 16)[0]
    d, fs, cs = _device_buffer(v, base=1, frame_pad=3, clip_pad=5)
    span = retimedgen.span(rate)
    assert _check(eng, 16, 16, d, 1, fs, cs, [rate], frames=(span, span + 1, 49, 100)) == 4 * 5


@pytest.mark.parametrize("h,w", [(64, 64), (90, 160), (200, 300)], ids=["64x64", "160x90", "300x200"])
def test_one_size_per_resize_route(eng, h, w):
    v = _clips(h, w)[0]
    d, fs, cs = _device_buffer(v)
    assert _check(eng, h, w, d, 0, fs, cs, RATES) == 5 * 8 * 5


def test_640x360_at_40_frames(eng):
    v = _clips(360, 640, long=40)[0]
    d, fs, cs = _device_buffer(v)
    assert _check(eng, 360, 640, d, 0, fs, cs, RATES, long=40, frames=(40,)) == 5 * 5


@pytest.mark.parametrize("f", [48, 64, 65])
def test_64x64_packed_and_at_padded_strides(eng, f):
    """Clips that follow each other without a gap (F a multiple of 16: the resize stage's packed layout; 65: by chunk, with a tail), and the same clips
    at an odd base with padded frame and clip strides."""
    full, small, _ = _clips(64, 64)
    v = np.ascontiguousarray(full[:, :f])
    _CACHE.setdefault((64, 64, f), (v, small[:, :f], {}))  # the first f frames of the 100-frame clips, as clips of their own
    for pads in (dict(), dict(base=1, frame_pad=3, clip_pad=5)):
        d, fs, cs = _device_buffer(v, **pads)
        assert _check(eng, 64, 64, d, pads.get("base", 0), fs, cs, [(6, 5), (2, 1)], long=f, frames=(f,), strides=(1, 17)) == 4


@pytest.mark.parametrize("rate", [(1, 1), (25, 24), (65535, 65535)])
def test_rates_whose_taps_are_plain_equal_hash_windows_word_for_word(eng, rate):
    import torch

    for (h, w), f in (((16, 16), 40), ((64, 64), 49)):
        v = np.ascontiguousarray(_clips(h, w)[0][:, :f])
        for stride in (1, 3, 17):
            want, want_dc = eng.hash_windows(v, stride, want_dontcare=True)
            got, dc = eng.hash_windows_retimed(v, rate, stride, want_dontcare=True)
            assert got.shape == want.shape == (3, (f - 16) // stride + 1, 16) and np.array_equal(got, want) and np.array_equal(dc, want_dc)
            d = torch.from_numpy(v).cuda()
            dev, dev_dc = _call(eng, d, 0, 3, f, h, w, h * w, f * h * w, stride, rate)
            assert np.array_equal(dev, want) and np.array_equal(dev_dc, want_dc)


def test_host_form_and_hash_frame_windows(eng):
    import vid_dup_finder_lib_amd as vdf

    rate, f = (3, 2), 49
    v = np.ascontiguousarray(_clips(90, 160)[0][:, :f])
    table = _oracle(90, 160, rate)
    got, dc = eng.hash_windows_retimed(v, rate, 3, want_dontcare=True)
    assert got.shape == (3, 9, 16)
    for c in range(3):
        assert np.array_equal(got[c], table[c][0][0:f - 23 + 1:3]) and np.array_equal(dc[c], table[c][1][0:f - 23 + 1:3])
    windows = vdf.hash_frame_windows(v, ["a", "b", "c"], [1, 2, 3], stride=3, engine=eng, rate=rate)
    assert [len(ws) for ws in windows] == [9, 9, 9] and all(np.array_equal(windows[c][k].hash, got[c, k]) for c in range(3) for k in range(9))
    stacks = vdf.hash_frame_windows([v[0], v[1, :30]], ["a", "b"], [1, 2], stride=3, engine=eng, rate=rate)
    assert [len(ws) for ws in stacks] == [9, 3] and all(np.array_equal(stacks[1][k].hash, got[1, k]) for k in range(3))
    with pytest.raises(vdf.NotEnoughFrames):
        vdf.hash_frame_windows(v[:, :22], ["a", "b", "c"], [1, 2, 3], engine=eng, rate=rate)


def test_no_clips_and_the_error_codes_in_their_order(eng):
    import torch

    import vid_dup_finder_lib_amd as vdf

    multi = None
    try:
        d = torch.zeros(64 * 256, dtype=torch.uint8, device="cuda")
        out = torch.zeros((64, 16), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        live = eng.lib.vdf_live_device_bytes()
        call = eng.lib.vdf_hash_windows_u8_retimed_device
        p, o = d.data_ptr(), out.data_ptr()
        last = lambda e=eng: e.lib.vdf_last_error(e.ctx).decode()
        # the plain call's checks first, in its order - each line breaks one more rule than the one it reports
        assert call(eng.ctx, None, 1, 15, 0, 16, 1, 4096, 0, 5, 2, None, None, None) == -1       # frames_per_clip < 16
        assert call(eng.ctx, None, 1, 16, 0, 16, 1, 4096, 0, 5, 2, None, None, None) == -2       # a zero dimension
        assert call(eng.ctx, None, 1, 16, 16, 16, 255, 4096, 0, 5, 2, None, None, None) == -5 and "frame_stride" in last()
        assert call(eng.ctx, None, 1, 16, 16, 16, 256, 4096, 0, 5, 2, None, None, None) == -5 and "window_stride" in last()
        assert call(eng.ctx, None, 1, 40, 16, 16, 256, 0, 1, 2, 1, o, None, None) == -5 and "null" in last()   # a null pointer, before the rate
        assert call(eng.ctx, None, 1, 40, 16, 16, 256, 0, 1, 5, 2, o, None, None) == -5 and "null" in last()
        # then the rate, then the span
        for num, den in ((5, 2), (4, 5), (3, 0), (0, 0), (65536, 65536), (65536, 40000)):
            assert call(eng.ctx, p, 1, 20, 16, 16, 256, 0, 1, num, den, o, None, None) == -5 and "rate" in last(), (num, den)
        assert call(eng.ctx, p, 1, 30, 16, 16, 256, 0, 1, 2, 1, o, None, None) == -1 and "spans" in last()      # 16 <= F < span = 31
        assert call(eng.ctx, p, 1, 18, 16, 16, 256, 0, 1, 6, 5, o, None, None) == -1
        # no clips: nothing to do, even with null pointers - but the arguments are still checked
        assert call(eng.ctx, None, 0, 40, 16, 16, 256, 0, 1, 2, 1, None, None, None) == 0
        assert call(eng.ctx, None, 0, 40, 16, 16, 256, 0, 1, 5, 2, None, None, None) == -5
        assert call(eng.ctx, None, 0, 30, 16, 16, 256, 0, 1, 2, 1, None, None, None) == -1
        assert eng.hash_windows_retimed(np.zeros((0, 40, 16, 16), np.uint8), (2, 1)).shape == (0, 10, 16)
        torch.cuda.synchronize()
        assert eng.lib.vdf_live_device_bytes() == live  # nothing was allocated, so nothing was launched
        multi = vdf.Engine(devices=[0, 0])
        assert call(multi.ctx, p, 1, 40, 16, 16, 256, 0, 1, 2, 1, o, None, None) == -5 and "single-device" in last(multi)
        with pytest.raises(vdf.VdfError) as ei:
            multi.hash_windows_retimed(np.zeros((1, 40, 16, 16), np.uint8), (2, 1))
        assert ei.value.code == -5
        for bad, code in (((5, 2), -5), ((2, 1), -1)):
            with pytest.raises(vdf.VdfError) as ei:
                eng.hash_windows_retimed(np.zeros((1, 30, 16, 16), np.uint8), bad)
            assert ei.value.code == code
    finally:
        if multi is not None:
            multi.close()


@pytest.mark.parametrize("rate", [(6, 5), (3, 2), (2, 1)], ids=["6_5", "3_2", "2_1"])
def test_end_to_end_hash_on_the_gpu_then_align_retimed_seeded(eng, rate):
    import vid_dup_finder_lib_amd as vdf
    from test_align_retimed_host import SEED, hashed

    A, B = retimedgen.corpus(rate, SEED[rate])
    wa = vdf.hash_frame_windows(A, ["a0", "a1"], [10, 11], engine=eng, rate=rate)
    wb = vdf.hash_frame_windows(B, [f"b{i}" for i in range(4)], [10, 11, 12, 13], engine=eng)
    _, _, _, oa, ob = hashed(rate)
    assert all(np.array_equal(np.stack([h.hash for h in ws]), o) for ws, o in zip(wa, oa)), "retimed windows differ from the oracle's"
    assert all(np.array_equal(np.stack([h.hash for h in ws]), o) for ws, o in zip(wb, ob))
    for tolerance, min_run in ((0.35, 2), (0.0, 2)):
        got = vdf.align_retimed(wa, wb, rate, tolerance, min_run=min_run, engine=eng, seed=True)
        want = retimedgen.align_retimed_twin(oa, ob, rate, vdf.engine.tolerance_int(tolerance), min_run)
        assert [tuple(r[:10]) for r in got] == want and len(got) >= 4
        assert got == vdf.align_retimed(wa, wb, rate, tolerance, min_run=min_run)  # the host forms on the same hashes
