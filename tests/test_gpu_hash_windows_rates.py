"""vdf_hash_windows_u8_rates[_device] (csrc/dct_hash.hip: dct_hash_windows_rates_kernel) on the GPU: the retimed windows of a clip at
several rates from one read of its frames.  Block r of the rate-major outputs is held, word for word and count for count, against ONE
vdf_hash_windows_u8_retimed_device call at rate r on the same buffer, and at 16 x 16 against the oracle on the gathered frames as well.
  - 16 x 16 read in place on dword boundaries, and at an odd base with odd strides (the byte-read form);
  - 3 clips per call; F in 31, 32, 47, 49, 65, 100 x strides 1, 3, 16, 17, 40 x the lists [1/1, 2/1], [2/1], the five usual rates, eight rates with a
    duplicate and an unreduced one;
  - F = 47: a span of 31 behind a first chunk of 16 frames; F = 49, stride 1: 2/1 owns no window in the last segment;
  - 64 x 64, 160 x 90, 300 x 200 and 640 x 360 x 40 frames: one size per class of resize route, the five rates;
  - the host form; hash_frame_windows(rates=); n_clips == 0; the error codes in their order;
  - end to end on retimedgen.corpus: hash_frame_windows(rates=) -> align_rates(native=True, seed=True) -> best_rates names the true rate at distance 0.
The clips, their device buffers' layout, the oracle's tables and the single-rate call are those of tests/test_gpu_hash_windows_retimed.py, made once."""
import ctypes as C

import numpy as np
import pytest

import retimedgen
from test_gpu_hash_windows_retimed import _call, _clips, _device_buffer, _oracle

pytestmark = pytest.mark.gpu

FIVE = [(1, 1), (6, 5), (5, 4), (3, 2), (2, 1)]
EIGHT = [(2, 1), (1, 1), (6, 5), (3, 2), (5, 4), (12, 10), (31, 16), (2, 1)]  # 12/10 is 6/5 unreduced, 2/1 is listed twice
LISTS = {"1_1+2_1": [(1, 1), (2, 1)], "2_1": [(2, 1)], "five": FIVE, "eight": EIGHT}
FRAMES = (31, 32, 47, 49, 65, 100)
STRIDES = (1, 3, 16, 17, 40)


@pytest.fixture(scope="module")
def eng():
    import vid_dup_finder_lib_amd as vdf

    e = vdf.Engine(0)
    yield e
    e.close()


def _rates_call(eng, d, base, n, f, h, w, fs, cs, stride, rates):
    """the new device call -> [(words [n, n_win_r, 16], counts [n, n_win_r]) per rate]; every row is pre-filled with ones and must be written"""
    import torch

    import vid_dup_finder_lib_amd as vdf

    total, first = vdf.hash_window_count_rates(n, f, stride, rates)
    assert first.tolist() == np.concatenate([[0], np.cumsum([n * retimedgen.n_windows(f, stride, r) for r in rates])]).tolist() and total == first[-1]
    out = torch.full((total, 16), -1, dtype=torch.int64, device="cuda")
    dc = torch.full((total,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    got_first = eng.hash_windows_rates_device(d.data_ptr() + base, n, f, w, h, stride, rates, out.data_ptr(), d_dontcare=dc.data_ptr(), frame_stride=fs,
                                              clip_stride=cs)
    torch.cuda.synchronize()
    assert got_first.tolist() == first.tolist()
    words, counts = out.cpu().numpy().view(np.uint64), dc.cpu().numpy().view(np.uint32)
    return [(words[first[r]:first[r + 1]].reshape(n, -1, 16), counts[first[r]:first[r + 1]].reshape(n, -1)) for r in range(len(rates))]


def _check(eng, h, w, d, base, fs, cs, rates, frames, strides, n=3, oracle=False, long=100):
    single = {}
    for f in frames:
        for stride in strides:
            blocks = _rates_call(eng, d, base, n, f, h, w, fs, cs, stride, rates)
            for rate, (got, dc) in zip(rates, blocks):
                if rate not in single:  # (a duplicate rate is held against the same call)
                    single[rate] = _call(eng, d, base, n, f, h, w, fs, cs, stride, rate)
                want, want_dc = single[rate]
                assert got.shape == want.shape and got.shape[1] == retimedgen.n_windows(f, stride, rate)
                bad = np.argwhere((got != want).any(axis=2))
                assert len(bad) == 0, f"{h} x {w} F {f} stride {stride} rates {rates}: (clip, window) {bad[:8].tolist()} of rate {rate} differ from the single-rate call's"
                assert np.array_equal(dc, want_dc), f"{h} x {w} F {f} stride {stride} rates {rates}: don't-care counts of rate {rate}"
                if oracle:
                    span = retimedgen.span(rate)
                    for c, (words, counts) in enumerate(_oracle(h, w, rate, long)):
                        assert np.array_equal(got[c], words[0:f - span + 1:stride]) and np.array_equal(dc[c], counts[0:f - span + 1:stride]), (f, stride, rate, c)
            single.clear()


@pytest.mark.parametrize("name", list(LISTS))
def test_16x16_read_in_place_on_dword_boundaries(eng, name):
    d, fs, cs = _device_buffer(_clips(16, 16)[0])
    _check(eng, 16, 16, d, 0, fs, cs, LISTS[name], FRAMES, STRIDES, oracle=name in ("five", "1_1+2_1"))


@pytest.mark.parametrize("name", ["1_1+2_1", "five"])
def test_16x16_read_by_bytes_at_an_odd_base_and_odd_strides(eng, name):
    d, fs, cs = _device_buffer(_clips(16, 16)[0], base=1, frame_pad=3, clip_pad=5)
    _check(eng, 16, 16, d, 1, fs, cs, LISTS[name], (31, 47, 49, 100), (1, 17), oracle=True)


def test_a_long_span_behind_the_first_chunk_and_a_last_segment_it_owns_nothing_of(eng):
    """F = 47, stride 1: after the first chunk have = 16 < span = 31, and the 2/1 windows must wait for the second; F = 49: 34 plain windows are two
    segments, the 19 windows of 2/1 all start in the first - the second segment walks frames 32 ... 48 for the plain windows alone."""
    assert retimedgen.n_windows(49, 1, (2, 1)) == 19 <= 32 < retimedgen.n_windows(49, 1, (1, 1)) == 34
    d, fs, cs = _device_buffer(_clips(16, 16)[0])
    for rates in ([(1, 1), (2, 1)], [(2, 1), (1, 1)], [(2, 1), (31, 16), (1, 1)]):
        _check(eng, 16, 16, d, 0, fs, cs, rates, (47, 49), (1,), oracle=True)


@pytest.mark.parametrize("h,w", [(64, 64), (90, 160), (200, 300)], ids=["64x64", "160x90", "300x200"])
def test_one_size_per_resize_route(eng, h, w):
    d, fs, cs = _device_buffer(_clips(h, w)[0])
    _check(eng, h, w, d, 0, fs, cs, FIVE, (31, 49, 64, 100), (1, 17))


def test_640x360_at_40_frames(eng):
    d, fs, cs = _device_buffer(_clips(360, 640, long=40)[0])
    _check(eng, 360, 640, d, 0, fs, cs, FIVE, (40,), (1, 3))


def test_host_form_and_hash_frame_windows(eng):
    import vid_dup_finder_lib_amd as vdf

    f = 49
    v = np.ascontiguousarray(_clips(90, 160)[0][:, :f])
    words, dc = eng.hash_windows_rates(v, FIVE, 3, dontcare=True)
    only = eng.hash_windows_rates(v, FIVE, 3)
    assert len(words) == len(dc) == len(only) == 5
    for r, rate in enumerate(FIVE):
        want, want_dc = eng.hash_windows_retimed(v, rate, 3, want_dontcare=True)
        assert words[r].shape == (3, retimedgen.n_windows(f, 3, rate), 16) and np.array_equal(words[r], want) and np.array_equal(dc[r], want_dc)
        assert np.array_equal(only[r], want)
    by_rate = vdf.hash_frame_windows(v, ["a", "b", "c"], [1, 2, 3], stride=3, engine=eng, rates=FIVE)
    assert list(by_rate) == FIVE
    for r, rate in enumerate(FIVE):
        ws = by_rate[rate]
        assert [len(x) for x in ws] == [words[r].shape[1]] * 3 and all(np.array_equal(ws[c][k].hash, words[r][c, k]) for c in range(3) for k in range(len(ws[c])))
        assert ws[1][0].src_path() == "b" and ws[2][0].duration() == 3
    stacks = vdf.hash_frame_windows([v[0], v[1, :34]], ["a", "b"], [1, 2], stride=3, engine=eng, rates=[(2, 1), (1, 1)])
    assert [len(x) for x in stacks[(2, 1)]] == [7, 2] and [len(x) for x in stacks[(1, 1)]] == [12, 7]
    assert all(np.array_equal(stacks[(2, 1)][1][k].hash, words[4][1, k]) for k in range(2)) and all(np.array_equal(stacks[(1, 1)][1][k].hash, words[0][1, k]) for k in range(7))
    with pytest.raises(vdf.NotEnoughFrames):
        vdf.hash_frame_windows(v[:, :30], ["a", "b", "c"], [1, 2, 3], engine=eng, rates=FIVE)
    for bad in (dict(rate=(2, 1)), dict(zero_plane=True), dict(one_call=True), dict(letterbox=True)):
        with pytest.raises(ValueError):
            vdf.hash_frame_windows(v, ["a", "b", "c"], [1, 2, 3], engine=eng, rates=FIVE, **bad)


def _job(frames, n_clips, f, w, h, fs, cs, stride, rates, out, dc=None, n_rates=None, null_rates=False):
    from vid_dup_finder_lib_amd import _capi

    num, den = np.array([r[0] for r in rates], np.uint32), np.array([r[1] for r in rates], np.uint32)
    job = _capi.VdfWindowsRatesJob(frames, n_clips, f, w, h, fs, cs, stride, len(rates) if n_rates is None else n_rates, None if null_rates else num.ctypes.data,
                                   None if null_rates else den.ctypes.data, out, dc, None)
    job._keep = (num, den)
    return job


def test_no_clips_and_the_error_codes_in_their_order(eng):
    import torch

    import vid_dup_finder_lib_amd as vdf

    multi = None
    try:
        d = torch.zeros(64 * 256, dtype=torch.uint8, device="cuda")
        out = torch.zeros((64, 16), dtype=torch.int64, device="cuda")
        host_frames, host_out = np.zeros(64 * 256, np.uint8), np.zeros((64, 16), np.uint64)
        torch.cuda.synchronize()
        live = eng.lib.vdf_live_device_bytes()
        last = lambda e=eng: e.lib.vdf_last_error(e.ctx).decode()
        for fn, p, o in ((eng.lib.vdf_hash_windows_u8_rates_device, d.data_ptr(), out.data_ptr()), (eng.lib.vdf_hash_windows_u8_rates, host_frames.ctypes.data, host_out.ctypes.data)):
            call = lambda *a, e=eng, **kw: fn(e.ctx, C.byref(_job(*a, **kw)))
            bad = [(1, 1), (5, 2), (2, 1), (4, 5)]  # rate 1 is outside the range; at F = 30 rate 2 spans too much
            assert fn(eng.ctx, None) == -5 and fn(None, C.byref(_job(p, 1, 40, 16, 16, 256, 0, 1, FIVE, o))) == -5
            # the plain call's checks first, in its order - each line breaks one more rule than the one it reports
            assert call(None, 1, 15, 0, 16, 1, 4096, 0, bad, None, n_rates=0) == -1       # frames_per_clip < 16
            assert call(None, 1, 16, 0, 16, 1, 4096, 0, bad, None, n_rates=0) == -2       # a zero dimension
            assert call(None, 1, 16, 16, 16, 255, 4096, 0, bad, None, n_rates=0) == -5 and "frame_stride" in last()
            assert call(None, 1, 16, 16, 16, 256, 4096, 0, bad, None, n_rates=0) == -5 and "window_stride" in last()
            assert call(None, 1, 40, 16, 16, 256, 0, 1, bad, o, n_rates=0) == -5 and "null" in last()      # a null pointer, before the rates
            assert call(p, 1, 40, 16, 16, 256, 0, 1, bad, None, n_rates=0) == -5 and "null" in last()
            # then the number of rates and their arrays, the range, the span
            assert call(p, 1, 30, 16, 16, 256, 0, 1, bad, o, n_rates=0) == -5 and "n_rates" in last()
            assert call(p, 1, 30, 16, 16, 256, 0, 1, [(5, 2)] * 9, o) == -5 and "n_rates" in last()
            assert call(p, 1, 30, 16, 16, 256, 0, 1, bad, o, null_rates=True) == -5 and "null rate array" in last()
            assert call(p, 1, 30, 16, 16, 256, 0, 1, bad, o) == -5 and "(rate 1)" in last()
            for num, den in ((5, 2), (4, 5), (3, 0), (0, 0), (65536, 65536), (65536, 40000)):
                assert call(p, 1, 30, 16, 16, 256, 0, 1, [(1, 1), (2, 1), (num, den)], o) == -5 and "(rate 2)" in last(), (num, den)
            assert call(p, 1, 30, 16, 16, 256, 0, 1, [(1, 1), (3, 2), (2, 1), (31, 16)], o) == -1 and "spans" in last() and "(rate 2)" in last()
            assert call(p, 1, 18, 16, 16, 256, 0, 1, [(6, 5)], o) == -1 and "(rate 0)" in last()
            # 2^32 rows in all, each rate below it: 2^29 clips of 17 frames have 2^30 windows at each of four rates (refused before anything is read)
            assert call(p, 1 << 29, 17, 16, 16, 256, 17 * 256, 1, [(1, 1)] * 4, o) == -5 and "2^32" in last()
            # no clips: nothing to do, even with null pointers - but the arguments are still checked
            assert call(None, 0, 40, 16, 16, 256, 0, 1, FIVE, None) == 0
            assert call(None, 0, 40, 16, 16, 256, 0, 1, bad, None) == -5
            assert call(None, 0, 30, 16, 16, 256, 0, 1, FIVE, None) == -1
        empty = eng.hash_windows_rates(np.zeros((0, 40, 16, 16), np.uint8), FIVE, dontcare=True)
        assert [x.shape for x in empty[0]] == [(0, 0, 16)] * 5 and [x.shape for x in empty[1]] == [(0, 0)] * 5
        torch.cuda.synchronize()
        assert eng.lib.vdf_live_device_bytes() == live  # nothing was allocated, so nothing was launched
        multi = vdf.Engine(devices=[0, 0])
        fn = multi.lib.vdf_hash_windows_u8_rates_device
        assert fn(multi.ctx, C.byref(_job(d.data_ptr(), 1, 40, 16, 16, 256, 0, 1, FIVE, out.data_ptr()))) == -5 and "single-device" in last(multi)
        assert fn(multi.ctx, C.byref(_job(None, 0, 40, 16, 16, 256, 0, 1, FIVE, None))) == -5 and "single-device" in last(multi)
        for rates, code in (([(1, 1), (5, 2)], -5), (FIVE, -1), ([], -5), ([(1, 1)] * 9, -5)):
            with pytest.raises(vdf.VdfError) as ei:
                eng.hash_windows_rates(np.zeros((1, 30, 16, 16), np.uint8), rates)
            assert ei.value.code == code
    finally:
        if multi is not None:
            multi.close()


@pytest.mark.parametrize("true", [(6, 5), (5, 4), (3, 2), (2, 1)], ids=["6_5", "5_4", "3_2", "2_1"])
def test_end_to_end_hash_at_five_rates_align_and_name_the_true_one(eng, true):
    import vid_dup_finder_lib_amd as vdf
    from test_align_rates_host import MIN_RUN, TOLERANCE, hashed

    A, B = retimedgen.corpus(true, 7)
    wa = vdf.hash_frame_windows(A, ["a0", "a1"], [10, 11], engine=eng, rates=FIVE)
    wb = vdf.hash_frame_windows(B, [f"b{i}" for i in range(4)], [10, 11, 12, 13], engine=eng, rates=[(1, 1)])[(1, 1)]
    _, _, oa, ob = hashed(true)
    for rate in FIVE:
        assert all(np.array_equal(np.stack([h.hash for h in ws]), o) for ws, o in zip(wa[rate], oa[rate])), f"windows at {rate} differ from the oracle's"
    assert all(np.array_equal(np.stack([h.hash for h in ws]), o) for ws, o in zip(wb, ob))
    result = vdf.align_rates(wa, wb, TOLERANCE, MIN_RUN, engine=eng, native=True, seed=True)
    assert result == vdf.align_rates(wa, wb, TOLERANCE, MIN_RUN)  # the host forms on the same hashes
    best = {(r.a, r.b): r for r in vdf.best_rates(result, TOLERANCE)}
    assert set(retimedgen.EXCERPTS) <= set(best) and not any(b == 3 for _, b in best)
    for pair in retimedgen.EXCERPTS:
        assert (best[pair].num, best[pair].den) == true, (true, pair, best[pair])
    exact = {(r.a, r.b): r for r in vdf.best_rates(vdf.align_rates(wa, wb, 0.0, MIN_RUN, engine=eng, native=True, seed=True), 0.0)}
    assert set(exact) == set(retimedgen.EXCERPTS)
    for pair, (c, fb0, nb) in retimedgen.EXCERPTS.items():
        r = exact[pair]
        assert (r.num, r.den) == true and r.mean_distance == 0 and (r.first_frame_a, r.first_frame_b, r.n_windows) == (c, fb0, (nb - 16) // true[1] + 1), (true, pair, r)
