"""vdf_hash_windows_clips_u8_rates* (csrc/dct_hash.hip: dct_hash_windows_mixed_rates_kernel behind resize_mfma_mixed_kernel): the retimed
windows of videos of different frame sizes and lengths at SEVERAL rates from one call, rate-major, every block a library in the layout the retimed align calls
read.  Block r is held, row for row and count for count, against ONE vdf_hash_windows_clips_u8_retimed_device call at rate r on the same buffer - also at the
plain taps, where that call takes the plain mixed route - and at the 16 x 16 videos against the oracle on the gathered frames (tests/retimedgen.py): whole words
and don't-care counts, equality, nothing masked.  The library is tests/test_gpu_hash_windows_clips_retimed.py's seven videos (16 x 16 x 31 ... 640 x 360 x 40,
shuffled in one buffer with padded strides, gaps and two boxes, one on each side of the 192-column split); it, the single-rate calls and the oracle's words are
made once and shared."""
import ctypes as C

import numpy as np
import pytest

import retimedgen
import windowgen
from test_gpu_hash_windows_clips_retimed import _library, _pack

pytestmark = pytest.mark.gpu

FIVE = [(1, 1), (6, 5), (5, 4), (3, 2), (2, 1)]
EIGHT = [(2, 1), (1, 1), (6, 5), (3, 2), (5, 4), (12, 10), (31, 16), (2, 1)]  # 12/10 is 6/5 unreduced, 2/1 is listed twice
LISTS = {"1_1+2_1": [(1, 1), (2, 1)], "2_1+1_1": [(2, 1), (1, 1)], "five": FIVE, "eight": EIGHT}
STRIDES = [1, 7, 33]
SENTINEL_ROWS = 8
ONES64, ONES32 = np.uint64(2**64 - 1), 2**32 - 1
_CACHE = {}


@pytest.fixture(scope="module")
def eng():
    import vid_dup_finder_lib_amd as vdf

    e = vdf.Engine(0)
    yield e
    e.close()


def _packed():
    if "packed" not in _CACHE:
        vids, crops, _ = _library()
        _CACHE["packed"] = _pack(vids, crops, order=np.random.default_rng(5).permutation(len(vids)), tail=77)
    return _CACHE["packed"]


def _job(buf_ptr, buf_bytes, recs, nf, stride, rates, out, dc=None, n_rates=None, null_rates=False, stream=None):
    from vid_dup_finder_lib_amd import _capi

    num, den = np.array([r[0] for r in rates], np.uint32), np.array([r[1] for r in rates], np.uint32)
    recs, nf = np.ascontiguousarray(recs), np.ascontiguousarray(nf, np.uint32)
    job = _capi.VdfWindowsClipsRatesJob(buf_ptr, buf_bytes, recs.ctypes.data if len(recs) else None, nf.ctypes.data if len(recs) else None, len(recs), stride,
                                        len(rates) if n_rates is None else n_rates, None if null_rates else num.ctypes.data, None if null_rates else den.ctypes.data,
                                        out, dc, stream)
    job._keep = (num, den, recs, nf)
    return job


def _device_call(eng, buf, recs, n_frames, stride, rates, rows, want_dc=True, raw=None):
    """-> (words [rows, 16], don't-care [rows]); the outputs hold SENTINEL_ROWS more rows than the call may write, filled with a sentinel that must survive.
    raw: keyword arguments of _job, straight to the C ABI (what the python mirror would refuse)."""
    import torch

    d_buf = torch.empty(len(buf), dtype=torch.uint8, device="cuda")  # exactly buf_bytes
    d_buf.copy_(torch.from_numpy(buf))
    d_out = torch.full(((rows + SENTINEL_ROWS) * 16,), -1, dtype=torch.int64, device="cuda")
    d_dc = torch.full((rows + SENTINEL_ROWS,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    try:
        if raw is not None:
            eng._check(eng.lib.vdf_hash_windows_clips_u8_rates_device(eng.ctx, C.byref(_job(d_buf.data_ptr(), len(buf), recs, n_frames, stride, rates, d_out.data_ptr(),
                                                                                         d_dc.data_ptr(), **raw))))
        else:
            eng.hash_windows_clips_rates_device(d_buf.data_ptr(), len(buf), recs, n_frames, stride, rates, d_out.data_ptr(), d_dc.data_ptr() if want_dc else 0)
    finally:
        torch.cuda.synchronize()
        out = d_out.cpu().numpy().view(np.uint64).reshape(-1, 16)
        dc = d_dc.cpu().numpy().view(np.uint32)
        _CACHE["last_outputs"] = (out, dc)
    assert (out[rows:] == ONES64).all() and (dc[rows:] == ONES32).all(), "a row behind the total was written"
    if not want_dc:
        assert (dc == ONES32).all()
    return out[:rows], dc[:rows]


def _single(eng, rate, stride):
    """ONE vdf_hash_windows_clips_u8_retimed_device call at `rate` on the same buffer: (words, counts); once per (quotient's taps, stride)."""
    import torch

    import vid_dup_finder_lib_amd as vdf

    k = ("single", rate, stride)
    if k not in _CACHE:
        buf, recs, nf = _packed()
        rows = int(vdf.hash_windows_first_retimed(nf, rate, stride)[-1])
        d_buf = torch.from_numpy(buf).cuda()
        d_out = torch.full((rows * 16,), -1, dtype=torch.int64, device="cuda")
        d_dc = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
        eng.hash_windows_clips_retimed_device(d_buf.data_ptr(), len(buf), recs, nf, stride, rate, d_out.data_ptr(), d_dc.data_ptr())
        torch.cuda.synchronize()
        _CACHE[k] = (d_out.cpu().numpy().view(np.uint64).reshape(-1, 16), d_dc.cpu().numpy().view(np.uint32))
    return _CACHE[k]


def _oracle(i, rate, stride):
    k = ("oracle", i, rate, stride)
    if k not in _CACHE:
        _CACHE[k] = retimedgen.oracle_windows(_library()[2][i], rate, stride)
    return _CACHE[k]


def _blocks_equal_the_single_rate_calls(eng, got, dc, nf, rates, stride, oracle=True):
    import vid_dup_finder_lib_amd as vdf

    first, rate_first = vdf.hash_windows_first_rates(nf, rates, stride)
    for r, rate in enumerate(rates):
        want, want_dc = _single(eng, rate, stride)
        assert first[r].tolist() == vdf.hash_windows_first_retimed(nf, rate, stride).tolist()
        a, b = int(rate_first[r]), int(rate_first[r + 1])
        assert b - a == len(want)
        for i in range(len(nf)):
            lo, hi = int(first[r, i]), int(first[r, i + 1])
            bad = np.argwhere((got[a + lo:a + hi] != want[lo:hi]).any(axis=1)).reshape(-1)
            assert len(bad) == 0, f"rates {rates} stride {stride}: block {r} ({rate}), video {i}, windows {bad[:8].tolist()} differ from the single-rate call's"
            if dc is not None:
                assert np.array_equal(dc[a + lo:a + hi], want_dc[lo:hi]), f"rates {rates} stride {stride}: block {r} ({rate}), video {i}: don't-care counts"
            if oracle and i < 2:  # the 16 x 16 videos (31 and 40 frames): the oracle on the gathered frames
                words, counts = _oracle(i, rate, stride)
                assert np.array_equal(got[a + lo:a + hi], words) and (dc is None or np.array_equal(dc[a + lo:a + hi], counts)), (rates, stride, r, i)


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("name", list(LISTS))
def test_parity_of_every_block_with_the_single_rate_library_call_and_the_oracle(eng, name, stride):
    import vid_dup_finder_lib_amd as vdf

    rates = LISTS[name]
    buf, recs, nf = _packed()
    assert (recs["offset"] % 4 != 0).all() and not np.array_equal(np.argsort(recs["offset"]), np.arange(len(recs)))  # odd offsets, shuffled in the buffer
    first, rate_first = vdf.hash_windows_first_rates(nf, rates, stride)
    want_first = np.stack([np.concatenate([[0], np.cumsum([retimedgen.n_windows(int(f), stride, r) for f in nf])]) for r in rates])
    assert first.tolist() == want_first.tolist() and rate_first.tolist() == np.concatenate([[0], np.cumsum(want_first[:, -1])]).tolist()
    rows = int(rate_first[-1])
    got, dc = _device_call(eng, buf, recs, nf, stride, rates, rows)
    _blocks_equal_the_single_rate_calls(eng, got, dc, nf, rates, stride)
    got_n, _ = _device_call(eng, buf, recs, nf, stride, rates, rows, want_dc=False)  # the don't-care pointer null
    assert np.array_equal(got_n, got)
    _CACHE["device", name, stride] = (got, dc)


@pytest.mark.parametrize("name,stride", [("five", 1), ("eight", 7)])
def test_host_form_equals_device_form(eng, name, stride):
    import vid_dup_finder_lib_amd as vdf

    rates = LISTS[name]
    vids, crops, _ = _library()
    buf, recs, nf = _packed()
    first, rate_first = vdf.hash_windows_first_rates(nf, rates, stride)
    rows = int(rate_first[-1])
    got, dc = _CACHE.get(("device", name, stride)) or _device_call(eng, buf, recs, nf, stride, rates, rows)
    out = np.full((rows + 1, 16), ONES64, np.uint64)
    out_dc = np.full(rows + 1, ONES32, np.uint32)
    eng._check(eng.lib.vdf_hash_windows_clips_u8_rates(eng.ctx, C.byref(_job(buf.ctypes.data, buf.size, recs, nf, stride, rates, out.ctypes.data, out_dc.ctypes.data))))
    assert np.array_equal(out[:rows], got) and np.array_equal(out_dc[:rows], dc) and (out[rows] == ONES64).all() and out_dc[rows] == ONES32
    words, first_l, dc_l = eng.hash_windows_clips_rates(vids, rates, stride, crops=crops, want_dontcare=True)  # packed on 64-byte boundaries: the same words
    assert first_l.tolist() == first.tolist() and len(words) == len(dc_l) == len(rates)
    assert np.array_equal(np.concatenate(words), got) and np.array_equal(np.concatenate(dc_l), dc)
    only, first_o = eng.hash_windows_clips_rates(vids, rates, stride, crops=crops)
    assert all(np.array_equal(x, y) for x, y in zip(only, words)) and first_o.tolist() == first.tolist()
    empty, first_e = eng.hash_windows_clips_rates([], rates, stride)  # n_videos == 0
    assert [x.shape for x in empty] == [(0, 16)] * len(rates) and first_e.tolist() == [[0]] * len(rates)


def test_a_thousand_videos_of_31_frames_one_segment_each(eng):
    """seg_first holds 1000 single-segment entries: every workgroup's binary search ends on another video; 16 windows in the 1/1 block and 1 in the 2/1 block per
    video, and every row is written once."""
    from vid_dup_finder_lib_amd.engine import CLIP_DTYPE

    rng = np.random.default_rng(31)
    frames = rng.integers(0, 256, size=(1000, 31, 16, 16), dtype=np.uint8)
    plain, plain_dc = eng.hash_windows_retimed(frames, (1, 1), 1, want_dontcare=True)
    twice, twice_dc = eng.hash_windows_retimed(frames, (2, 1), 1, want_dontcare=True)
    assert plain.shape == (1000, 16, 16) and twice.shape == (1000, 1, 16)
    recs = np.zeros(1000, CLIP_DTYPE)
    recs["frame_stride"], recs["w"], recs["h"] = 256, 16, 16
    gaps = rng.integers(0, 3, size=1000) * 4  # irregular offsets: not the uniform route
    recs["offset"] = (np.arange(1000) * 31 * 256 + np.cumsum(gaps)).astype(np.uint64)
    buf = np.full(int(recs["offset"][-1]) + 31 * 256, 0xAA, np.uint8)
    for i in range(1000):
        buf[int(recs["offset"][i]):int(recs["offset"][i]) + 31 * 256] = frames[i].reshape(-1)
    got, dc = _device_call(eng, buf, recs, np.full(1000, 31, np.uint32), 1, [(1, 1), (2, 1)], 17000)
    bad = np.argwhere((got[:16000].reshape(1000, 16, 16) != plain).any(axis=(1, 2))).reshape(-1)
    assert len(bad) == 0, f"1/1 block: videos {bad[:8].tolist()} differ from the uniform call's"
    bad = np.argwhere((got[16000:] != twice[:, 0]).any(axis=1)).reshape(-1)
    assert len(bad) == 0, f"2/1 block: videos {bad[:8].tolist()} differ from the uniform call's"
    assert np.array_equal(dc[:16000], plain_dc.reshape(-1)) and np.array_equal(dc[16000:], twice_dc[:, 0])


def test_every_row_up_to_the_total_is_overwritten_and_none_behind_it(eng):
    """The outputs are prefilled with ones and hold 8 rows behind the total: _device_call asserts those survive; here every row in front is NOT the sentinel."""
    import vid_dup_finder_lib_amd as vdf

    buf, recs, nf = _packed()
    for rates, stride in ((FIVE, 1), ([(2, 1), (1, 1)], 33), ([(3, 2)], 7)):
        rows = int(vdf.hash_windows_first_rates(nf, rates, stride)[1][-1])
        got, dc = _device_call(eng, buf, recs, nf, stride, rates, rows)
        assert not (got[:, 15] == ONES64).any(), "a row kept its sentinel: word 15 of a hash has bits 1000 ... 1023 clear"
        assert (dc <= 1000).all(), "a don't-care count kept its sentinel"
        if len(rates) == 1:  # a one-rate list takes the new kernel too: the single-rate call's words
            _blocks_equal_the_single_rate_calls(eng, got, dc, nf, rates, stride, oracle=False)


@pytest.mark.parametrize("w,h,nf", [(64, 48, 40), (16, 16, 33)])
def test_a_uniform_library_takes_the_uniform_rates_route(eng, w, h, nf):
    import torch

    from vid_dup_finder_lib_amd.engine import CLIP_DTYPE

    rng = np.random.default_rng(w + nf)
    frames = np.stack([windowgen.video(rng, nf, h, w, lead=(0, 5, 3)[c % 3]) for c in range(5)])
    step = nf * w * h + 12  # padded between the videos: still one step
    buf = np.full(5 * step, 0xAA, np.uint8)
    for c in range(5):
        buf[c * step:c * step + nf * w * h] = frames[c].reshape(-1)
    recs = np.zeros(5, CLIP_DTYPE)
    recs["offset"], recs["frame_stride"], recs["w"], recs["h"] = np.arange(5, dtype=np.uint64) * np.uint64(step), w * h, w, h
    import vid_dup_finder_lib_amd as vdf

    for rates, stride in ((FIVE, 1), ([(2, 1), (1, 1)], 5)):
        total, _ = vdf.hash_window_count_rates(5, nf, stride, rates)
        d_buf = torch.from_numpy(buf).cuda()
        d_out = torch.full((total * 16,), -1, dtype=torch.int64, device="cuda")
        d_dc = torch.full((total,), -1, dtype=torch.int32, device="cuda")
        eng.hash_windows_rates_device(d_buf.data_ptr(), 5, nf, w, h, stride, rates, d_out.data_ptr(), d_dontcare=d_dc.data_ptr(), clip_stride=step)
        torch.cuda.synchronize()
        got, dc = _device_call(eng, buf, recs, np.full(5, nf, np.uint32), stride, rates, total)
        assert np.array_equal(got, d_out.cpu().numpy().view(np.uint64).reshape(-1, 16)) and np.array_equal(dc, d_dc.cpu().numpy().view(np.uint32))
        first, rate_first = vdf.hash_windows_first_rates(np.full(5, nf), rates, stride)  # the rows coincide: first[r][c] = c n_win_r
        assert rate_first[-1] == total and all(first[r].tolist() == (np.arange(6) * retimedgen.n_windows(nf, stride, rate)).tolist() for r, rate in enumerate(rates))


def test_errors_come_in_the_stated_order_and_launch_nothing(eng):
    import vid_dup_finder_lib_amd as vdf

    vids, crops, _ = _library()
    vids, crops = vids[:4], crops[:4]  # 31, 40, 33 and 47 frames
    buf, recs, nf = _pack(vids, crops)
    good = [(1, 1), (6, 5)]
    rows = int(vdf.hash_windows_first_rates(nf, good, 1)[1][-1])

    def refused(code, texts, rates, r=recs, f=nf, stride=1, nbytes=None, **raw):
        with pytest.raises(vdf.VdfError) as ei:
            _device_call(eng, buf if nbytes is None else buf[:nbytes], r, f, stride, rates, rows, raw=raw)
        assert ei.value.code == code and all(t in str(ei.value) for t in texts), (ei.value, code, texts)
        out, dc = _CACHE["last_outputs"]
        assert (out == ONES64).all() and (dc == ONES32).all(), "a rejected call wrote to its outputs"

    assert eng.lib.vdf_hash_windows_clips_u8_rates_device(eng.ctx, None) == -5 and eng.lib.vdf_hash_windows_clips_u8_rates(eng.ctx, None) == -5
    last = int(np.argmax(recs["offset"]))
    f15 = nf.copy(); f15[2] = 15
    bad = [(1, 1), (5, 2), (2, 1)]  # rate 1 is no rate; f30 below is too short for rate 2
    f30 = nf.copy(); f30[1] = 30; f30[2] = 29  # (the video at the end of the buffer keeps its frames)
    assert last == 3
    # the plain mixed call's checks first, in their order, each with a bad list, a bad rate AND a too-short video behind it
    refused(-1, ["fewer than 16", "video 2"], bad, f=f15, stride=0, nbytes=10, n_rates=0)
    refused(-5, ["past the end", f"video {last}"], bad, f=f30, nbytes=len(buf) - 1)
    refused(-5, ["window_stride"], bad, f=f30, stride=0)
    # then the number of rates and their arrays
    refused(-5, ["n_rates"], bad, f=f30, n_rates=0)
    refused(-5, ["n_rates"], [(5, 2)] * 9, f=f30)
    refused(-5, ["null rate array"], bad, f=f30, null_rates=True)
    # then the first rate outside the range, in front of the too-short video
    refused(-5, ["(rate 1)"], bad, f=f30)
    for num, den in ((5, 2), (4, 5), (1, 0), (0, 0), (65536, 65536)):
        refused(-5, ["(rate 2)"], [(1, 1), (2, 1), (num, den)], f=f30)
    # then, in LIST order, the first rate some video is too short for, and the first such video: 30 and 29 frames at 31/16 (span 30) and 2/1 (span 31)
    refused(-1, ["spans", "rate 1", "video 2"], [(1, 1), (31, 16), (2, 1)], f=f30)
    refused(-1, ["spans", "rate 1", "video 1"], [(1, 1), (2, 1), (31, 16)], f=f30)
    refused(-1, ["spans", "rate 0", "video 0"], [(2, 1), (1, 1)], f=np.array([30, 40, 33, 47], np.uint32))
    # n_videos == 0: VDF_OK, nothing launched - but the rates are still checked
    got, _ = _device_call(eng, buf, recs[:0], nf[:0], 1, good, 0, raw={})
    assert got.shape == (0, 16)
    refused(-5, ["(rate 1)"], bad, r=recs[:0], f=nf[:0])
    # the python mirror reports the library's codes
    for rates, code in (([(1, 1), (5, 2)], -5), ([], -5), ([(1, 1)] * 9, -5)):
        with pytest.raises(vdf.VdfError) as ei:
            eng.hash_windows_clips_rates(vids, rates)
        assert ei.value.code == code
    with pytest.raises(vdf.VdfError) as ei:
        eng.hash_windows_clips_rates([v[:30] for v in vids], FIVE)
    assert ei.value.code == -1
    # the context goes on: the same videos, valid
    got, dc = _device_call(eng, buf, recs, nf, 1, good, rows)
    first, rate_first = vdf.hash_windows_first_rates(nf, good, 1)
    _, _, cropped = _library()
    for r, rate in enumerate(good):
        want = np.concatenate([eng.hash_windows_retimed(v[None], rate, 1)[0] for v in cropped[:4]])
        assert np.array_equal(got[int(rate_first[r]):int(rate_first[r + 1])], want)


def test_a_multi_gpu_context_is_refused(eng):
    import vid_dup_finder_lib_amd as vdf

    multi = vdf.Engine(devices=[0, 0])
    try:
        vids, crops, _ = _library()
        buf, recs, nf = _pack(vids[:2], crops[:2])
        with pytest.raises(vdf.VdfError) as ei:
            _device_call(multi, buf, recs, nf, 1, [(1, 1), (6, 5)], 4)
        assert ei.value.code == -5 and "single-device" in str(ei.value)
        out, dc = _CACHE["last_outputs"]
        assert (out == ONES64).all() and (dc == ONES32).all()
    finally:
        multi.close()


def _planted(seed):
    """Six noise videos of three frame sizes, and three files that hold B[j] = A[c + (j * num) // den] of videos 0, 2 and 4 - two different true rates."""
    rng = np.random.default_rng(seed)
    sizes = [(16, 16), (32, 24), (64, 48)]
    a = [rng.integers(0, 256, size=(f, sizes[i % 3][1], sizes[i % 3][0]), dtype=np.uint8) for i, f in enumerate((100, 90, 110, 80, 95, 85))]
    cut = lambda v, c, n, rate: np.ascontiguousarray(v[c + (np.arange(n) * rate[0]) // rate[1]])
    plan = {(0, 0): (0, 40, (6, 5)), (2, 1): (7, 36, (2, 1)), (4, 2): (13, 30, (6, 5))}
    return a, [cut(a[i], c, n, rate) for (i, _), (c, n, rate) in sorted(plan.items(), key=lambda kv: kv[0][1])], plan


def test_end_to_end_hash_the_library_once_align_and_name_every_true_rate(eng):
    import vid_dup_finder_lib_amd as vdf

    a, b, planted = _planted(21)
    pa, pb = [f"/a/{i}.mp4" for i in range(len(a))], [f"/b/{i}.mp4" for i in range(len(b))]
    wa = vdf.hash_frame_windows(a, pa, [len(v) for v in a], engine=eng, rates=FIVE, one_call=True)
    wa_each = vdf.hash_frame_windows(a, pa, [len(v) for v in a], engine=eng, rates=FIVE)
    assert list(wa) == FIVE == list(wa_each)
    for rate in FIVE:
        assert [len(w) for w in wa[rate]] == [retimedgen.n_windows(len(v), 1, rate) for v in a]
        for x, y in zip(wa[rate], wa_each[rate]):
            assert len(x) == len(y) and all(np.array_equal(p.hash, q.hash) and p.src_path() == q.src_path() and p.duration() == q.duration() for p, q in zip(x, y))
    wb = vdf.hash_frame_windows(b, pb, [len(v) for v in b], engine=eng, rates=[(1, 1)], one_call=True)[(1, 1)]  # the 1/1 block is a B side
    plain = vdf.hash_frame_windows(b, pb, [len(v) for v in b], engine=eng)
    assert all(np.array_equal(p.hash, q.hash) for x, y in zip(wb, plain) for p, q in zip(x, y)) and [len(x) for x in wb] == [len(x) for x in plain]
    result = vdf.align_rates(wa, wb, 0.0, 2, engine=eng, native=True, seed=True)
    assert result == vdf.align_rates(wa_each, wb, 0.0, 2, engine=eng, native=True, seed=True)  # the records equal those from one_call=False
    best = {(r.a, r.b): r for r in vdf.best_rates(result, 0.0)}
    assert set(best) == set(planted), best
    for pair, (c, n, rate) in planted.items():
        r = best[pair]
        assert (r.num, r.den) == rate and r.mean_distance == 0 and (r.first_frame_a, r.first_frame_b, r.n_windows) == (c, 0, (n - 16) // rate[1] + 1), (pair, r)
        assert r.path_a == pa[pair[0]] and r.path_b == pb[pair[1]]


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
    rates = [(6, 5), (1, 1), (2, 1)]
    auto = vdf.hash_frame_windows(vids, paths, durs, stride=2, engine=eng, rates=rates, one_call=True, letterbox=True)
    by_hand = vdf.hash_frame_windows(vids, paths, durs, stride=2, engine=eng, rates=rates, one_call=True, crops=boxes)
    bare = vdf.hash_frame_windows(vids, paths, durs, stride=2, engine=eng, rates=rates, one_call=True)
    for rate in rates:
        single = vdf.hash_frame_windows(vids, paths, durs, stride=2, engine=eng, rate=rate, one_call=True, letterbox=True)
        assert any(not np.array_equal(p.hash, q.hash) for p, q in zip(auto[rate][0], bare[rate][0]))  # the bars are not hashed
        for i in range(len(vids)):
            assert len(auto[rate][i]) == len(single[i]) == retimedgen.n_windows(len(vids[i]), 2, rate)
            assert all(np.array_equal(x.hash, y.hash) for x, y in zip(auto[rate][i], single[i])), f"video {i} at {rate}: words differ from the single-rate one_call's"
            assert all(np.array_equal(x.hash, y.hash) for x, y in zip(auto[rate][i], by_hand[rate][i]))
    for bad in (dict(rate=(2, 1)), dict(zero_plane=True)):
        with pytest.raises(ValueError):
            vdf.hash_frame_windows(vids, paths, durs, engine=eng, rates=rates, one_call=True, **bad)
    with pytest.raises(ValueError):
        vdf.hash_frame_windows(vids, paths, durs, engine=eng, rates=rates, letterbox=True)  # boxes need the one call
