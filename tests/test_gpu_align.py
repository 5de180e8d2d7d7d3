"""vdf_align_windows[_device] (csrc/align.hip: align_bands_kernel and its reductions) against the numpy twin of tests/aligngen.py, records equal
field for field: the device form on device arrays and the host-array form, on every problem tests/test_align_host.py gives the plain C++ definition - window
counts on both sides of the 64-diagonal band and the 64-row reload wrap, runs on the corner diagonals, at every matrix edge, across the wrap and on the two
sides of a band boundary, ties, tolerances on and one over, min_run, skip bytes, static videos where every cell matches, self mode - then the buffer
protocol, hash_frame_windows -> align end to end, and the argument checks with their messages."""
import numpy as np
import pytest

import aligngen
import hashgen
import windowgen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import vid_dup_finder_lib_amd as vdf

    e = vdf.Engine(0)
    yield e
    e.close()


def _dev(x, dtype):
    import torch

    return None if x is None else torch.from_numpy(np.ascontiguousarray(x).view(dtype).copy()).cuda()


def device_form(eng, p, capacity=4096):
    """the problem's arrays as device arrays of exactly their size -> (records, found)"""
    import torch

    ah, af, ak = _dev(p.a_hashes, np.int64), _dev(p.a_first, np.int32), _dev(p.a_skip, np.uint8)
    bh, bf, bk = _dev(p.b_hashes, np.int64), _dev(p.b_first, np.int32), _dev(p.b_skip, np.uint8)
    torch.cuda.synchronize()
    ptr = lambda t: 0 if t is None else t.data_ptr()
    rec, found = eng.align_windows_device(ptr(ah), ptr(af), len(p.a_first) - 1, ptr(bh), ptr(bf), 0 if bf is None else len(p.b_first) - 1, tol_int=p.tol,
                                          min_run=p.min_run, d_a_skip=ptr(ak), d_b_skip=ptr(bk), capacity=capacity)
    return aligngen.records(rec), found


def host_array_form(eng, p, capacity=4096):
    rec, found = eng.align_windows(p.a_hashes, p.a_first, p.b_hashes, p.b_first, tol_int=p.tol, min_run=p.min_run, a_skip=p.a_skip, b_skip=p.b_skip,
                                   capacity=capacity)
    return aligngen.records(rec), found


@pytest.mark.parametrize("name", sorted(aligngen.CASES))
def test_kernel_matches_the_twin(eng, name):
    p, want = aligngen.case(name), list(aligngen.expected(name))
    got, found = device_form(eng, p)
    print(f"{name}: {len(want)} records, device form found {found}")
    assert found == len(want)
    assert got == want
    got, found = host_array_form(eng, p)
    assert found == len(want) and got == want


def test_static_videos_give_one_record_per_pair(eng):
    """every cell matches: 4 x 3 pairs of up to 200 x 129 cells each, and still 12 records and no overflow of anything"""
    p = aligngen._static([200, 64, 65, 1], [129, 200, 63])
    want = aligngen.align_twin(p)
    assert len(want) == 12 and want[0] == (0, 0, -71, 71, 129, 0) and want[1] == (0, 1, 0, 0, 200, 0) and want[5] == (1, 2, -1, 1, 63, 0)
    assert device_form(eng, p) == (want, 12)


def test_self_mode_is_a_against_a_without_the_lower_triangle(eng):
    p = aligngen.case("self_mode")
    both, _ = device_form(eng, p._replace(b_hashes=p.a_hashes, b_first=p.a_first))
    assert [r for r in both if r[0] < r[1]] == list(aligngen.expected("self_mode"))
    got, _ = device_form(eng, p)
    assert all(a < b for a, b, *_ in got) and got == list(aligngen.expected("self_mode"))


def test_capacity_smaller_than_the_result(eng):
    p, want = aligngen.case("self_mode"), list(aligngen.expected("self_mode"))
    assert len(want) > 5
    for form in (device_form, host_array_form):
        got, found = form(eng, p, capacity=5)
        assert found == len(want) and got == want[:5]  # the count is right and the prefix is valid
        got, found = form(eng, p, capacity=0)
        assert found == len(want) and got == []
        got, found = form(eng, p, capacity=found)      # the second call is complete
        assert found == len(want) and got == want


def test_end_to_end_excerpt_of_a_longer_video(eng):
    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(31)
    v0 = windowgen.video(rng, 80, 64, 64)
    v1 = np.concatenate([v0[23:], rng.integers(0, 256, size=(23, 64, 64), dtype=np.uint8)])  # frames 23 .. 79 of video 0, then something else
    v2 = windowgen.video(np.random.default_rng(32), 80, 64, 64, lead=9)
    videos = np.stack([v0, v1, v2])
    windows = vdf.hash_frame_windows(videos, ["a.mp4", "b.mp4", "c.mp4"], [80, 80, 80], stride=1, engine=eng)
    assert [len(w) for w in windows] == [65, 65, 65]
    got = vdf.align(windows, tolerance=vdf.DEFAULT_SEARCH_TOLERANCE, min_run=4, engine=eng)
    # the twin on the same hashes
    words = np.stack([h.hash for ws in windows for h in ws])
    p = aligngen.Problem(words, aligngen.first_of([65, 65, 65]), None, None, 350, 4)
    want = aligngen.align_twin(p)
    assert [(g.a, g.b, g.offset_frames, g.first_frame_a, g.n_windows, round(g.mean_distance * g.n_windows)) for g in got] == want
    g = got[0]
    assert (g.a, g.b, g.offset_frames, g.first_frame_a, g.first_frame_b, g.n_frames, g.n_windows, g.mean_distance) == (0, 1, -23, 23, 0, 57, 42, 0.0)
    assert (g.path_a, g.path_b) == ("a.mp4", "b.mp4")
    # static windows abstain: the excerpt is still found, whatever the static stretches of video 2 matched before
    _, dc = eng.hash_windows(videos, 1, want_dontcare=True)
    flags = [vdf.static_windows(d) for d in dc]
    assert sum(int(f.sum()) for f in flags) >= 6  # (two static and one constant window per generated video, fewer where the excerpt cut them)
    quiet = vdf.align(windows, min_run=4, static_a=flags, engine=eng)
    assert quiet[0] == g
    skip = np.concatenate(flags)
    assert [(q.a, q.b, q.offset_frames, q.first_frame_a, q.n_windows) for q in quiet] == [r[:5] for r in aligngen.align_twin(p._replace(a_skip=skip))]
    # stride 4: every fourth window, the excerpt starts 23 frames in - not a multiple of the stride, so its windows hold other frames
    w4 = vdf.hash_frame_windows(videos, ["a.mp4", "b.mp4", "c.mp4"], [80, 80, 80], stride=4, engine=eng)
    shifted = np.stack([v0, np.concatenate([v0[24:], v0[:24]]), v2])  # frames 24 ..: six windows of stride 4 in
    w4s = vdf.hash_frame_windows(shifted, ["a.mp4", "b.mp4", "c.mp4"], [80, 80, 80], stride=4, engine=eng)
    g4 = [g for g in vdf.align(w4, w4s, min_run=4, stride=4, engine=eng) if (g.a, g.b) == (0, 1)][0]
    assert (g4.offset_frames, g4.first_frame_a, g4.first_frame_b, g4.n_windows, g4.n_frames, g4.mean_distance) == (-24, 24, 0, 11, 56, 0.0)


def test_argument_checks_in_their_order(eng):
    import torch

    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(3)
    h = _dev(hashgen.random_hashes(rng, 8), np.int64)
    first = lambda *v: _dev(np.array(v, np.uint32), np.int32)
    f = first(0, 3, 8)
    out = np.zeros(16, vdf.ALIGN_DTYPE)
    n = __import__("ctypes").c_size_t(99)
    torch.cuda.synchronize()
    lib = eng.lib
    ref = __import__("ctypes").byref

    def call(ctx, ah, af, n_a, bh, bf, n_b, min_run, o=out.ctypes.data, cap=16, n_out=True):
        p = lambda t: None if t is None else t.data_ptr()
        return lib.vdf_align_windows_device(ctx, p(ah), p(af), n_a, None, p(bh), p(bf), n_b, None, 350, min_run, o, cap, ref(n) if n_out else None, None)

    err = lambda c: lib.vdf_last_error(c).decode()
    # each line breaks one more rule than the one it reports: the earlier check wins
    assert call(eng.ctx, None, f, 2, None, None, 0, 0) == -5 and "null" in err(eng.ctx)          # a null pointer (and min_run == 0)
    assert call(eng.ctx, h, f, 2, None, None, 0, 1, n_out=False) == -5 and "null" in err(eng.ctx)
    assert call(eng.ctx, h, f, 2, None, None, 0, 1, o=None) == -5 and "null" in err(eng.ctx)
    big = first(0, 2**20 + 1, 2**20 - 5)
    assert call(eng.ctx, h, big, 2, None, None, 0, 0) == -5 and "min_run" in err(eng.ctx)        # min_run == 0 (and too many windows, ...)
    assert call(eng.ctx, h, big, 2, None, None, 0, 1) == -5 and "2^20" in err(eng.ctx)           # too many windows (and a decreasing first array)
    assert call(eng.ctx, h, f, 2, h, first(0, 2**20 + 1), 1, 1) == -5 and "of B" in err(eng.ctx)
    assert call(eng.ctx, h, first(0, 5, 3), 2, None, None, 0, 1) == -5 and "decreases" in err(eng.ctx)
    zeros = _dev(np.zeros(4098, np.uint32), np.int32)
    assert call(eng.ctx, h, zeros, 4097, h, zeros, 4097, 1) == -5 and "2^24" in err(eng.ctx)
    assert call(eng.ctx, h, zeros, 4096, h, zeros, 4096, 1) == 0 and n.value == 0                   # 2^24 pairs of empty videos: legal, nothing to do
    # nothing to do
    n.value = 99
    assert call(eng.ctx, h, f, 0, None, None, 0, 1) == 0 and n.value == 0
    n.value = 99
    assert call(eng.ctx, h, f, 1, None, None, 0, 1) == 0 and n.value == 0                           # self mode with one video
    n.value = 99
    assert call(eng.ctx, h, f, 2, h, f, 0, 1) == 0 and n.value == 0
    assert call(eng.ctx, h, first(0, 0, 8), 2, h, first(0, 8, 8), 2, 1) == 0                       # videos of 0 windows are legal
    # a multi-GPU context: the last check, in both forms
    multi = vdf.Engine(devices=[0, 0])
    try:
        assert call(multi.ctx, h, f, 2, None, None, 0, 0) == -5 and "min_run" in err(multi.ctx)
        assert call(multi.ctx, h, f, 2, None, None, 0, 1) == -5 and "single-device" in err(multi.ctx)
        with pytest.raises(vdf.VdfError) as ei:
            multi.align_windows(hashgen.random_hashes(rng, 8), [0, 3, 8])
        assert ei.value.code == -5 and "single-device" in str(ei.value)
    finally:
        multi.close()


def test_no_device_memory_is_left_behind():
    import vid_dup_finder_lib_amd as vdf

    lib = vdf._capi.load()
    before = lib.vdf_live_device_bytes()
    e = vdf.Engine(0)
    p = aligngen.case("reload_wrap")
    assert host_array_form(e, p)[0] == list(aligngen.expected("reload_wrap"))
    assert lib.vdf_live_device_bytes() > before
    e.close()
    assert lib.vdf_live_device_bytes() == before
