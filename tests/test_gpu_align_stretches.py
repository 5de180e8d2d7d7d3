"""vdf_align_windows_stretches[_device] (csrc/align.hip: align_bands_kernel<AlignPairUnits<false>, true> behind the plain kernel's round 0) against the numpy
twin of tests/stretchgen.py, records equal field for field: the device form on device arrays and the host-array form, on every problem
tests/test_align_stretches_host.py gives the plain C++ definition - an ad break removed, a source used twice, two runs on one diagonal, static
videos tiled rank by rank, slowly changing content with and without the guard, a rectangle across three bands and the 64-row reload wrap that
cuts a run in two, both clamps of the guard, a run that falls under min_run once it is cut, self mode, skip bytes, mixed window counts - at
max_stretches 1, 2 and 8; then the rank-0 subset against the plain align call, the buffer protocol, the argument checks with their messages in
their order, hash_frame_windows -> align_all end to end, and the device memory after close."""
import ctypes as C

import numpy as np
import pytest

import aligngen
import hashgen
import stretchgen

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


def _device_arrays(p):
    import torch

    arrays = (_dev(p.a_hashes, np.int64), _dev(p.a_first, np.int32), _dev(p.a_skip, np.uint8), _dev(p.b_hashes, np.int64), _dev(p.b_first, np.int32),
              _dev(p.b_skip, np.uint8))
    torch.cuda.synchronize()
    return arrays


def device_form(eng, p, max_stretches, guard, capacity=8192):
    """the problem's arrays as device arrays of exactly their size -> (records, found)"""
    ah, af, ak, bh, bf, bk = _device_arrays(p)
    ptr = lambda t: 0 if t is None else t.data_ptr()
    rec, found = eng.align_windows_stretches_device(ptr(ah), ptr(af), len(p.a_first) - 1, ptr(bh), ptr(bf), 0 if bf is None else len(p.b_first) - 1,
                                                    tol_int=p.tol, min_run=p.min_run, max_stretches=max_stretches, guard=guard, d_a_skip=ptr(ak),
                                                    d_b_skip=ptr(bk), capacity=capacity)
    return stretchgen.records(rec), found


def host_array_form(eng, p, max_stretches, guard, capacity=8192):
    rec, found = eng.align_windows_stretches(p.a_hashes, p.a_first, p.b_hashes, p.b_first, tol_int=p.tol, min_run=p.min_run, max_stretches=max_stretches,
                                             guard=guard, a_skip=p.a_skip, b_skip=p.b_skip, capacity=capacity)
    return stretchgen.records(rec), found


@pytest.mark.parametrize("name,guard", stretchgen.CASES)
def test_kernel_matches_the_twin(eng, name, guard):
    p = stretchgen.case(name)
    for max_stretches in (1, 2, 8):
        want = list(stretchgen.expected(name, guard, max_stretches))
        got, found = device_form(eng, p, max_stretches, guard)
        print(f"{name} guard {guard} max_stretches {max_stretches}: {len(want)} records, device form found {found}")
        assert found == len(want)
        assert got == want
        got, found = host_array_form(eng, p, max_stretches, guard)
        assert found == len(want) and got == want


def test_rank_zero_is_the_plain_align_call(eng):
    for name, guard in (("mixed_counts", 2), ("self_mode", 0), ("rect_across_bands", 2), ("skip_cuts", 0)):
        p = stretchgen.case(name)
        ah, af, ak, bh, bf, bk = _device_arrays(p)
        ptr = lambda t: 0 if t is None else t.data_ptr()
        n_b = 0 if bf is None else len(p.b_first) - 1
        plain, n_plain = eng.align_windows_device(ptr(ah), ptr(af), len(p.a_first) - 1, ptr(bh), ptr(bf), n_b, tol_int=p.tol, min_run=p.min_run, d_a_skip=ptr(ak),
                                                  d_b_skip=ptr(bk), capacity=8192)
        rec, _ = eng.align_windows_stretches_device(ptr(ah), ptr(af), len(p.a_first) - 1, ptr(bh), ptr(bf), n_b, tol_int=p.tol, min_run=p.min_run, max_stretches=8,
                                                    guard=guard, d_a_skip=ptr(ak), d_b_skip=ptr(bk), capacity=8192)
        got = stretchgen.records(rec)
        assert n_plain == len(plain) > 0 and [r[:6] for r in got if r[6] == 0] == aligngen.records(plain)
        one, n_one = eng.align_windows_stretches_device(ptr(ah), ptr(af), len(p.a_first) - 1, ptr(bh), ptr(bf), n_b, tol_int=p.tol, min_run=p.min_run,
                                                        max_stretches=1, guard=guard, d_a_skip=ptr(ak), d_b_skip=ptr(bk), capacity=8192)
        assert n_one == n_plain and stretchgen.records(one) == [r + (0,) for r in aligngen.records(plain)]


def test_capacity_smaller_than_the_result(eng):
    p, want = stretchgen.case("self_mode"), list(stretchgen.expected("self_mode", 0))
    assert len(want) > 5
    for form in (device_form, host_array_form):
        got, found = form(eng, p, 8, 0, capacity=5)
        assert found == len(want) and got == want[:5]  # the count is right and the prefix is valid
        got, found = form(eng, p, 8, 0, capacity=0)
        assert found == len(want) and got == []
        got, found = form(eng, p, 8, 0, capacity=found)  # the second call is complete
        assert found == len(want) and got == want


def test_end_to_end_a_reupload_with_a_break_removed(eng):
    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(41)
    v0 = rng.integers(0, 256, size=(120, 64, 64), dtype=np.uint8)
    v1 = np.concatenate([v0[:40], v0[60:], rng.integers(0, 256, size=(20, 64, 64), dtype=np.uint8)])  # frames 40 .. 59 removed, noise appended
    v2 = rng.integers(0, 256, size=(120, 64, 64), dtype=np.uint8)
    windows = vdf.hash_frame_windows(np.stack([v0, v1, v2]), ["a.mp4", "b.mp4", "c.mp4"], [120, 120, 120], stride=1, engine=eng)
    assert [len(w) for w in windows] == [105, 105, 105]
    got = vdf.align_all(windows, tolerance=vdf.DEFAULT_SEARCH_TOLERANCE, min_run=4, stride=1, engine=eng)
    # the twin on the same hashes, at align_all's defaults: four stretches, the guard of stride 1
    words = np.stack([h.hash for ws in windows for h in ws])
    p = aligngen.Problem(words, aligngen.first_of([105, 105, 105]), None, None, 350, 4)
    want = stretchgen.stretches_twin(p, 4, 15)
    assert [(g.a, g.b, g.offset_frames, g.first_frame_a, g.n_windows, round(g.mean_distance * g.n_windows), g.rank) for g in got] == want
    assert [(g.a, g.b, g.rank) for g in got] == [(0, 1, 0), (0, 1, 1)]
    assert sorted(g.offset_frames for g in got) == [-20, 0]
    late, early = got  # the longer stretch is rank 0: frames 60 .. 119 of a are frames 40 .. 99 of b
    # (windows that straddle the cut share most of their frames with a window of a and may match too: the stretch may begin before frame 60)
    assert late.offset_frames == -20 and late.first_frame_a <= 60 and late.first_frame_a + late.n_windows == 105 and late.first_frame_b == late.first_frame_a - 20
    assert late.n_frames == late.n_windows + 15 >= 60
    assert (early.offset_frames, early.first_frame_a, early.first_frame_b) == (0, 0, 0) and early.n_windows >= 25 and early.n_frames >= 40
    assert (late.path_a, late.path_b, early.path_b) == ("a.mp4", "b.mp4", "b.mp4")
    # align sees the better one only
    one = vdf.align(windows, min_run=4, engine=eng)
    assert [tuple(g) for g in one] == [late[:10]]


def test_argument_checks_in_their_order(eng):
    import torch

    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(3)
    h = _dev(hashgen.random_hashes(rng, 8), np.int64)
    first = lambda *v: _dev(np.array(v, np.uint32), np.int32)
    f = first(0, 3, 8)
    out = np.zeros(16, vdf.ALIGN_STRETCH_DTYPE)
    n = C.c_size_t(99)
    torch.cuda.synchronize()
    lib = eng.lib

    def call(ctx, ah, af, n_a, bh, bf, n_b, min_run, max_stretches, guard, o=out.ctypes.data, cap=16, n_out=True):
        p = lambda t: None if t is None else t.data_ptr()
        return lib.vdf_align_windows_stretches_device(ctx, p(ah), p(af), n_a, None, p(bh), p(bf), n_b, None, 350, min_run, max_stretches, guard, o, cap,
                                                      C.byref(n) if n_out else None, None)

    err = lambda c: lib.vdf_last_error(c).decode()
    G = 2**20 + 1
    # each line breaks one more rule than the one it reports: the earlier check wins
    assert call(eng.ctx, None, f, 2, None, None, 0, 0, 0, G) == -5 and "null" in err(eng.ctx)          # a null pointer (and everything behind it)
    assert call(eng.ctx, h, f, 2, None, None, 0, 1, 0, G, n_out=False) == -5 and "null" in err(eng.ctx)
    assert call(eng.ctx, h, f, 2, None, None, 0, 1, 0, G, o=None) == -5 and "null" in err(eng.ctx)
    big = first(0, 2**20 + 1, 2**20 - 5)
    assert call(eng.ctx, h, big, 2, None, None, 0, 0, 0, G) == -5 and "min_run" in err(eng.ctx)
    assert call(eng.ctx, h, big, 2, None, None, 0, 1, 0, G) == -5 and "2^20 windows" in err(eng.ctx)   # too many windows (and a decreasing first array, ...)
    assert call(eng.ctx, h, f, 2, h, first(0, 2**20 + 1), 1, 1, 0, G) == -5 and "of B" in err(eng.ctx)
    assert call(eng.ctx, h, first(0, 5, 3), 2, None, None, 0, 1, 0, G) == -5 and "decreases" in err(eng.ctx)
    zeros = _dev(np.zeros(4098, np.uint32), np.int32)
    assert call(eng.ctx, h, zeros, 4097, h, zeros, 4097, 1, 0, G) == -5 and "2^24" in err(eng.ctx)
    for bad in (0, 9, 2**32 - 1):
        assert call(eng.ctx, h, f, 2, None, None, 0, 1, bad, G) == -5 and "max_stretches" in err(eng.ctx)  # max_stretches (and the guard)
    assert call(eng.ctx, h, f, 2, None, None, 0, 1, 8, G) == -5 and "guard" in err(eng.ctx)
    assert call(eng.ctx, h, f, 2, None, None, 0, 1, 8, 2**20) == 0 and n.value == 0
    assert call(eng.ctx, h, zeros, 4096, h, zeros, 4096, 1, 1, 0) == 0 and n.value == 0                  # 2^24 pairs of empty videos: legal, nothing to do
    # nothing to do - and still checked
    n.value = 99
    assert call(eng.ctx, h, f, 0, None, None, 0, 1, 4, 0) == 0 and n.value == 0
    n.value = 99
    assert call(eng.ctx, h, f, 1, None, None, 0, 1, 4, 0) == 0 and n.value == 0                          # self mode with one video
    assert call(eng.ctx, h, f, 1, None, None, 0, 1, 9, 0) == -5 and "max_stretches" in err(eng.ctx)
    n.value = 99
    assert call(eng.ctx, h, f, 2, h, f, 0, 1, 4, 0) == 0 and n.value == 0
    assert call(eng.ctx, h, first(0, 0, 8), 2, h, first(0, 8, 8), 2, 1, 4, 0) == 0                       # videos of 0 windows are legal
    # the host-array form reads the same checks
    hh, hf = hashgen.random_hashes(rng, 8), np.array([0, 3, 8], np.uint32)
    for kw, word in ((dict(min_run=0, max_stretches=0), "min_run"), (dict(max_stretches=0, guard=G), "max_stretches"), (dict(guard=G), "guard")):
        with pytest.raises(vdf.VdfError) as ei:
            eng.align_windows_stretches(hh, hf, **kw)
        assert ei.value.code == -5 and word in str(ei.value)
    # a multi-GPU context: the last check, in both forms
    multi = vdf.Engine(devices=[0, 0])
    try:
        assert call(multi.ctx, h, f, 2, None, None, 0, 0, 0, G) == -5 and "min_run" in err(multi.ctx)
        assert call(multi.ctx, h, f, 2, None, None, 0, 1, 0, G) == -5 and "max_stretches" in err(multi.ctx)
        assert call(multi.ctx, h, f, 2, None, None, 0, 1, 8, G) == -5 and "guard" in err(multi.ctx)
        assert call(multi.ctx, h, f, 2, None, None, 0, 1, 8, 0) == -5 and "single-device" in err(multi.ctx)
        for kw, word in ((dict(max_stretches=9), "max_stretches"), (dict(guard=G), "guard"), (dict(), "single-device")):
            with pytest.raises(vdf.VdfError) as ei:
                multi.align_windows_stretches(hh, hf, **kw)
            assert ei.value.code == -5 and word in str(ei.value)
    finally:
        multi.close()


def test_no_device_memory_is_left_behind():
    import vid_dup_finder_lib_amd as vdf

    lib = vdf._capi.load()
    before = lib.vdf_live_device_bytes()
    e = vdf.Engine(0)
    assert host_array_form(e, stretchgen.case("rect_across_bands"), 8, 2)[0] == list(stretchgen.expected("rect_across_bands", 2))
    assert device_form(e, stretchgen.case("static_self"), 8, 0)[0] == list(stretchgen.expected("static_self", 0))
    assert lib.vdf_live_device_bytes() > before
    e.close()
    assert lib.vdf_live_device_bytes() == before
