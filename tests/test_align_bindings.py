"""The align calls' mirrors without a GPU (include/vdf.h: vdf_align_windows_host needs no context): the argument checks through ctypes, and
api.align's mapping from windows to frames, its split above the C ABI's pair limit and its retry on a too-small buffer - all on inputs small
enough that align() walks them on the CPU."""
import ctypes as C

import numpy as np
import pytest

import aligngen
import hashgen
import vid_dup_finder_lib_amd as vdf
from vid_dup_finder_lib_amd import _capi, api


def call_host(a_hashes, a_first, n_a, b_hashes=None, b_first=None, n_b=0, min_run=1, capacity=8, n_out=True, out=True, a_skip=None, b_skip=None):
    lib = _capi.load()
    buf = np.zeros(max(capacity, 1), vdf.ALIGN_DTYPE)
    n = C.c_size_t(12345)
    ptr = lambda x: None if x is None else x.ctypes.data
    rc = lib.vdf_align_windows_host(ptr(a_hashes), ptr(a_first), n_a, ptr(a_skip), ptr(b_hashes), ptr(b_first), n_b, ptr(b_skip), 350, min_run,
                                    buf.ctypes.data if out else None, capacity, C.byref(n) if n_out else None)
    return rc, n.value


def test_host_form_argument_checks():
    rng = np.random.default_rng(5)
    h = hashgen.random_hashes(rng, 6)
    f = np.array([0, 2, 6], np.uint32)
    assert call_host(h, f, 2) == (_capi.VDF_OK, 0)
    assert call_host(h, f, 2, h, f, 2)[0] == _capi.VDF_OK
    # a null required pointer
    assert call_host(h, f, 2, n_out=False)[0] == _capi.VDF_E_INVAL
    assert call_host(None, f, 2)[0] == _capi.VDF_E_INVAL
    assert call_host(h, None, 2)[0] == _capi.VDF_E_INVAL
    assert call_host(h, f, 2, h, None, 2)[0] == _capi.VDF_E_INVAL
    assert call_host(h, f, 2, out=False)[0] == _capi.VDF_E_INVAL
    assert call_host(h, f, 2, out=False, capacity=0)[0] == _capi.VDF_OK  # counting only
    # min_run of zero
    assert call_host(h, f, 2, min_run=0)[0] == _capi.VDF_E_INVAL
    # a video of more than 2^20 windows (nothing is read: the check comes before the walk)
    assert call_host(h, np.array([0, 2, 2 + 2**20 + 1], np.uint32), 2)[0] == _capi.VDF_E_INVAL
    assert call_host(h, f, 2, h, np.array([0, 2**20 + 1], np.uint32), 1)[0] == _capi.VDF_E_INVAL
    # a first array that decreases
    assert call_host(h, np.array([0, 5, 3], np.uint32), 2)[0] == _capi.VDF_E_INVAL
    assert call_host(h, f, 2, h, np.array([4, 3, 6], np.uint32), 2)[0] == _capi.VDF_E_INVAL
    # more than 2^24 pairs: 4097 x 4097 videos, and 5794 videos against themselves (5794 * 5793 / 2 > 2^24 >= 5793 * 5792 / 2)
    zeros = np.zeros(5795, np.uint32)
    assert call_host(h, zeros, 4097, h, zeros, 4097)[0] == _capi.VDF_E_INVAL
    assert call_host(h, zeros, 4096, h, zeros, 4096) == (_capi.VDF_OK, 0)
    assert call_host(h, zeros, 5794)[0] == _capi.VDF_E_INVAL
    assert call_host(h, zeros, 5793) == (_capi.VDF_OK, 0)
    # nothing to do
    assert call_host(h, f, 0) == (_capi.VDF_OK, 0)
    assert call_host(h, f, 2, h, f, 0) == (_capi.VDF_OK, 0)
    assert call_host(h, f, 1) == (_capi.VDF_OK, 0)  # self mode with one video
    assert call_host(h, np.array([0, 0, 6], np.uint32), 2, h, np.array([0, 6, 6], np.uint32), 2)[0] == _capi.VDF_OK  # videos of 0 windows


def test_python_mirror_refuses_what_ctypes_would_wrap():
    h = hashgen.random_hashes(np.random.default_rng(6), 4)
    with pytest.raises(ValueError):
        vdf.align_windows_host(h, [0, 4], min_run=-1)
    with pytest.raises(ValueError):
        vdf.align_windows_host(h, [0, 4], tol_int=2**32)
    with pytest.raises(ValueError):
        vdf.align_windows_host(h, [0, 5])  # first points behind the hashes
    with pytest.raises(ValueError):
        vdf.align_windows_host(h, [0, 4], a_skip=np.zeros(3, np.uint8))
    with pytest.raises(vdf.VdfError):
        vdf.align_windows_host(h, [0, 4], min_run=0)


def library(rng, counts, plants, flips=(0, 30)):
    """per video a list of VideoHash (what hash_frame_windows returns); plants: (src video, ka, dst video, kb, n)"""
    words, first = aligngen.videos(rng, counts)
    for src, ka, dst, kb, n in plants:
        aligngen.plant(rng, words, first, src, ka, words, first, dst, kb, n, flips)
    return [[vdf.VideoHash(words[k], f"/v/{v}.mp4", 60 + v) for k in range(int(first[v]), int(first[v + 1]))] for v in range(len(counts))], words, first


@pytest.mark.parametrize("stride", [1, 4, 16])
def test_align_maps_windows_to_frames(stride):
    rng = np.random.default_rng(7)
    wins, words, first = library(rng, [30, 50, 0, 20], [(0, 4, 1, 27, 12), (0, 20, 3, 0, 9)])
    got = api.align(wins, tolerance=0.35, min_run=2, stride=stride)
    assert [(g.a, g.b) for g in got] == [(0, 1), (0, 3)]
    g = got[0]
    assert (g.offset_frames, g.first_frame_a, g.first_frame_b, g.n_windows, g.n_frames) == (23 * stride, 4 * stride, 27 * stride, 12, 11 * stride + 16)
    assert g.first_frame_b - g.first_frame_a == g.offset_frames and (g.path_a, g.path_b) == ("/v/0.mp4", "/v/1.mp4")
    dist = sum(hashgen.hamming(words[int(first[0]) + 4 + i], words[int(first[1]) + 27 + i]) for i in range(12))
    assert g.mean_distance == dist / 12
    g = got[1]
    assert (g.offset_frames, g.first_frame_a, g.first_frame_b, g.n_windows, g.n_frames) == (-20 * stride, 20 * stride, 0, 9, 8 * stride + 16)
    # two libraries: B = videos 1 and 3, lists of different lengths
    got = api.align(wins[:1], [wins[1], wins[3]], tolerance=0.35, stride=stride)
    assert [(g.a, g.b, g.offset_frames, g.n_windows, g.path_b) for g in got] == [(0, 0, 23 * stride, 12, "/v/1.mp4"), (0, 1, -20 * stride, 9, "/v/3.mp4")]
    with pytest.raises(ValueError):
        api.align(wins, stride=0)


def test_align_splits_above_the_pair_limit(monkeypatch):
    rng = np.random.default_rng(8)
    counts = [12, 9, 0, 15, 7, 11, 14]
    plants = [(0, 2, 1, 0, 6), (0, 1, 3, 8, 7), (1, 0, 5, 4, 5), (3, 3, 6, 0, 10), (4, 0, 5, 0, 7), (5, 2, 6, 5, 8)]
    wins, _, _ = library(rng, counts, plants)
    other, _, _ = library(np.random.default_rng(8), counts, plants)  # the same videos again: B == A
    whole_self, whole_ab = api.align(wins, min_run=2), api.align(wins, other[:5], min_run=2)
    assert len(whole_self) >= 6 and len(whole_ab) >= 10
    calls = []
    real = api.align_windows_host
    monkeypatch.setattr(api, "align_windows_host", lambda *a, **k: (calls.append((len(a[1]) - 1, None if k.get("b_first") is None else len(k["b_first"]) - 1)), real(*a, **k))[1])
    for limit, n_self, n_ab in ((4, 10, 12), (1, 28, 35), (9, 6, 6)):
        monkeypatch.setattr(api, "ALIGN_MAX_PAIRS", limit)
        del calls[:]
        assert api.align(wins, min_run=2) == whole_self
        assert len(calls) == n_self and all((a * (a - 1) // 2 if b is None else a * b) <= limit for a, b in calls)
        del calls[:]
        assert api.align(wins, other[:5], min_run=2) == whole_ab
        assert len(calls) == n_ab and all(b is not None and a * b <= limit for a, b in calls)


def test_align_retries_on_a_small_buffer(monkeypatch):
    rng = np.random.default_rng(9)
    wins, _, _ = library(rng, [10] * 6, [(0, 0, v, 1, 8) for v in range(1, 6)])
    whole = api.align(wins)
    assert len(whole) == 15  # every video holds the stretch: every pair shares it
    calls = []
    real = api.align_windows_host
    monkeypatch.setattr(api, "align_windows_host", lambda *a, **k: (calls.append(k["capacity"]), real(*a, **k))[1])
    monkeypatch.setattr(api, "ALIGN_FIRST_CAPACITY", 4)
    assert api.align(wins) == whole and calls == [4, 15]
    del calls[:]
    monkeypatch.setattr(api, "ALIGN_FIRST_CAPACITY", 15)
    assert api.align(wins) == whole and calls == [15]


def test_static_windows_abstain():
    rng = np.random.default_rng(10)
    wins, words, first = library(rng, [20, 20], [(0, 2, 1, 5, 12)], flips=0)
    assert [(g.first_frame_a, g.n_windows) for g in api.align(wins)] == [(2, 12)]
    dc = np.zeros(20, np.uint32)
    dc[8] = 900   # a static window in the middle of the stretch
    dc[3] = 899   # not static
    flags = api.static_windows(dc)
    assert flags.dtype == np.uint8 and flags.tolist() == [0] * 8 + [1] + [0] * 11
    got = api.align(wins, static_a=[flags, np.zeros(20, np.uint8)])
    assert [(g.first_frame_a, g.n_windows) for g in got] == [(2, 6)]  # 2 .. 7 | 9 .. 13: the longer half
    got = api.align(wins[:1], wins[1:], static_b=[np.ones(20, bool)])
    assert got == []
    with pytest.raises(ValueError):
        api.align(wins, static_a=[flags])
