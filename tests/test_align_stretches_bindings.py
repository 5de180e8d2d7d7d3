"""The align-stretches calls' mirrors without a GPU (include/vdf.h: vdf_align_windows_stretches_host needs no context): api.align_all's mapping from
windows to frames, its default guard per stride, its order, its paths, its split above the C ABI's pair limit and its retry on a too-small buffer
- all on inputs small enough that align_all() walks them on the CPU - and what the python mirror refuses before ctypes would wrap it."""
import numpy as np
import pytest

import aligngen
import hashgen
import stretchgen
import vid_dup_finder_lib_amd as vdf
from vid_dup_finder_lib_amd import api


def library(rng, counts, plants, flips=(0, 30)):
    """per video a list of VideoHash (what hash_frame_windows returns); plants: (src video, ka, dst video, kb, n)"""
    words, first = aligngen.videos(rng, counts)
    for src, ka, dst, kb, n in plants:
        aligngen.plant(rng, words, first, src, ka, words, first, dst, kb, n, flips)
    return [[vdf.VideoHash(words[k], f"/v/{v}.mp4", 60 + v) for k in range(int(first[v]), int(first[v + 1]))] for v in range(len(counts))], words, first


def test_the_record_is_the_header_s():
    assert vdf.ALIGN_STRETCH_DTYPE.itemsize == 28 and vdf.ALIGN_STRETCH_DTYPE.names == vdf.ALIGN_DTYPE.names + ("rank",)
    assert vdf.AlignmentStretch._fields == vdf.Alignment._fields + ("rank",)


@pytest.mark.parametrize("stride", [1, 4, 16])
def test_align_all_maps_windows_to_frames(stride):
    rng = np.random.default_rng(7)
    # video 1 holds two stretches of video 0 at two offsets (an ad break removed), video 3 one
    wins, words, first = library(rng, [60, 50, 0, 20], [(0, 0, 1, 0, 20), (0, 30, 1, 20, 25), (0, 20, 3, 0, 9)])
    got = api.align_all(wins, tolerance=0.35, min_run=2, stride=stride, guard=0)  # the two stretches touch in video 1: a guard would trim the second
    assert [(g.a, g.b, g.rank) for g in got] == [(0, 1, 0), (0, 1, 1), (0, 3, 0)]
    g = got[0]
    assert (g.offset_frames, g.first_frame_a, g.first_frame_b, g.n_windows, g.n_frames) == (-10 * stride, 30 * stride, 20 * stride, 25, 24 * stride + 16)
    assert g.first_frame_b - g.first_frame_a == g.offset_frames and (g.path_a, g.path_b) == ("/v/0.mp4", "/v/1.mp4")
    dist = sum(hashgen.hamming(words[int(first[0]) + 30 + i], words[int(first[1]) + 20 + i]) for i in range(25))
    assert g.mean_distance == dist / 25
    g = got[1]
    assert (g.offset_frames, g.first_frame_a, g.first_frame_b, g.n_windows, g.n_frames, g.rank) == (0, 0, 0, 20, 19 * stride + 16, 1)
    # rank 0 is what align reports, field for field
    assert [g[:10] for g in got if g.rank == 0] == [tuple(x) for x in api.align(wins, tolerance=0.35, min_run=2, stride=stride)]
    # two libraries: B = videos 1 and 3, lists of different lengths
    got = api.align_all(wins[:1], [wins[1], wins[3]], tolerance=0.35, min_run=2, stride=stride, guard=0)
    assert [(g.a, g.b, g.rank, g.offset_frames, g.n_windows, g.path_b) for g in got] == [
        (0, 0, 0, -10 * stride, 25, "/v/1.mp4"), (0, 0, 1, 0, 20, "/v/1.mp4"), (0, 1, 0, -20 * stride, 9, "/v/3.mp4")]
    assert [g[:10] for g in api.align_all(wins, min_run=2, stride=stride, max_stretches=1)] == [tuple(x) for x in api.align(wins, min_run=2, stride=stride)]
    with pytest.raises(ValueError):
        api.align_all(wins, stride=0)
    with pytest.raises(vdf.VdfError):
        api.align_all(wins, max_stretches=9)


def test_the_default_guard_is_the_frames_two_windows_share(monkeypatch):
    rng = np.random.default_rng(11)
    wins, _, _ = library(rng, [20, 20], [(0, 2, 1, 5, 12)])
    seen = []
    real = api.align_windows_stretches_host
    monkeypatch.setattr(api, "align_windows_stretches_host", lambda *a, **k: (seen.append((k["guard"], k["max_stretches"])), real(*a, **k))[1])
    for stride, guard in ((1, 15), (2, 8), (4, 4), (5, 3), (15, 1), (16, 1), (40, 1)):
        api.align_all(wins, stride=stride)
        assert seen[-1] == (guard, 4)  # ceil(15 / stride) windows
    api.align_all(wins, stride=1, guard=0, max_stretches=7)
    assert seen[-1] == (0, 7)
    # what the guard is for: the slow walk of stretchgen, as VideoHash lists
    p = stretchgen.case("slow_content_echo")
    a = [[vdf.VideoHash(h, "/a.mp4", 1) for h in p.a_hashes]]
    b = [[vdf.VideoHash(h, "/b.mp4", 1) for h in p.b_hashes]]
    assert len(api.align_all(a, b, min_run=3, guard=0, max_stretches=8)) > 1
    only = api.align_all(a, b, min_run=3)
    assert [(g.offset_frames, g.first_frame_a, g.n_windows, g.rank) for g in only] == [(10, 20, 30, 0)]


def test_align_all_equals_the_twin_in_its_order():
    lists = lambda hashes, first, tag: [[vdf.VideoHash(hashes[k], f"/{tag}/{v}.mp4", 1) for k in range(int(first[v]), int(first[v + 1]))] for v in range(len(first) - 1)]
    for name in ("ad_removed", "repeat_in_b", "static_tiles", "skip_cuts"):
        p = stretchgen.case(name)
        static = lambda skip, first: None if skip is None else [skip[int(first[v]):int(first[v + 1])] for v in range(len(first) - 1)]
        got = api.align_all(lists(p.a_hashes, p.a_first, "a"), lists(p.b_hashes, p.b_first, "b"), min_run=p.min_run, guard=2, max_stretches=8,
                            static_a=static(p.a_skip, p.a_first), static_b=static(p.b_skip, p.b_first))
        want = stretchgen.expected(name, 2)
        assert [(g.a, g.b, g.offset_frames, g.first_frame_a, g.n_windows, round(g.mean_distance * g.n_windows), g.rank) for g in got] == list(want)
        assert [(g.a, g.b, g.rank) for g in got] == sorted((g.a, g.b, g.rank) for g in got)
        assert all(g.path_a == f"/a/{g.a}.mp4" and g.path_b == f"/b/{g.b}.mp4" for g in got)


def test_align_all_splits_above_the_pair_limit(monkeypatch):
    rng = np.random.default_rng(8)
    counts = [22, 9, 0, 15, 7, 11, 14]
    plants = [(0, 2, 1, 0, 6), (0, 12, 1, 6, 3), (0, 1, 3, 8, 7), (1, 0, 5, 4, 5), (3, 3, 6, 0, 10), (4, 0, 5, 0, 7), (5, 2, 6, 5, 8)]
    wins, _, _ = library(rng, counts, plants)
    other, _, _ = library(np.random.default_rng(8), counts, plants)  # the same videos again: B == A
    whole_self, whole_ab = api.align_all(wins, min_run=2, guard=1), api.align_all(wins, other[:5], min_run=2, guard=1)
    assert len(whole_self) >= 7 and len(whole_ab) >= 11 and any(g.rank for g in whole_self) and any(g.rank for g in whole_ab)
    calls = []
    real = api.align_windows_stretches_host
    monkeypatch.setattr(api, "align_windows_stretches_host",
                        lambda *a, **k: (calls.append((len(a[1]) - 1, None if k.get("b_first") is None else len(k["b_first"]) - 1)), real(*a, **k))[1])
    for limit, n_self, n_ab in ((4, 10, 12), (1, 28, 35), (9, 6, 6)):
        monkeypatch.setattr(api, "ALIGN_MAX_PAIRS", limit)
        del calls[:]
        assert api.align_all(wins, min_run=2, guard=1) == whole_self
        assert len(calls) == n_self and all((a * (a - 1) // 2 if b is None else a * b) <= limit for a, b in calls)
        del calls[:]
        assert api.align_all(wins, other[:5], min_run=2, guard=1) == whole_ab
        assert len(calls) == n_ab and all(b is not None and a * b <= limit for a, b in calls)


def test_align_all_retries_on_a_small_buffer(monkeypatch):
    rng = np.random.default_rng(9)
    wins, _, _ = library(rng, [10] * 6, [(0, 0, v, 1, 8) for v in range(1, 6)])
    whole = api.align_all(wins, guard=0)
    assert len(whole) >= 15
    calls = []
    real = api.align_windows_stretches_host
    monkeypatch.setattr(api, "align_windows_stretches_host", lambda *a, **k: (calls.append(k["capacity"]), real(*a, **k))[1])
    monkeypatch.setattr(api, "ALIGN_FIRST_CAPACITY", 4)
    assert api.align_all(wins, guard=0) == whole and calls == [4, len(whole)]
    del calls[:]
    monkeypatch.setattr(api, "ALIGN_FIRST_CAPACITY", len(whole))
    assert api.align_all(wins, guard=0) == whole and calls == [len(whole)]


def test_static_windows_abstain():
    rng = np.random.default_rng(10)
    wins, _, _ = library(rng, [20, 20], [(0, 2, 1, 5, 12)], flips=0)
    assert [(g.first_frame_a, g.n_windows, g.rank) for g in api.align_all(wins, guard=0)] == [(2, 12, 0)]
    flags = np.zeros(20, np.uint8)
    flags[8] = 1  # a static window in the middle of the stretch: 2 .. 7 | 9 .. 13, both halves are reported
    got = api.align_all(wins, guard=0, static_a=[flags, np.zeros(20, np.uint8)])
    assert [(g.first_frame_a, g.n_windows, g.rank) for g in got] == [(2, 6, 0), (9, 5, 1)]
    assert api.align_all(wins[:1], wins[1:], static_b=[np.ones(20, bool)]) == []


def test_python_mirror_refuses_what_ctypes_would_wrap():
    h = hashgen.random_hashes(np.random.default_rng(6), 4)
    for kw in (dict(min_run=-1), dict(tol_int=2**32), dict(max_stretches=-1), dict(guard=2**32), dict(guard=1.5)):
        with pytest.raises(ValueError):
            vdf.align_windows_stretches_host(h, [0, 4], **kw)
    for kw in (dict(min_run=0), dict(max_stretches=0), dict(max_stretches=9), dict(guard=2**20 + 1)):
        with pytest.raises(vdf.VdfError):
            vdf.align_windows_stretches_host(h, [0, 4], **kw)
