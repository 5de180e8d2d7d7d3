"""vdf_align_seed_pairs[_device] (csrc/align.hip: align_seed_kernel and its compaction) and the align calls on a list of pairs
against the numpy twin of tests/seedgen.py, pairs and records equal: the device form on device arrays and the host-array form, on the problems
tests/test_align_seed_host.py gives the plain C++ definitions - more than one tile of rows of B with a ragged last one and a video across the
edge, more than one chunk of seeds, empty videos first, last and in between, both modes; tolerance 0 and 1024 (every live pair: the contended
bitmap); min_run 1 and above every window count; skipped seeds and skipped videos; hashes on and one over the tolerance with their differing
bits in front of and behind the early exit; two problems back to back on one context; the *_pairs forms on the seed call's own output and on a
sublist; then the buffer protocol, the argument checks in their order, hash_frame_windows -> align(seed=True) end to end, device memory after
close in a fresh child process."""
import ctypes as C

import numpy as np
import pytest

import aligngen
import hashgen
import seedgen
import stretchgen
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


class OnDevice:
    """a problem's arrays as device arrays of exactly their size"""

    def __init__(self, p):
        import torch

        self.t = [_dev(p.a_hashes, np.int64), _dev(p.a_first, np.int32), _dev(p.a_skip, np.uint8), _dev(p.b_hashes, np.int64), _dev(p.b_first, np.int32),
                  _dev(p.b_skip, np.uint8)]
        torch.cuda.synchronize()
        ptr = lambda t: 0 if t is None else t.data_ptr()
        ah, af, ak, bh, bf, bk = self.t
        self.args = (ptr(ah), ptr(af), len(p.a_first) - 1)
        self.kw = dict(d_b_hashes=ptr(bh), d_b_first=ptr(bf), n_b=0 if bf is None else len(p.b_first) - 1, tol_int=p.tol, min_run=p.min_run, d_a_skip=ptr(ak),
                       d_b_skip=ptr(bk))


def host_kw(p):
    return dict(b_hashes=p.b_hashes, b_first=p.b_first, tol_int=p.tol, min_run=p.min_run, a_skip=p.a_skip, b_skip=p.b_skip)


def seed_device(eng, p, capacity=4096):
    d = OnDevice(p)
    got, found = eng.align_seed_pairs_device(*d.args, capacity=capacity, **d.kw)
    return seedgen.pairs_of(got), found


def seed_host_arrays(eng, p, capacity=4096):
    got, found = eng.align_seed_pairs(p.a_hashes, p.a_first, capacity=capacity, **host_kw(p))
    return seedgen.pairs_of(got), found


def pairs_device(eng, p, pairs, capacity=4096):
    d = OnDevice(p)
    rec, found = eng.align_windows_pairs_device(*d.args, pairs, capacity=capacity, **d.kw)
    return aligngen.records(rec), found


def pairs_host_arrays(eng, p, pairs, capacity=4096):
    rec, found = eng.align_windows_pairs(p.a_hashes, p.a_first, pairs, capacity=capacity, **host_kw(p))
    return aligngen.records(rec), found


def stretches_pairs_device(eng, p, pairs, max_stretches, guard, capacity=4096):
    d = OnDevice(p)
    rec, found = eng.align_windows_stretches_pairs_device(*d.args, pairs, max_stretches=max_stretches, guard=guard, capacity=capacity, **d.kw)
    return stretchgen.records(rec), found


def stretches_pairs_host_arrays(eng, p, pairs, max_stretches, guard, capacity=4096):
    rec, found = eng.align_windows_stretches_pairs(p.a_hashes, p.a_first, pairs, max_stretches=max_stretches, guard=guard, capacity=capacity, **host_kw(p))
    return stretchgen.records(rec), found


# tile and chunk edges in both modes; tolerance 0 and 1024; min_run 1 and above every window count; skip bytes; the early exit; the phases of a run
@pytest.mark.parametrize("name", sorted(seedgen.BUILDERS))
def test_seed_kernel_matches_the_twin(eng, name):
    p, want = seedgen.case(name), list(seedgen.expected(name))
    got, found = seed_device(eng, p)
    print(f"{name}: {len(want)} candidate pairs, device form found {found}")
    assert found == len(want)
    assert got == want
    got, found = seed_host_arrays(eng, p)
    assert found == len(want) and got == want


@pytest.mark.parametrize("name", ["mixed_counts", "self_mode", "skip_cuts", "skip_silences", "static_self", "static_a_shorter", "tolerance_0", "tolerance_350",
                                  "tolerance_5000", "min_run_16"])
def test_seed_kernel_on_the_align_cases(eng, name):
    p = aligngen.case(name)
    want = seedgen.seed_twin(p)
    assert seed_device(eng, p) == (want, len(want))
    assert {(r[0], r[1]) for r in aligngen.expected(name)} <= set(want)


def test_early_exit_hits_and_misses(eng):
    """on the tolerance with the differing bits behind the exit, on it with them in front, one over it with nothing to see at the exit"""
    for name in ("early_exit", "early_exit_tol_100"):
        assert seed_device(eng, seedgen.case(name))[0] == [(0, 0), (1, 1)]


def test_no_stale_bits_between_calls(eng):
    """two different problems back to back on one context give what fresh contexts give: the bitmap is cleared by every call"""
    import vid_dup_finder_lib_amd as vdf

    dense, sparse = seedgen.case("tile_edges_all"), seedgen.case("tile_edges")   # the same shape: every bit of the second call was set by the first
    assert seed_device(eng, dense)[0] == list(seedgen.expected("tile_edges_all"))
    assert seed_device(eng, sparse)[0] == list(seedgen.expected("tile_edges"))
    assert seed_host_arrays(eng, seedgen.case("tile_edges_self_all"))[0] == list(seedgen.expected("tile_edges_self_all"))
    assert seed_host_arrays(eng, seedgen.case("skipped_seeds"))[0] == [(3, 4)]
    fresh = vdf.Engine(0)
    try:
        assert seed_device(fresh, sparse)[0] == list(seedgen.expected("tile_edges"))
    finally:
        fresh.close()


@pytest.mark.parametrize("name", ["tile_edges", "tile_edges_self"])
def test_pairs_forms_on_the_seed_call_s_output_and_on_a_sublist(eng, name):
    p = seedgen.case(name)
    cand, _ = seed_device(eng, p)
    whole = list(seedgen.expected_records(name))
    rec, found = eng.align_windows(p.a_hashes, p.a_first, capacity=4096, **host_kw(p))
    assert aligngen.records(rec) == whole                                   # the all-pairs call itself
    assert pairs_device(eng, p, cand) == (whole, len(whole))
    assert pairs_host_arrays(eng, p, cand) == (whole, len(whole))
    st, found = eng.align_windows_stretches(p.a_hashes, p.a_first, max_stretches=8, guard=1, capacity=4096, **host_kw(p))
    whole_st = stretchgen.records(st)
    assert found == len(whole_st) and whole_st == stretchgen.stretches_twin(p, 8, 1)
    assert stretches_pairs_device(eng, p, cand, 8, 1) == (whole_st, len(whole_st))
    assert stretches_pairs_host_arrays(eng, p, cand, 8, 1) == (whole_st, len(whole_st))
    sub = seedgen.sublist(p, 5)
    part = [r for r in whole if (r[0], r[1]) in set(sub)]
    assert 0 < len(part) < len(whole)
    assert pairs_device(eng, p, sub)[0] == part and pairs_host_arrays(eng, p, sub)[0] == part
    part_st = [r for r in whole_st if (r[0], r[1]) in set(sub)]
    assert stretches_pairs_device(eng, p, sub, 8, 1)[0] == part_st and stretches_pairs_host_arrays(eng, p, sub, 8, 1)[0] == part_st
    assert pairs_device(eng, p, []) == ([], 0)


def test_capacity_smaller_than_the_result(eng):
    p, want = seedgen.case("tile_edges"), list(seedgen.expected("tile_edges"))
    recs = list(seedgen.expected_records("tile_edges"))
    assert len(want) > 5 and len(recs) > 5
    for seed, pairs, stretches in ((seed_device, pairs_device, stretches_pairs_device), (seed_host_arrays, pairs_host_arrays, stretches_pairs_host_arrays)):
        for cap in (5, 0, len(want)):
            got, found = seed(eng, p, capacity=cap)
            assert found == len(want) and got == want[:cap]  # the count is right and the prefix is valid
        for cap in (5, 0, len(recs)):
            got, found = pairs(eng, p, want, capacity=cap)
            assert found == len(recs) and got == recs[:cap]
            got, found = stretches(eng, p, want, 1, 0, capacity=cap)
            assert found == len(recs) and [r[:6] for r in got] == recs[:cap]


def test_end_to_end_trimmed_reupload(eng):
    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(41)
    v0 = windowgen.video(rng, 80, 64, 64)
    v1 = np.concatenate([v0[23:], rng.integers(0, 256, size=(23, 64, 64), dtype=np.uint8)])  # the re-upload: frames 23 .. 79 of video 0, then something else
    v2 = windowgen.video(np.random.default_rng(42), 80, 64, 64, lead=9)
    videos = np.stack([v0, v1, v2])
    windows = vdf.hash_frame_windows(videos, ["a.mp4", "b.mp4", "c.mp4"], [80, 80, 80], stride=1, engine=eng)
    plain = vdf.align(windows, min_run=4, engine=eng)
    seeded = vdf.align(windows, min_run=4, engine=eng, seed=True)
    assert seeded == plain and (plain[0].a, plain[0].b, plain[0].offset_frames, plain[0].n_windows) == (0, 1, -23, 42)
    cand = vdf.candidate_pairs(windows, min_run=4, engine=eng)
    assert {(g.a, g.b) for g in plain} <= set(cand)
    words = np.stack([h.hash for ws in windows for h in ws])
    assert cand == seedgen.seed_twin(aligngen.Problem(words, aligngen.first_of([65, 65, 65]), None, None, 350, 4))
    assert vdf.align_all(windows, min_run=4, engine=eng, seed=True) == vdf.align_all(windows, min_run=4, engine=eng)
    assert vdf.align(windows, min_run=4, engine=eng, pairs=[(0, 1)]) == [g for g in plain if (g.a, g.b) == (0, 1)]


def test_argument_checks_in_their_order(eng):
    import torch

    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(3)
    h = _dev(hashgen.random_hashes(rng, 8), np.int64)
    first = lambda *v: _dev(np.array(v, np.uint32), np.int32)
    f = first(0, 3, 8)
    out = np.zeros(16, vdf.ALIGN_STRETCH_DTYPE)  # room for 16 records of any of the three calls
    n = C.c_size_t(99)
    torch.cuda.synchronize()
    lib = eng.lib
    p = lambda t: None if t is None else t.data_ptr()
    err = lambda c: lib.vdf_last_error(c).decode()

    def seed(ctx, ah, af, n_a, bh, bf, n_b, min_run, o=out.ctypes.data, cap=16, n_out=True):
        return lib.vdf_align_seed_pairs_device(ctx, p(ah), p(af), n_a, None, p(bh), p(bf), n_b, None, 350, min_run, o, cap, C.byref(n) if n_out else None, None)

    # the seed call: the align calls' checks, in their order
    assert seed(eng.ctx, None, f, 2, None, None, 0, 0) == -5 and "null" in err(eng.ctx)
    assert seed(eng.ctx, h, f, 2, None, None, 0, 1, n_out=False) == -5 and "null" in err(eng.ctx)
    assert seed(eng.ctx, h, f, 2, None, None, 0, 1, o=None) == -5 and "null" in err(eng.ctx)
    big = first(0, 2**20 + 1, 2**20 - 5)
    assert seed(eng.ctx, h, big, 2, None, None, 0, 0) == -5 and "min_run" in err(eng.ctx)
    assert seed(eng.ctx, h, big, 2, None, None, 0, 1) == -5 and "2^20" in err(eng.ctx)
    assert seed(eng.ctx, h, first(0, 5, 3), 2, None, None, 0, 1) == -5 and "decreases" in err(eng.ctx)
    zeros = _dev(np.zeros(4098, np.uint32), np.int32)
    assert seed(eng.ctx, h, zeros, 4097, h, zeros, 4097, 1) == -5 and "2^24 pairs of videos" in err(eng.ctx)
    assert seed(eng.ctx, h, zeros, 4096, h, zeros, 4096, 1) == 0 and n.value == 0     # 2^24 pairs of empty videos: legal, nothing to do
    for args in ((h, f, 0, None, None, 0), (h, f, 1, None, None, 0), (h, f, 2, h, f, 0)):
        n.value = 99
        assert seed(eng.ctx, *args, 1) == 0 and n.value == 0

    # the *_pairs calls: a null list first, the align checks, the stretches checks, the list, the multi-GPU refusal last
    good = np.array([(0, 1)], vdf.VIDEO_PAIR_DTYPE)
    unsorted = np.array([(0, 1), (0, 1)], vdf.VIDEO_PAIR_DTYPE)
    beyond = np.array([(0, 2)], vdf.VIDEO_PAIR_DTYPE)
    diag = np.array([(1, 1)], vdf.VIDEO_PAIR_DTYPE)

    def pairs(ctx, af, n_a, bh, lst, n_list, min_run):
        return lib.vdf_align_windows_pairs_device(ctx, p(h), p(af), n_a, None, p(bh), p(af) if bh is not None else None, n_a if bh is not None else 0, None,
                                                  None if lst is None else lst.ctypes.data, n_list, 350, min_run, out.ctypes.data, 16, C.byref(n), None)

    def stretches(ctx, af, n_a, lst, n_list, min_run, max_stretches, guard):
        return lib.vdf_align_windows_stretches_pairs_device(ctx, p(h), p(af), n_a, None, None, None, 0, None, None if lst is None else lst.ctypes.data, n_list,
                                                            350, min_run, max_stretches, guard, out.ctypes.data, 16, C.byref(n), None)

    assert pairs(eng.ctx, f, 2, None, None, 1, 0) == -5 and "null pair list" in err(eng.ctx)               # (and min_run == 0)
    assert pairs(eng.ctx, f, 2, None, unsorted, 2, 0) == -5 and "min_run" in err(eng.ctx)                  # (and an unsorted list)
    assert pairs(eng.ctx, f, 2, None, unsorted, (1 << 24) + 1, 1) == -5 and "2^24 listed pairs" in err(eng.ctx)
    assert pairs(eng.ctx, f, 2, None, unsorted, 2, 1) == -5 and "strictly increasing" in err(eng.ctx)
    assert pairs(eng.ctx, f, 2, None, beyond, 1, 1) == -5 and "does not exist" in err(eng.ctx)
    assert pairs(eng.ctx, f, 2, None, diag, 1, 1) == -5 and "a >= b in self mode" in err(eng.ctx)
    assert pairs(eng.ctx, f, 2, h, diag, 1, 1) == 0                                                         # fine between two sets
    assert pairs(eng.ctx, first(0, 5, 3), 2, None, good, 1, 1) == -5 and "decreases" in err(eng.ctx)       # the first arrays, once they are down
    assert pairs(eng.ctx, zeros, 4097, h, good, 1, 1) == 0 and n.value == 0                                 # 4097 x 4097 videos: the limit is on the list
    assert pairs(eng.ctx, zeros, 2**32, h, unsorted, (1 << 24) + 1, 1) == -5 and "does not fit 32 bits" in err(eng.ctx)   # (and too long a list; nothing is read)
    n.value = 99
    assert pairs(eng.ctx, f, 2, None, None, 0, 1) == 0 and n.value == 0
    assert stretches(eng.ctx, f, 2, unsorted, 2, 0, 9, 0) == -5 and "min_run" in err(eng.ctx)
    assert stretches(eng.ctx, f, 2, unsorted, 2, 1, 9, 2**20 + 1) == -5 and "max_stretches" in err(eng.ctx)
    assert stretches(eng.ctx, f, 2, unsorted, 2, 1, 8, 2**20 + 1) == -5 and "guard" in err(eng.ctx)
    assert stretches(eng.ctx, f, 2, unsorted, 2, 1, 8, 0) == -5 and "strictly increasing" in err(eng.ctx)
    assert stretches(eng.ctx, f, 2, good, 1, 1, 8, 0) == 0
    multi = vdf.Engine(devices=[0, 0])
    try:
        assert seed(multi.ctx, h, f, 2, None, None, 0, 0) == -5 and "min_run" in err(multi.ctx)
        assert seed(multi.ctx, h, f, 2, None, None, 0, 1) == -5 and "single-device" in err(multi.ctx)
        assert pairs(multi.ctx, f, 2, None, unsorted, 2, 1) == -5 and "strictly increasing" in err(multi.ctx)
        assert pairs(multi.ctx, f, 2, None, good, 1, 1) == -5 and "single-device" in err(multi.ctx)
        assert stretches(multi.ctx, f, 2, good, 1, 1, 8, 2**20 + 1) == -5 and "guard" in err(multi.ctx)
        assert stretches(multi.ctx, f, 2, good, 1, 1, 8, 0) == -5 and "single-device" in err(multi.ctx)
        words = hashgen.random_hashes(rng, 8)
        for call in (lambda: multi.align_seed_pairs(words, [0, 3, 8]), lambda: multi.align_windows_pairs(words, [0, 3, 8], [(0, 1)]),
                     lambda: multi.align_windows_stretches_pairs(words, [0, 3, 8], [(0, 1)])):
            with pytest.raises(vdf.VdfError) as ei:
                call()
            assert ei.value.code == -5 and "single-device" in str(ei.value)
    finally:
        multi.close()


CHILD = """
import sys
sys.path.insert(0, {tests!r})
import seedgen
import vid_dup_finder_lib_amd as vdf
from test_gpu_align_seed import pairs_host_arrays, seed_device, seed_host_arrays, stretches_pairs_host_arrays

lib = vdf._capi.load()
assert lib.vdf_live_device_bytes() == 0      # a fresh process: no other engine is alive
e = vdf.Engine(0)
p = seedgen.case("tile_edges_self")
cand, _ = seed_host_arrays(e, p)
assert cand == list(seedgen.expected("tile_edges_self"))
assert pairs_host_arrays(e, p, cand)[0] == list(seedgen.expected_records("tile_edges_self"))
assert len(stretches_pairs_host_arrays(e, p, cand, 2, 1)[0]) >= len(seedgen.expected_records("tile_edges_self"))
assert seed_device(e, seedgen.case("tile_edges"))[0] == list(seedgen.expected("tile_edges"))
held = lib.vdf_live_device_bytes()
e.close()
print("LIVE", held, lib.vdf_live_device_bytes())
"""


def test_no_device_memory_is_left_behind():
    """in a fresh child process, where no other engine - this module's fixture, another test's default engine - holds device memory: the
    library's count of live device bytes is 0 before the engine, above 0 after the seed call, the pairs calls and their buffers (bitmap, plan,
    dense pairs), and 0 again after close"""
    import os
    import subprocess
    import sys

    tests = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, "-c", CHILD.format(tests=tests)], cwd=os.path.dirname(tests), capture_output=True, text=True, timeout=300)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("LIVE ")]
    assert out.returncode == 0 and line, out.stdout[-2000:] + out.stderr[-3000:]
    held, after = (int(x) for x in line[-1].split()[1:])
    assert held > 0 and after == 0
