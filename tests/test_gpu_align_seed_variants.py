"""vdf_align_seed_pairs_variants[_device] (csrc/align.hip: align_class_layout_kernel, align_seed_variants_kernel and its compaction; DESIGN.md
4.14) and vdf_align_windows_variants_pairs[_device] against the numpy twin of tests/seedvariantgen.py, triples and records equal: the device form
on device arrays and the host-array form, on the problems tests/test_align_seed_variants_host.py gives the plain C++ definitions - more than four
tiles of 256 rows of B with a ragged last one and videos across the edges, more than one chunk of seeds, empty videos, both modes; tolerance 0
and 1024 (every live pair under every variant: the contended bitmap); min_run 1 and above every window count; skip bytes; sparse, dense and
static planes; hashes on and one over the tolerance under a variant with the deciding bits in the last class streamed, in a flipped class and
among the padding bits; a pair that is a candidate under one variant only; two problems back to back on one context; the list form on the seed
call's own output and on a sublist; the layout kernel's rows equal to its host twin's word for word; then the capacity protocol, the argument checks in their order, hash_frame_windows -> align_flipped(seed=True)
end to end, device memory after close in a fresh child process."""
import ctypes as C

import numpy as np
import pytest

import hashgen
import seedvariantgen as svg
import variantgen

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

    def __init__(self, vp):
        import torch

        p = vp.p
        self.t = [_dev(p.a_hashes, np.int64), _dev(p.a_first, np.int32), _dev(p.a_skip, np.uint8), _dev(p.b_hashes, np.int64), _dev(p.b_first, np.int32),
                  _dev(p.b_skip, np.uint8), _dev(vp.a_zero, np.int64), _dev(vp.b_zero, np.int64)]
        torch.cuda.synchronize()
        ptr = lambda t: 0 if t is None else t.data_ptr()
        ah, af, ak, bh, bf, bk, az, bz = self.t
        self.args = (ptr(ah), ptr(af), len(p.a_first) - 1)
        self.kw = dict(d_a_zero=ptr(az), d_b_hashes=ptr(bh), d_b_first=ptr(bf), n_b=0 if bf is None else len(p.b_first) - 1, d_b_zero=ptr(bz), tol_int=p.tol,
                       min_run=p.min_run, d_a_skip=ptr(ak), d_b_skip=ptr(bk))


def _host_kw(kw):
    return {k: v for k, v in kw.items() if k not in ("a_hashes", "a_first")}


def seed_device(eng, vp, mask=None, capacity=1 << 16):
    d = OnDevice(vp)
    got, found = eng.align_seed_pairs_variants_device(*d.args, variant_mask=vp.mask if mask is None else mask, capacity=capacity, **d.kw)
    return svg.triples_of(got), found


def seed_host_arrays(eng, vp, mask=None, capacity=1 << 16):
    kw = svg.call_args(vp, mask)
    got, found = eng.align_seed_pairs_variants(kw["a_hashes"], kw["a_first"], capacity=capacity, **_host_kw(kw))
    return svg.triples_of(got), found


def _triples(eng_vdf, triples):
    return np.array([(a, b, v) for v, a, b in triples], eng_vdf.VIDEO_PAIR_VARIANT_DTYPE)


def pairs_device(eng, vp, triples, capacity=1 << 16):
    import vid_dup_finder_lib_amd as vdf

    d = OnDevice(vp)
    rec, found = eng.align_windows_variants_pairs_device(*d.args, _triples(vdf, triples), capacity=capacity, **d.kw)
    return variantgen.records(rec), found


def pairs_host_arrays(eng, vp, triples, capacity=1 << 16):
    import vid_dup_finder_lib_amd as vdf

    kw = svg.list_args(vp)
    rec, found = eng.align_windows_variants_pairs(kw["a_hashes"], kw["a_first"], _triples(vdf, triples), capacity=capacity, **_host_kw(kw))
    return variantgen.records(rec), found


@pytest.mark.parametrize("name", sorted(svg.BUILDERS))
def test_seed_kernel_matches_the_twin(eng, name):
    vp, want = svg.case(name), list(svg.expected(name))
    got, found = seed_device(eng, vp)
    print(f"{name}: mask {vp.mask:#010b}, {len(want)} candidate triples, device form found {found}")
    assert found == len(want)
    assert got == want
    got, found = seed_host_arrays(eng, vp)
    assert found == len(want) and got == want


def test_on_and_one_over_the_tolerance_under_a_variant(eng):
    for name in ("on_the_tolerance", "on_the_tolerance_100"):
        vp = svg.case(name)
        got = set(seed_device(eng, vp)[0])
        for i in range(len(vp.p.a_first) - 1):
            assert ((1 + i // 12, i, i) in got) == (i % 2 == 0), (name, i)


def test_candidate_under_one_variant_only(eng):
    got5 = seed_device(eng, svg.case("only_under_5"))[0]
    assert (5, 0, 1) in got5 and not {(1, 0, 1), (4, 0, 1)} & set(got5)
    for v in (1, 4):
        got = seed_device(eng, svg.case(f"only_under_{v}"))[0]
        assert (v, 0, 1) in got and (5, 0, 1) not in got


@pytest.mark.parametrize("min_run", [1, 3, 300])
def test_layout_kernel_equals_its_host_twin_word_for_word(eng, min_run):
    """align_class_layout_kernel through vdf_window_class_layout_device against vdf_window_class_layout_host, all 36 dwords of every seed and all
    72 of every row: a set that begins behind row 0, empty and one-window videos, skip bytes, 772 rows (three full workgroups of rows and a
    ragged one), arbitrary words; nothing is written behind the last row"""
    import torch

    import vid_dup_finder_lib_amd as vdf

    hashes, zero, first, skip = svg.layout_problem()
    d_h, d_z, d_f, d_s = _dev(hashes, np.int64), _dev(zero, np.int64), _dev(first, np.int32), _dev(skip, np.uint8)
    for sk, d_sk in ((None, None), (skip, d_s)):
        for z, d_zz, width in ((None, None, 36), (zero, d_z, 72)):
            want = vdf.window_class_layout_host(hashes, first, zero=z, skip=sk, min_run=min_run)
            assert np.array_equal(want, svg.class_layout_twin(hashes, first, z, sk, min_run)) and len(want)
            room = len(want) + 3
            d_out = torch.full((room, width), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            n = eng.window_class_layout_device(d_h.data_ptr(), d_f.data_ptr(), len(first) - 1, d_out.data_ptr(), room, d_zero=0 if d_zz is None else d_zz.data_ptr(),
                                               d_skip=0 if d_sk is None else d_sk.data_ptr(), min_run=min_run)
            got = d_out.cpu().numpy().view(np.uint32)
            assert n == len(want)
            assert np.array_equal(got[:n], want)
            assert (got[n:] == 0x5A5A5A5A).all()
    with pytest.raises(vdf.VdfError, match="fewer rows"):
        eng.window_class_layout_device(d_h.data_ptr(), d_f.data_ptr(), len(first) - 1, d_out.data_ptr(), 5, d_zero=d_z.data_ptr())


def test_no_stale_bits_between_calls(eng):
    """a tol-1024 problem at all seven variants, then a sparse problem of the same shape at one: the bitmap's requested slots are cleared by every call"""
    import vid_dup_finder_lib_amd as vdf

    dense, sparse = svg.case("tile_edges_all"), svg.case("tile_edges_no_planes")   # both from seedgen's tile_edges shape
    assert sparse.mask == 0b00000010 and dense.mask == svg.ALL
    assert [len(x) for x in (dense.p.a_first, dense.p.b_first)] == [len(x) for x in (sparse.p.a_first, sparse.p.b_first)]
    assert seed_device(eng, dense)[0] == list(svg.expected("tile_edges_all"))
    assert seed_device(eng, sparse)[0] == list(svg.expected("tile_edges_no_planes"))
    assert seed_host_arrays(eng, svg.case("tile_edges_self_all"))[0] == list(svg.expected("tile_edges_self_all"))
    assert seed_host_arrays(eng, svg.case("skipped_seeds"))[0] == list(svg.expected("skipped_seeds"))
    fresh = vdf.Engine(0)
    try:
        assert seed_device(fresh, sparse)[0] == list(svg.expected("tile_edges_no_planes"))
    finally:
        fresh.close()


@pytest.mark.parametrize("name", ["tile_edges", "tile_edges_self"])
def test_list_form_on_the_seed_call_s_output_and_on_a_sublist(eng, name):
    vp = svg.case(name)
    cand, _ = seed_device(eng, vp)
    d = OnDevice(vp)
    rec, found = eng.align_windows_variants_device(*d.args, variant_mask=vp.mask, capacity=1 << 16, **d.kw)
    whole = variantgen.records(rec)
    assert found == len(whole) > 0 and whole == list(svg.expected_records(name))          # the all-pairs variants call itself
    assert pairs_device(eng, vp, cand) == (whole, len(whole))
    assert pairs_host_arrays(eng, vp, cand) == (whole, len(whole))
    sub = cand[::2]
    part = [r for r in whole if r[:3] in set(sub)]
    assert 0 < len(part) < len(whole)
    assert pairs_device(eng, vp, sub)[0] == part and pairs_host_arrays(eng, vp, sub)[0] == part
    assert pairs_device(eng, vp, []) == ([], 0)


def test_capacity_smaller_than_the_result(eng):
    vp, want = svg.case("tile_edges"), list(svg.expected("tile_edges"))
    recs = list(svg.expected_records("tile_edges"))
    assert len(want) > 5 and len(recs) > 5
    for seed, pairs in ((seed_device, pairs_device), (seed_host_arrays, pairs_host_arrays)):
        for cap in (5, 0, len(want)):
            got, found = seed(eng, vp, capacity=cap)
            assert found == len(want) and got == want[:cap]  # the count is right and the prefix is valid
        for cap in (5, 0, len(recs)):
            got, found = pairs(eng, vp, want, capacity=cap)
            assert found == len(recs) and got == recs[:cap]


def test_end_to_end_a_mirrored_reversed_and_trimmed_reupload(eng):
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd import Flip

    rng = np.random.default_rng(41)
    a = rng.integers(0, 256, size=(80, 16, 16), dtype=np.uint8)
    noise = lambda n: rng.integers(0, 256, size=(n, 16, 16), dtype=np.uint8)
    b = np.ascontiguousarray(np.concatenate([noise(3), a[10:50][::-1, :, ::-1], noise(5)]))  # frames 10 ... 49 of a mirrored and played backwards, trimmed
    c = noise(64)
    windows = [vdf.hash_frame_windows(v[None], [name], [len(v)], stride=1, engine=eng, zero_plane=True)[0] for v, name in ((a, "a.mp4"), (b, "b.mp4"), (c, "c.mp4"))]
    flips = [Flip.X, Flip.T, Flip.X | Flip.T]
    for tolerance in (0.0, vdf.DEFAULT_SEARCH_TOLERANCE):
        plain = vdf.align_flipped(windows, tolerance=tolerance, min_run=4, flips=flips, engine=eng)
        assert (0, 1) in [(g.a, g.b) for g in plain[Flip.X | Flip.T]]
        if tolerance == 0.0:
            assert plain[Flip.X] == [] and plain[Flip.T] == [] and len(plain[Flip.X | Flip.T]) == 1
        assert vdf.align_flipped(windows, tolerance=tolerance, min_run=4, flips=flips, engine=eng, seed=True) == plain
        cand = vdf.candidate_pairs_flipped(windows, tolerance=tolerance, min_run=4, flips=flips, engine=eng)
        assert all({(g.a, g.b) for g in plain[f]} <= set(cand[f]) for f in flips)
        assert vdf.align_flipped(windows, tolerance=tolerance, min_run=4, flips=flips, engine=eng, pairs=cand) == plain
    g = [g for g in plain[Flip.X | Flip.T] if (g.a, g.b) == (0, 1)][0]
    assert g.first_frame_a + g.first_frame_b + g.n_frames == 10 + 3 + 40
    two = vdf.align_flipped([windows[0]], [windows[2], windows[1]], tolerance=0.0, min_run=4, flips=[Flip.X | Flip.T], engine=eng, seed=True)[Flip.X | Flip.T]
    assert [(t.a, t.b, t.first_frame_a, t.first_frame_b, t.n_frames) for t in two] == [(0, 1, 10, 3, 40)]


def test_argument_checks_in_their_order(eng):
    import torch

    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(3)
    h = _dev(hashgen.random_hashes(rng, 8), np.int64)
    z = _dev(np.zeros((8, 16), np.uint64), np.int64)
    first = lambda *v: _dev(np.array(v, np.uint32), np.int32)
    f = first(0, 3, 8)
    out = np.zeros(16, vdf.ALIGN_VARIANT_DTYPE)  # room for 16 records of either call
    n = C.c_size_t(99)
    torch.cuda.synchronize()
    lib = eng.lib
    p = lambda t: None if t is None else t.data_ptr()
    err = lambda c: lib.vdf_last_error(c).decode()

    def seed(ctx, ah, az, af, n_a, bh, bz, bf, n_b, min_run, mask, o=out.ctypes.data, cap=16, n_out=True):
        return lib.vdf_align_seed_pairs_variants_device(ctx, p(ah), p(az), p(af), n_a, None, p(bh), p(bz), p(bf), n_b, None, 350, min_run, mask, o, cap,
                                                        C.byref(n) if n_out else None, None)

    # the seed call: the checks of vdf_align_seed_pairs in their order, then the mask, the zero plane, the multi-GPU refusal
    assert seed(eng.ctx, None, None, f, 2, None, None, None, 0, 0, 1) == -5 and "null" in err(eng.ctx)
    assert seed(eng.ctx, h, None, f, 2, None, None, None, 0, 1, 1, n_out=False) == -5 and "null" in err(eng.ctx)
    assert seed(eng.ctx, h, None, f, 2, None, None, None, 0, 1, 1, o=None) == -5 and "null" in err(eng.ctx)
    big = first(0, 2**20 + 1, 2**20 - 5)
    assert seed(eng.ctx, h, None, big, 2, None, None, None, 0, 0, 1) == -5 and "min_run" in err(eng.ctx)
    assert seed(eng.ctx, h, None, big, 2, None, None, None, 0, 1, 1) == -5 and "2^20" in err(eng.ctx)
    assert seed(eng.ctx, h, None, first(0, 5, 3), 2, None, None, None, 0, 1, 1) == -5 and "decreases" in err(eng.ctx)
    zeros = _dev(np.zeros(4098, np.uint32), np.int32)
    assert seed(eng.ctx, h, None, zeros, 4097, h, None, zeros, 4097, 1, 1) == -5 and "2^24 pairs of videos" in err(eng.ctx)
    assert seed(eng.ctx, h, None, f, 2, None, None, None, 0, 1, 1) == -5 and "variant_mask" in err(eng.ctx)          # (and no zero plane)
    assert seed(eng.ctx, h, None, f, 2, None, None, None, 0, 1, 0x102) == -5 and "variant_mask" in err(eng.ctx)
    assert seed(eng.ctx, h, None, f, 2, None, None, None, 0, 1, 2) == -5 and "zero plane" in err(eng.ctx)
    assert seed(eng.ctx, h, z, f, 2, h, None, f, 2, 1, 2) == -5 and "zero plane" in err(eng.ctx)                     # two sets: B's plane is the one that counts
    assert seed(eng.ctx, h, None, f, 2, h, z, f, 2, 1, 0xFE) == 0
    assert seed(eng.ctx, h, z, f, 2, None, None, None, 0, 1, 0) == 0 and n.value == 0                               # no variant asked for
    assert seed(eng.ctx, h, z, zeros, 4096, h, z, zeros, 4096, 1, 0xFE) == 0 and n.value == 0                       # 2^24 pairs of empty videos: nothing to do
    for args in ((h, z, f, 0, None, None, None, 0), (h, z, f, 1, None, None, None, 0), (h, None, f, 2, h, z, f, 0)):
        n.value = 99
        assert seed(eng.ctx, *args, 1, 2) == 0 and n.value == 0

    # the list call: a null list first, the align checks, the list, the zero plane, the multi-GPU refusal last
    T = lambda *t: np.array([(a, b, v) for v, a, b in t], vdf.VIDEO_PAIR_VARIANT_DTYPE)
    good, unsorted, bad_variant, beyond, diag = T((1, 0, 1)), T((2, 0, 1), (1, 0, 1)), T((8, 0, 1)), T((1, 0, 2)), T((1, 1, 1))

    def pairs(ctx, af, n_a, az, bh, bz, lst, n_list, min_run):
        two = bh is not None
        return lib.vdf_align_windows_variants_pairs_device(ctx, p(h), p(az), p(af), n_a, None, p(bh), p(bz), p(af) if two else None, n_a if two else 0, None,
                                                           None if lst is None else lst.ctypes.data, n_list, 350, min_run, out.ctypes.data, 16, C.byref(n), None)

    assert pairs(eng.ctx, f, 2, z, None, None, None, 1, 0) == -5 and "null triple list" in err(eng.ctx)          # (and min_run == 0)
    assert pairs(eng.ctx, f, 2, z, None, None, unsorted, 2, 0) == -5 and "min_run" in err(eng.ctx)               # (and an unsorted list)
    assert pairs(eng.ctx, f, 2, z, None, None, unsorted, (1 << 24) + 1, 1) == -5 and "2^24 listed triples" in err(eng.ctx)
    assert pairs(eng.ctx, f, 2, None, None, None, unsorted, 2, 1) == -5 and "strictly increasing in (variant, a, b) at entry 1" in err(eng.ctx)   # (and no plane)
    assert pairs(eng.ctx, f, 2, z, None, None, bad_variant, 1, 1) == -5 and "variant outside 1 ... 7" in err(eng.ctx)
    assert pairs(eng.ctx, f, 2, z, None, None, beyond, 1, 1) == -5 and "does not exist" in err(eng.ctx)
    assert pairs(eng.ctx, f, 2, z, None, None, diag, 1, 1) == -5 and "a >= b in self mode" in err(eng.ctx)
    assert pairs(eng.ctx, f, 2, None, None, None, good, 1, 1) == -5 and "zero plane" in err(eng.ctx)
    assert pairs(eng.ctx, f, 2, None, h, z, diag, 1, 1) == 0                                                      # fine between two sets
    assert pairs(eng.ctx, first(0, 5, 3), 2, z, None, None, good, 1, 1) == -5 and "decreases" in err(eng.ctx)    # the first arrays, once they are down
    n.value = 99
    assert pairs(eng.ctx, f, 2, z, None, None, None, 0, 1) == 0 and n.value == 0
    multi = vdf.Engine(devices=[0, 0])
    try:
        assert seed(multi.ctx, h, None, f, 2, None, None, None, 0, 0, 1) == -5 and "min_run" in err(multi.ctx)
        assert seed(multi.ctx, h, None, f, 2, None, None, None, 0, 1, 1) == -5 and "variant_mask" in err(multi.ctx)
        assert seed(multi.ctx, h, None, f, 2, None, None, None, 0, 1, 2) == -5 and "zero plane" in err(multi.ctx)
        assert seed(multi.ctx, h, z, f, 2, None, None, None, 0, 1, 2) == -5 and "single-device" in err(multi.ctx)
        assert pairs(multi.ctx, f, 2, z, None, None, unsorted, 2, 1) == -5 and "strictly increasing" in err(multi.ctx)
        assert pairs(multi.ctx, f, 2, None, None, None, good, 1, 1) == -5 and "zero plane" in err(multi.ctx)
        assert pairs(multi.ctx, f, 2, z, None, None, good, 1, 1) == -5 and "single-device" in err(multi.ctx)
        words, planes = hashgen.random_hashes(rng, 8), np.zeros((8, 16), np.uint64)
        for call in (lambda: multi.align_seed_pairs_variants(words, [0, 3, 8], a_zero=planes),
                     lambda: multi.align_windows_variants_pairs(words, [0, 3, 8], [(1, 0, 1)], a_zero=planes)):
            with pytest.raises(vdf.VdfError) as ei:
                call()
            assert ei.value.code == -5 and "single-device" in str(ei.value)
    finally:
        multi.close()


CHILD = """
import sys
sys.path.insert(0, {tests!r})
import seedvariantgen as svg
import vid_dup_finder_lib_amd as vdf
from test_gpu_align_seed_variants import pairs_host_arrays, seed_device, seed_host_arrays

lib = vdf._capi.load()
assert lib.vdf_live_device_bytes() == 0      # a fresh process: no other engine is alive
e = vdf.Engine(0)
vp = svg.case("tile_edges_self")
cand, _ = seed_host_arrays(e, vp)
assert cand == list(svg.expected("tile_edges_self"))
assert pairs_host_arrays(e, vp, cand)[0] == list(svg.expected_records("tile_edges_self"))
assert seed_device(e, svg.case("tile_edges"))[0] == list(svg.expected("tile_edges"))
held = lib.vdf_live_device_bytes()
e.close()
print("LIVE", held, lib.vdf_live_device_bytes())
"""


def test_no_device_memory_is_left_behind():
    """in a fresh child process: the library's count of live device bytes is 0 before the engine, above 0 after the seed call, the list call and
    their buffers (class-major rows, bitmap, plan, dense triples), and 0 again after close"""
    import os
    import subprocess
    import sys

    tests = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, "-c", CHILD.format(tests=tests)], cwd=os.path.dirname(tests), capture_output=True, text=True, timeout=300)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("LIVE ")]
    assert out.returncode == 0 and line, out.stdout[-2000:] + out.stderr[-3000:]
    held, after = (int(x) for x in line[-1].split()[1:])
    assert held > 0 and after == 0
