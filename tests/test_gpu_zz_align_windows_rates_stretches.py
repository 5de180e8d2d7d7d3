"""vdf_align_windows_rates_stretches[_device] (csrc/align.hip: align_bands_kernel<AlignTripleUnits, true> behind the rates kernel's round 0, on the rounds of
csrc/align_rates_stretch_plan.h) against the plain C++ definition (vdf_align_windows_rates_stretches_host) and the numpy twin of
tests/ratestretchgen.py, records equal: the device form on device arrays and the host-array form.  Four rates whose units share one workgroup,
each wave with its own rectangles; a triple at 3/2 with 200 x 134 windows and tolerance 500 - three bands per phase, a rectangle across the band
boundaries; rectangles clamped at row 0 and at Na / Nb; seven rectangles on one triple under max_stretches = 8; one surviving triple in a chunk of
many; skip arrays 1 and 3 bytes off a dword with first arrays 5 and 3 rows in; a dense case that runs every round; the capacity protocol; lists
that name empty videos and an empty list; seed = 1 equal to seed = 0; the device call behind copies pending on its stream; seeded random problems;
the refusals through a context; and hash_frame_windows(one_call=True) -> align_rates_all(seed=True) -> best_rates_all end to end on a 6/5 copy
with a cut.

The file's name sorts it behind test_gpu_zz_align_windows_rates.py, so every test before it sees the process it saw without this file."""
import os

import numpy as np
import pytest

import hashgen
import ratealigngen as gen
import ratestretchgen as sg

pytestmark = pytest.mark.gpu
SEEDS = max(20, int(os.environ.get("VDF_FUZZ_SEEDS", "0")))


@pytest.fixture(scope="module")
def eng():
    import vid_dup_finder_lib_amd as vdf

    e = vdf.Engine(0)
    yield e
    e.close()


class OnDevice:
    """a problem's arrays as device arrays; the skip arrays begin 1 (A) and 3 (B) bytes off a 4-byte boundary, inside buffers padded to whole dwords"""

    def __init__(self, p):
        import torch

        dev = lambda x, dtype: torch.from_numpy(np.ascontiguousarray(x).view(dtype).copy()).cuda()

        def skip(x, off):
            if x is None:
                return None, 0
            host = np.zeros((off + len(x) + 7) & ~3, np.uint8)
            host[:off] = 1          # the bytes beside the array are read with its first word and must be ignored
            host[off + len(x):] = 1
            host[off:off + len(x)] = x
            t = torch.from_numpy(host).cuda()
            return t, t.data_ptr() + off
        self.ah, self.af = dev(p.a_hashes, np.int64), dev(np.ascontiguousarray(p.a_first, dtype=np.uint32), np.int32)
        self.bh, self.bf = dev(p.b_hashes, np.int64), dev(np.ascontiguousarray(p.b_first, dtype=np.uint32), np.int32)
        self.ak, ak_ptr = skip(p.a_skip, 1)
        self.bk, bk_ptr = skip(p.b_skip, 3)
        torch.cuda.synchronize()
        assert ak_ptr % 4 in (0, 1) and bk_ptr % 4 in (0, 3)
        self.args = (self.ah.data_ptr(), self.af.data_ptr(), p.a_first.shape[1] - 1, self.bh.data_ptr(), self.bf.data_ptr(), len(p.b_first) - 1, p.rates)
        self.kw = dict(tol_int=p.tol, min_run=p.min_run, a_rate_first=p.a_rate_first, d_a_skip=ak_ptr, d_b_skip=bk_ptr, exclude_same=p.exclude_same)


def device(eng, p, most, guard, capacity=4096, **over):
    d = OnDevice(p)
    got, found = eng.align_windows_rates_stretches_device(*d.args, max_stretches=most, guard=guard, capacity=capacity, **dict(d.kw, **over))
    return sg.records(got), found


def host_arrays(eng, p, most, guard, capacity=4096, **over):
    kw = dict(tol_int=p.tol, min_run=p.min_run, max_stretches=most, guard=guard, a_rate_first=p.a_rate_first, a_skip=p.a_skip, b_skip=p.b_skip,
              exclude_same=p.exclude_same, capacity=capacity)
    got, found = eng.align_windows_rates_stretches(p.a_hashes, p.a_first, p.b_hashes, p.b_first, p.rates, **dict(kw, **over))
    return sg.records(got), found


def host(p, most, guard, capacity=4096, **over):
    """the plain C++ definition: what the kernel is held against"""
    import vid_dup_finder_lib_amd as vdf

    kw = dict(tol_int=p.tol, min_run=p.min_run, max_stretches=most, guard=guard, a_rate_first=p.a_rate_first, a_skip=p.a_skip, b_skip=p.b_skip,
              exclude_same=p.exclude_same, capacity=capacity)
    got, found = vdf.align_windows_rates_stretches_host(p.a_hashes, p.a_first, p.b_hashes, p.b_first, p.rates, **dict(kw, **over))
    return sg.records(got), found


@pytest.mark.parametrize("name", list(sg.CASES))
def test_masked_rates_kernel_matches_the_host_form(eng, name):
    sg.check_non_vacuous(name)   # on the twin's own output, before anything runs
    p, most, guard = sg.case(name)
    want = host(p, most, guard)
    assert want == (list(sg.expected(name)), len(sg.expected(name)))
    got = device(eng, p, most, guard)
    print(f"{name}: {len(want[0])} records of {gen.n_triples(p)} triples, ranks up to {max([0] + [w[8] for w in want[0]])}, device form found {got[1]}")
    assert got == want
    assert host_arrays(eng, p, most, guard) == want


def test_four_rates_in_one_workgroup_each_with_its_own_rectangles(eng):
    """the list form: units 0 .. 3 of every round are four triples at four rates - four waves of one workgroup - and each has other rectangles"""
    for name in ("four_rates", "four_rates_offsets"):
        p, most, guard = sg.case(name)
        want = sg.twin(p, most, guard, sg.FOUR_LIST)
        first = [w for w in want if w[:2] == (0, 0)]
        assert [(w[2], w[8]) for w in first] == [(r, k) for r in range(4) for k in range(3)]
        assert any(w[8] == 1 and w[:3] == (2, 1, 3) for w in want)
        for r in range(4):   # one unit each: one window of a
            assert int(p.a_first[r, 1] - p.a_first[r, 0]) == 1
        triples = gen.triple_array(sg.FOUR_LIST)
        assert device(eng, p, most, guard, triples=triples) == (want, len(want))
        assert host_arrays(eng, p, most, guard, triples=triples) == (want, len(want))
    q = sg.case("four_rates_offsets")[0]   # first arrays 5 and 3 rows in, skip arrays 1 and 3 bytes off a dword
    assert all(int(f[0]) == 5 for f in q.a_first) and int(q.b_first[0]) == 3 and q.a_skip.any() and q.b_skip.any()


def test_the_layout_the_cases_promise():
    """what the cases are there for, asserted on their arrays and on the twin's output"""
    bands = lambda na, nb: 0 if not na or not nb else (na + nb - 1 + 63) // 64
    p, most, guard = sg.case("bands3")
    assert bands(67, 67) == 3 and int(p.a_first[1, 1] - p.a_first[1, 0]) == 200 and int(p.b_first[1] - p.b_first[0]) == 134 and p.tol == 500
    r0 = [w for w in sg.expected("bands3") if (w[2], w[0], w[1], w[8]) == (1, 0, 0, 0)][0]
    a_lo, a_hi, b_lo, b_hi = sg.rect_of(r0[3], r0[4], r0[5], (3, 2), guard, 200, 134)
    offsets = {rb // 2 - (ra - ph) // 3 for ph in range(3) for ra in range(a_lo + (ph - a_lo) % 3, a_hi, 3) for rb in range(b_lo + b_lo % 2, b_hi, 2)}
    assert min(offsets) < -3 and max(offsets) > -2, "the rectangle has cells in bands 0 and 1 of a phase: band 1 of 67 x 67 cells begins at diagonal -2"
    assert max(w[8] for w in sg.expected("bands3") if (w[2], w[0], w[1]) == (1, 0, 0)) == most - 1
    # one surviving triple in a chunk of many
    want = sg.expected("cut_6_5")
    assert {(w[2], w[0], w[1]) for w in want} == {(1, 2, 1)} and gen.n_triples(sg.case("cut_6_5")[0]) == 36


def test_capacity_protocol(eng):
    p, most, guard = sg.case("dense")
    want = list(sg.expected("dense"))
    for call in (device, host_arrays):
        for kw in (dict(), dict(seed=True)):
            for m in (most, 1):
                w = [x for x in want if x[8] < m]
                assert call(eng, p, m, guard, capacity=0, **kw) == ([], len(w))
                assert call(eng, p, m, guard, capacity=5, **kw) == (w[:5], len(w)) and len(w) > 5
                assert call(eng, p, m, guard, capacity=len(w), **kw) == (w, len(w))


def test_lists_that_name_empty_videos_and_an_empty_list(eng):
    p, most, guard = sg.case("bands3")    # video 1 of B has no windows
    listed = [(0, 0, 1), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 1)]
    want = sg.twin(p, most, guard, listed)
    assert want and all(w[1] != 1 for w in want)
    for call in (device, host_arrays):
        assert call(eng, p, most, guard, triples=gen.triple_array(listed)) == (want, len(want))
        assert call(eng, p, most, guard, triples=gen.triple_array([(0, 0, 1), (1, 1, 1)])) == ([], 0)     # nothing but empty videos: no unit, no launch
        assert call(eng, p, most, guard, triples=gen.triple_array([])) == ([], 0)
    q, most, guard = sg.case("unrelated")   # no record in round 0: no later round
    assert device(eng, q, most, guard) == ([], 0) and host_arrays(eng, q, most, guard, seed=True) == ([], 0)


@pytest.mark.parametrize("name", sg.SEEDED)
def test_seed_one_equals_seed_zero(eng, name):
    p, most, guard = sg.case(name)
    want = list(sg.expected(name))
    assert device(eng, p, most, guard, seed=True) == (want, len(want))
    assert host_arrays(eng, p, most, guard, seed=True) == (want, len(want))


def test_max_stretches_one_is_the_rates_call(eng):
    for name in ("cut_6_5_offsets", "dense"):
        p, _, guard = sg.case(name)
        d = OnDevice(p)
        plain, n = eng.align_windows_rates_device(*d.args, capacity=4096, **d.kw)
        assert n == len(plain) >= 1 and device(eng, p, 1, guard) == ([r + (0,) for r in gen.records(plain)], n)


def test_guard_zero_and_a_guard_larger_than_the_videos(eng):
    for name in ("cut_6_5", "seven_rects", "dense"):
        p, most, _ = sg.case(name)
        for guard in (0, 1 << 20):
            assert device(eng, p, most, guard) == host(p, most, guard) == (sg.twin(p, most, guard), len(sg.twin(p, most, guard)))


def test_refusals_through_a_context(eng):
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd import _capi

    p = sg.case("square")[0]
    d = OnDevice(p)

    def refused(what, **over):
        with pytest.raises(vdf.VdfError) as ei:
            eng.align_windows_rates_stretches_device(*d.args, **dict(d.kw, **over))
        assert ei.value.code == _capi.VDF_E_INVAL and what in str(ei.value), (what, str(ei.value))

    one = gen.triple_array([(0, 0, 1)])
    refused("min_run", min_run=0, max_stretches=0)
    refused("together with seed or exclude_same", triples=one, max_stretches=0)                    # the case's exclude_same; the list comes before max_stretches
    refused("rate that is not in the rate list", triples=gen.triple_array([(2, 0, 0)]), exclude_same=False, max_stretches=9)
    refused("max_stretches", max_stretches=0, guard=1 << 21)
    refused("max_stretches", max_stretches=9)
    refused("guard", guard=(1 << 20) + 1)
    multi = vdf.Engine(devices=[0, 0])
    try:
        with pytest.raises(vdf.VdfError) as ei:
            multi.align_windows_rates_stretches_device(*d.args, **d.kw)
        assert ei.value.code == _capi.VDF_E_INVAL and "single-device" in str(ei.value)
        with pytest.raises(vdf.VdfError) as ei:   # max_stretches and guard are checked before the context
            multi.align_windows_rates_stretches_device(*d.args, **dict(d.kw, guard=1 << 21))
        assert "guard" in str(ei.value)
    finally:
        multi.close()


def test_the_device_call_waits_for_copies_pending_on_its_stream(eng):
    """decoy contents first, a stretch of work, the real contents queued just before the call - all on the job's stream: the records are the real one's"""
    import torch

    real, most, guard = sg.case("cut_6_5_offsets")
    want = list(sg.expected("cut_6_5_offsets"))
    rng = np.random.default_rng([92, 13])   # the decoy: the same layout without the planted cells, every skip byte of B set - nothing has a record
    decoy = real._replace(a_hashes=hashgen.random_hashes(rng, len(real.a_hashes)), b_hashes=hashgen.random_hashes(rng, len(real.b_hashes)),
                          a_skip=np.zeros_like(real.a_skip), b_skip=np.ones_like(real.b_skip))
    assert sg.twin(decoy, most, guard) == [] and any(w[8] == 1 for w in want)
    for seed in (False, True):
        d = OnDevice(decoy)
        pin = lambda x, dtype: torch.from_numpy(np.ascontiguousarray(x).view(dtype).copy()).pin_memory()
        src = [(d.ah, pin(real.a_hashes, np.int64)), (d.bh, pin(real.b_hashes, np.int64))]
        for t, off, x in ((d.ak, 1, real.a_skip), (d.bk, 3, real.b_skip)):
            h = t.cpu().numpy().copy()
            h[off:off + len(x)] = x
            src.append((t, torch.from_numpy(h).pin_memory()))
        st = torch.cuda.Stream(device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            busy = torch.ones((2048, 2048), device="cuda")
            for _ in range(20):
                busy = busy @ busy * 1e-4
            for dst, h in src:
                dst.copy_(h, non_blocking=True)
            got, found = eng.align_windows_rates_stretches_device(*d.args, max_stretches=most, guard=guard, capacity=4096, stream=st.cuda_stream, seed=seed, **d.kw)
        st.synchronize()
        assert (sg.records(got), found) == (want, len(want)), "the call ran ahead of the copies queued on its stream"


@pytest.mark.parametrize("seed", range(SEEDS))
def test_seeded_random_problems(eng, seed):
    p, most, guard = sg.random_problem(np.random.default_rng([92, 11, seed]))
    want = host(p, most, guard)
    assert want[0] == sg.twin(p, most, guard)
    assert device(eng, p, most, guard) == want, (seed, p.rates, p.tol, p.min_run, most, guard)
    assert device(eng, p, most, guard, seed=True) == want, (seed, p.rates, p.tol, p.min_run, most, guard)
    if seed % 4 == 0:
        assert host_arrays(eng, p, most, guard) == want, (seed, p.rates, p.tol, p.min_run, most, guard)
        assert host_arrays(eng, p, most, guard, seed=True) == want, (seed, p.rates, p.tol, p.min_run, most, guard)


def test_end_to_end_a_6_5_copy_with_a_cut(eng):
    """hash_frame_windows(one_call=True), then align_rates_all(seed=True), then best_rates_all: three calls; the records are the host route's"""
    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(29)
    a = [rng.integers(0, 256, size=(f, 24, 32), dtype=np.uint8) for f in (120, 60, 70)]
    take = lambda v, c, n: v[c + (np.arange(n) * 6) // 5]
    b = [np.ascontiguousarray(np.concatenate([take(a[0], 0, 32), take(a[0], 70, 34)])), rng.integers(0, 256, size=(40, 24, 32), dtype=np.uint8)]   # frames 39 .. 69 cut out
    rates = [(1, 1), (6, 5), (3, 2)]
    pa, pb = [f"/a/{i}.mp4" for i in range(len(a))], [f"/b/{i}.mp4" for i in range(len(b))]
    wa = vdf.hash_frame_windows(a, pa, [len(v) for v in a], engine=eng, rates=rates, one_call=True)
    wb = vdf.hash_frame_windows(b, pb, [len(v) for v in b], engine=eng, rates=[(1, 1)], one_call=True)[(1, 1)]
    assert max(sum(len(w) for w in wa[r]) for r in rates) * sum(len(w) for w in wb) <= 1 << 16, "small enough for the host route"
    for tolerance in (0.0, 0.35):
        for kw in (dict(), dict(max_stretches=8, guard=0), dict(pairs=[(0, 0), (1, 1)])):
            want = vdf.align_rates_all(wa, wb, tolerance, 2, **kw)                 # no engine, tiny input: vdf_align_windows_rates_stretches_host
            assert vdf.align_rates_all(wa, wb, tolerance, 2, engine=eng, seed=True, **kw) == want
            assert vdf.align_rates_all(wa, wb, tolerance, 2, engine=eng, **kw) == want
    got = vdf.align_rates_all(wa, wb, 0.35, 2, engine=eng, seed=True)
    copy = [r for r in got[(6, 5)] if (r.a, r.b) == (0, 0)]
    # two stretches on two lines first_frame_a - first_frame_b * 6 / 5: 0 in front of the cut, 70 - 32 * 6 / 5 = 31.6 behind it (a window that holds a
    # frame or two from the other side of the cut still matches, so the second stretch may begin a window early: the line is what is planted)
    lines = sorted(r.first_frame_a - r.first_frame_b * 6 / 5 for r in copy[:2])
    assert [r.rank for r in copy[:2]] == [0, 1] and abs(lines[0]) <= 1 and abs(lines[1] - 31.6) <= 1, copy[:2]
    assert sum(r.n_frames_b for r in copy[:2]) >= 40 and all(r.first_frame_b % 5 == 0 for r in copy)
    best = vdf.best_rates_all(got, 0.35)
    assert (0, 0) in best and {(r.num, r.den) for r in best[(0, 0)]} == {(6, 5)} and len(best[(0, 0)]) >= 2
    assert best == vdf.best_rates_all(vdf.align_rates_all(wa, wb, 0.35, 2), 0.35)
