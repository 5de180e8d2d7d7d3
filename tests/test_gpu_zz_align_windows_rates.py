"""vdf_align_windows_rates[_device] (csrc/align.hip: align_bands_kernel<AlignTripleUnits, false>, align_reduce_rates_kernel and the 32-byte scatter on the plan of
csrc/align_rates_plan.h) against the twin of tests/ratealigngen.py, records equal: the device form on device arrays and the
host-array form, on the problems tests/test_align_windows_rates_host.py gives the plain C++ definition.  Four rates in one workgroup (a list whose
first four triples are one unit each, at 1/1, 3/2, 6/5 and 32/17; videos of 1, 2, 3 and 130 windows against 1, 2 and 129, other counts per rate,
empty phases); three bands at 3/2 and tolerance 500; the planted lines of 4.17, each in another rate slot; first arrays that begin 5 and 3 rows
in with skip arrays 1 and 3 bytes off a dword; a dense case; the capacity protocol; lists that name empty videos and an empty list; seed = 1
equal to seed = 0; the device call behind copies pending on its stream; seeded random problems; and hash_frame_windows(one_call=True) ->
align_rates(one_call=True, seed=True) end to end.

The file's name sorts it behind test_gpu_zz_align_seed_rates.py, so every test before it sees the process it saw without this file (DESIGN.md
4.22, "Found on the way")."""
import os

import numpy as np
import pytest

import hashgen
import ratealigngen as gen

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


def device(eng, p, capacity=4096, **over):
    d = OnDevice(p)
    got, found = eng.align_windows_rates_device(*d.args, capacity=capacity, **dict(d.kw, **over))
    return gen.records(got), found


def host_arrays(eng, p, capacity=4096, **over):
    kw = dict(tol_int=p.tol, min_run=p.min_run, a_rate_first=p.a_rate_first, a_skip=p.a_skip, b_skip=p.b_skip, exclude_same=p.exclude_same, capacity=capacity)
    got, found = eng.align_windows_rates(p.a_hashes, p.a_first, p.b_hashes, p.b_first, p.rates, **dict(kw, **over))
    return gen.records(got), found


@pytest.mark.parametrize("name", list(gen.CASES))
def test_rates_kernel_matches_the_twin(eng, name):
    gen.check_non_vacuous(name)   # on the twin's own output, before anything runs
    p, want = gen.case(name), list(gen.expected(name))
    got, found = device(eng, p)
    print(f"{name}: {len(want)} records of {gen.n_triples(p)} triples, device form found {found}")
    assert found == len(want)
    assert got == want
    got, found = host_arrays(eng, p)
    assert found == len(want) and got == want


def test_four_rates_in_one_workgroup(eng):
    """the list form: units 0 .. 3 of the launch are four triples at four rates - four waves of one workgroup, each with its own slot"""
    p = gen.case("mixed")
    want = gen.twin(p, gen.MIXED_LIST)
    assert [w[2] for w in want[:4]] == [0, 1, 2, 3] and len({w[2] for w in want}) == 4 and len(want) < len(gen.MIXED_LIST)
    triples = gen.triple_array(gen.MIXED_LIST)
    assert device(eng, p, triples=triples) == (want, len(want))
    assert host_arrays(eng, p, triples=triples) == (want, len(want))
    q = gen.case("mixed_offsets")   # first arrays 5 and 3 rows in, skip arrays 1 and 3 bytes off a dword
    assert int(q.a_first[0, 0]) == 5 and all(int(f[0]) == 5 for f in q.a_first) and int(q.b_first[0]) == 3 and q.a_skip.any() and q.b_skip.any()
    want = gen.twin(q, gen.MIXED_LIST)
    assert want and device(eng, q, triples=triples) == (want, len(want)) and host_arrays(eng, q, triples=triples) == (want, len(want))


def test_the_layout_the_cases_promise():
    """what the cases are there for, asserted on their arrays: the units per triple, the three bands, the counts that differ per rate"""
    from math import ceil

    bands = lambda na, nb: 0 if not na or not nb else (na + nb - 1 + 63) // 64
    p = gen.case("mixed")
    units = []
    for r, a, b in gen.all_triples(p):
        num, den = gen.reduced(p.rates[r])
        na, nb = int(p.a_first[r, a + 1] - p.a_first[r, a]), int(p.b_first[b + 1] - p.b_first[b])
        units.append(sum(bands(len(range(ph, na, num)), ceil(nb / den)) for ph in range(num)))
    assert min(units) == 1 and 5 in units and 6 in units and max(units) >= 32     # 1 x 1; 1/1: 258 diagonals; 3/2: 3 x 2; 32/17: a band per phase
    assert len({tuple(np.diff(f.astype(np.int64))) for f in p.a_first}) == len(p.rates)
    q = gen.case("bands3")
    assert bands(67, 65) == 3 and int(q.a_first[1, 1] - q.a_first[1, 0]) == 200 and int(q.b_first[1] - q.b_first[0]) == 130 and q.tol == 500
    assert len({gen.reduced(r) for r in gen.PLANTED_RATES}) == 1 and len(gen.PLANTED_RATES) == 8


def test_capacity_protocol(eng):
    p, want = gen.case("planted_min_run_1"), list(gen.expected("planted_min_run_1"))
    for call in (device, host_arrays):
        for kw in (dict(), dict(seed=True)):
            assert call(eng, p, capacity=0, **kw) == ([], len(want))
            assert call(eng, p, capacity=5, **kw) == (want[:5], len(want)) and len(want) > 5
            assert call(eng, p, capacity=len(want), **kw) == (want, len(want))


def test_lists_that_name_empty_videos_and_an_empty_list(eng):
    p = gen.case("bands3")    # video 1 of B has no windows; video 1 of A has 3 and 2
    listed = [(0, 0, 1), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 1)]
    want = gen.twin(p, listed)
    assert want and all(w[1] != 1 for w in want)
    for call in (device, host_arrays):
        assert call(eng, p, triples=gen.triple_array(listed)) == (want, len(want))
        assert call(eng, p, triples=gen.triple_array([(0, 0, 1), (1, 1, 1)])) == ([], 0)     # nothing but empty videos: no unit, no launch
        assert call(eng, p, triples=gen.triple_array([])) == ([], 0)


@pytest.mark.parametrize("name", gen.SEEDED)
def test_seed_one_equals_seed_zero(eng, name):
    gen.check_non_vacuous(name)
    p, want = gen.case(name), list(gen.expected(name))
    assert device(eng, p, seed=True) == (want, len(want))
    assert host_arrays(eng, p, seed=True) == (want, len(want))


def test_refusals_through_a_context(eng):
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd import _capi

    p = gen.case("square")
    d = OnDevice(p)

    def refused(what, **over):
        with pytest.raises(vdf.VdfError) as ei:
            eng.align_windows_rates_device(*d.args, **dict(d.kw, **over))
        assert ei.value.code == _capi.VDF_E_INVAL and what in str(ei.value), (what, str(ei.value))

    one = gen.triple_array([(0, 0, 1)])
    refused("min_run", min_run=0, triples=one)
    refused("together with seed or exclude_same", triples=one)                    # the case's exclude_same
    refused("together with seed or exclude_same", triples=one, exclude_same=False, seed=True)
    refused("not strictly increasing", triples=gen.triple_array([(1, 0, 0), (0, 0, 0)]), exclude_same=False)
    refused("rate that is not in the rate list", triples=gen.triple_array([(2, 0, 0)]), exclude_same=False)
    refused("video that does not exist", triples=gen.triple_array([(0, 0, 7)]), exclude_same=False)
    multi = vdf.Engine(devices=[0, 0])
    try:
        with pytest.raises(vdf.VdfError) as ei:
            multi.align_windows_rates_device(*d.args, **d.kw)
        assert ei.value.code == _capi.VDF_E_INVAL and "single-device" in str(ei.value)
        with pytest.raises(vdf.VdfError) as ei:   # the list is checked before the context
            multi.align_windows_rates_device(*d.args, **dict(d.kw, exclude_same=False, triples=gen.triple_array([(2, 0, 0)])))
        assert "rate that is not in the rate list" in str(ei.value)
    finally:
        multi.close()


def test_the_device_call_waits_for_copies_pending_on_its_stream(eng):
    """decoy contents first, a stretch of work, the real contents queued just before the call - all on the job's stream: the records are the real one's"""
    import torch

    real = gen.case("mixed_offsets")
    want = list(gen.expected("mixed_offsets"))
    rng = np.random.default_rng([91, 13])   # the decoy: the same layout without the planted cells, every skip byte of B set - nothing has a record
    decoy = real._replace(a_hashes=hashgen.random_hashes(rng, len(real.a_hashes)), b_hashes=hashgen.random_hashes(rng, len(real.b_hashes)),
                          a_skip=np.zeros_like(real.a_skip), b_skip=np.ones_like(real.b_skip))
    assert gen.twin(decoy) == [] and want
    for seed in (False, True):
        d = OnDevice(decoy)
        pin = lambda x, dtype: torch.from_numpy(np.ascontiguousarray(x).view(dtype).copy()).pin_memory()
        src = [(d.ah, pin(real.a_hashes, np.int64)), (d.bh, pin(real.b_hashes, np.int64))]
        for t, off, x in ((d.ak, 1, real.a_skip), (d.bk, 3, real.b_skip)):
            host = t.cpu().numpy().copy()
            host[off:off + len(x)] = x
            src.append((t, torch.from_numpy(host).pin_memory()))
        st = torch.cuda.Stream(device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            busy = torch.ones((2048, 2048), device="cuda")
            for _ in range(20):
                busy = busy @ busy * 1e-4
            for dst, host in src:
                dst.copy_(host, non_blocking=True)
            got, found = eng.align_windows_rates_device(*d.args, capacity=4096, stream=st.cuda_stream, seed=seed, **d.kw)
        st.synchronize()
        assert (gen.records(got), found) == (want, len(want)), "the call ran ahead of the copies queued on its stream"


@pytest.mark.parametrize("seed", range(SEEDS))
def test_seeded_random_problems(eng, seed):
    p = gen.random_problem(np.random.default_rng([91, 11, seed]))
    want = gen.twin(p)
    assert device(eng, p) == (want, len(want)), (seed, p.rates, p.tol, p.min_run)
    assert device(eng, p, seed=True) == (want, len(want)), (seed, p.rates, p.tol, p.min_run)
    if seed % 4 == 0:
        assert host_arrays(eng, p) == (want, len(want)), (seed, p.rates, p.tol, p.min_run)
        assert host_arrays(eng, p, seed=True) == (want, len(want)), (seed, p.rates, p.tol, p.min_run)


def test_end_to_end_one_call_equals_one_call_per_rate(eng):
    """hash_windows_clips_rates, then align_windows_rates(seed = 1), then best_rates: three calls, the answer of the default route"""
    import vid_dup_finder_lib_amd as vdf
    from test_gpu_zz_align_seed_rates import _excerpts

    five = [(1, 1), (6, 5), (5, 4), (3, 2), (2, 1)]
    a, b, planted = _excerpts(23)
    pa, pb = [f"/a/{i}.mp4" for i in range(len(a))], [f"/b/{i}.mp4" for i in range(len(b))]
    wa = vdf.hash_frame_windows(a, pa, [len(v) for v in a], engine=eng, rates=five, one_call=True)
    wb = vdf.hash_frame_windows(b, pb, [len(v) for v in b], engine=eng, rates=[(1, 1)], one_call=True)[(1, 1)]
    for tolerance in (0.0, 0.35):
        today = vdf.align_rates(wa, wb, tolerance, 2, engine=eng, native=True, seed=True)
        assert vdf.align_rates(wa, wb, tolerance, 2, engine=eng, seed=True, one_call=True) == today
        assert vdf.align_rates(wa, wb, tolerance, 2, engine=eng, one_call=True) == today
    best = {(r.a, r.b): r for r in vdf.best_rates(vdf.align_rates(wa, wb, 0.35, 2, engine=eng, seed=True, one_call=True), 0.35)}
    assert set(planted) <= set(best)
    for pair, (c, n, rate) in planted.items():
        assert (best[pair].num, best[pair].den) == rate, (pair, best[pair])
    listed = [(0, 0), (1, 1), (4, 2)]
    want = vdf.align_rates(wa, wb, 0.35, 2, engine=eng, native=True, seed=True, pairs=listed)
    assert vdf.align_rates(wa, wb, 0.35, 2, engine=eng, seed=True, pairs=listed, one_call=True) == want
    assert vdf.align_rates(wa, wb, 0.35, 2, engine=eng, pairs=listed, one_call=True) == want
