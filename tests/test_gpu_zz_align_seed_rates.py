"""vdf_align_seed_pairs_rates[_device] (csrc/align.hip: align_seed_rates_kernel on the plan of csrc/align_seed_rates_plan.h) against
the numpy twin of tests/seedrategen.py, triples equal: the device form on device arrays and the host-array form, on the problems
tests/test_align_seed_rates_host.py gives the plain C++ definition.  B: videos of 0, 1, 4, 700, 5 and 1900 windows - six tiles in the class of den 1,
a second tile of 11 rows in the class of den 5 whose waves 1 - 3 are padding; A: 0, 1, 2, 3, 31, 33 and 600 windows per rate block - empty phases,
more than one chunk of 256 seeds per class; single cells planted at distance tol and tol + 1, off the row grid, off the seed grid and under either
skip byte, at the edges of tiles and waves; tolerances 150, 250, 350 and 400 - the four early-exit instantiations - and one dense problem at 500;
five rates in one call, 31/16 with 32/17, one rate, duplicates; skip arrays 1 and 3 bytes off a 4-byte boundary, first arrays that begin at 5 and 3;
7 x 6 videos, so slot boundaries fall inside bitmap words.  Then the capacity protocol, exclude_same, the refusals in their order, the device call
behind copies still pending on its stream, seeded random problems, and hash_frame_windows(one_call=True) -> align_rates(one_pass=True) end to end.

The file's name sorts it behind every other GPU test on purpose.  In alphabetical place (as test_gpu_align_seed_rates.py) the whole suite failed two
tests that run none of this code and pass without this file in front of them: the suspect-queue overflow test of test_gpu_search_structured.py (a
queue that grew read stale bytes where the allocator had handed the old address back: fixed in api.cpp) and
test_gpu_stream_order.py::test_control_a_call_on_another_stream_runs_ahead, a control that EXPECTS a call on another stream to overtake a delay, which
depends on which hardware queues the process's streams share - on every stream made before it.  Behind them this file changes nothing they see."""
import ctypes as C
import os

import numpy as np
import pytest

import hashgen
import seedrategen as gen

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
    got, found = eng.align_seed_pairs_rates_device(*d.args, capacity=capacity, **dict(d.kw, **over))
    return gen.triples_of(got), found


def host_arrays(eng, p, capacity=4096):
    got, found = eng.align_seed_pairs_rates(p.a_hashes, p.a_first, p.b_hashes, p.b_first, p.rates, tol_int=p.tol, min_run=p.min_run, a_rate_first=p.a_rate_first,
                                            a_skip=p.a_skip, b_skip=p.b_skip, exclude_same=p.exclude_same, capacity=capacity)
    return gen.triples_of(got), found


@pytest.mark.parametrize("name", list(gen.CASES) + ["dense"])
def test_seed_rates_kernel_matches_the_twin(eng, name):
    p, want = gen.case(name), list(gen.expected(name))
    got, found = device(eng, p)
    print(f"{name}: {len(want)} candidate triples, device form found {found}")
    assert found == len(want)
    assert got == want
    got, found = host_arrays(eng, p)
    assert found == len(want) and got == want


def test_the_layout_the_cases_promise():
    """what the cases are there for, asserted on their arrays: the tiles, the ragged class, the chunks, the word boundaries, the off-grid starts"""
    p = gen.case("tol350_run3")
    counts_b = np.diff(p.b_first.astype(np.int64))
    rows = {den: int(sum(-(-n // den) for n in counts_b)) for den in (1, 2, 4, 5)}
    assert rows == {1: 2610, 2: 1306, 4: 654, 5: 523} and -(-rows[1] // 512) == 6 and rows[5] - 512 == 11
    assert int(p.a_first[0, 0]) == 5 and int(p.b_first[0]) == 3
    assert ((p.a_first.shape[1] - 1) * (len(p.b_first) - 1)) % 32
    for min_run in (1, 2, 3):
        assert sum(int(np.count_nonzero((np.arange(n) // num) % min_run == 0)) for num in (1, 2) for n in gen.A_COUNTS) > 256   # the class of den 1
    assert {gen.case(n).tol for n in gen.CASES} >= {150, 250, 350, 400}


def test_capacity_protocol(eng):
    p, want = gen.case("tol250_run2"), list(gen.expected("tol250_run2"))
    for call in (device, host_arrays):
        assert call(eng, p, capacity=0) == ([], len(want))
        assert call(eng, p, capacity=5) == (want[:5], len(want)) and len(want) > 5
        assert call(eng, p, capacity=len(want)) == (want, len(want))


def test_exclude_same_on_a_square_problem(eng):
    p = gen.square()
    full = gen.seed_rates_twin(p)
    assert device(eng, p) == (full, len(full)) and any(a == b for a, b, _ in full)
    ex = p._replace(exclude_same=True)
    want = [t for t in full if t[0] != t[1]]
    assert device(eng, ex) == (want, len(want)) and host_arrays(eng, ex) == (want, len(want))


def test_no_stale_bits_between_calls(eng):
    """the dense problem and then a sparse one of the same shape on one context: the bitmap is cleared by every call"""
    assert device(eng, gen.case("dense"))[0] == list(gen.expected("dense"))
    assert device(eng, gen.case("tol400_run2"))[0] == list(gen.expected("tol400_run2"))
    assert host_arrays(eng, gen.case("one_rate"))[0] == list(gen.expected("one_rate"))


def test_refusals_in_their_order(eng):
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd import _capi

    p = gen.square()
    d = OnDevice(p)

    def refused(what, args=None, rates=None, **over):
        a = list(d.args if args is None else args)
        if rates is not None:
            a[6] = rates
        with pytest.raises(vdf.VdfError) as ei:
            eng.align_seed_pairs_rates_device(*a, **dict(d.kw, **over))
        assert ei.value.code == _capi.VDF_E_INVAL and what in str(ei.value), (what, str(ei.value))

    ah, af, n_a, bh, bf, n_b, rates = d.args
    refused("null pointer", args=(0, af, n_a, bh, bf, n_b, rates), min_run=0)
    refused("min_run", min_run=0, rates=[])
    refused("pairs of videos", args=(ah, af, 4097, bh, bf, 4096, rates), rates=[])
    refused("n_rates", rates=[], exclude_same=True, args=(ah, af, n_a, bh, bf, n_b - 1, rates))
    refused("n_rates", rates=[(1, 1)] * 9, a_rate_first=None)
    refused("rate 1 must have", rates=[(37, 36), (1, 2)])          # the range comes before the limit on num, whatever the positions
    refused("rate 0 is above 32", rates=[(37, 36), (1, 1)])
    refused("exclude_same", exclude_same=True, args=(ah, af, n_a, bh, bf, n_b - 1, rates))
    # the first arrays come down and are checked
    down = p.a_first.copy()
    down[1, 2] = down[1, 1] - 1
    bad = OnDevice(p._replace(a_first=down))
    with pytest.raises(vdf.VdfError) as ei:
        eng.align_seed_pairs_rates_device(*bad.args, **bad.kw)
    assert "decreases at video 1 of rate 1" in str(ei.value)
    # an empty side: VDF_OK and nothing found
    assert eng.align_seed_pairs_rates_device(ah, af, 0, bh, bf, n_b, rates, **d.kw)[1] == 0
    assert eng.align_seed_pairs_rates_device(ah, af, n_a, bh, bf, 0, rates, **d.kw)[1] == 0
    # a multi-GPU context is refused, behind the other checks
    multi = vdf.Engine(devices=[0, 0])
    try:
        with pytest.raises(vdf.VdfError) as ei:
            multi.align_seed_pairs_rates_device(*d.args, **d.kw)
        assert ei.value.code == _capi.VDF_E_INVAL and "single-device" in str(ei.value)
        with pytest.raises(vdf.VdfError) as ei:
            multi.align_seed_pairs_rates(p.a_hashes, p.a_first, p.b_hashes, p.b_first, [(1, 1), (3, 1)], a_rate_first=p.a_rate_first)
        assert "must have" in str(ei.value)
    finally:
        multi.close()


def test_the_device_call_waits_for_copies_pending_on_its_stream(eng):
    """decoy contents first, a stretch of work, the real contents queued just before the call - all on the job's stream: the result is the real one's"""
    import torch

    real = gen.case("tol350_run3")
    want = list(gen.expected("tol350_run3"))
    rng = np.random.default_rng([83, 13])   # the decoy: the same layout without the planted cells, every skip byte of B set - nothing is a candidate
    decoy = real._replace(a_hashes=hashgen.random_hashes(rng, len(real.a_hashes)), b_hashes=hashgen.random_hashes(rng, len(real.b_hashes)),
                          a_skip=np.zeros_like(real.a_skip), b_skip=np.ones_like(real.b_skip))
    assert gen.seed_rates_twin(decoy) != want and decoy.a_hashes.shape == real.a_hashes.shape and np.array_equal(decoy.a_first, real.a_first)
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
        got, found = eng.align_seed_pairs_rates_device(*d.args, capacity=4096, stream=st.cuda_stream, **d.kw)
    st.synchronize()
    assert (gen.triples_of(got), found) == (want, len(want)), "the call ran ahead of the copies queued on its stream"


@pytest.mark.parametrize("seed", range(SEEDS))
def test_seeded_random_problems(eng, seed):
    p = gen.random_problem(np.random.default_rng([83, 11, seed]))
    want = gen.seed_rates_twin(p)
    assert device(eng, p) == (want, len(want)), (seed, p.rates, p.tol, p.min_run)
    if seed % 4 == 0:
        assert host_arrays(eng, p) == (want, len(want)), (seed, p.rates, p.tol, p.min_run)


def _excerpts(seed):
    """Six noise videos of three frame sizes, and four files that hold B[j] = A[c + (j * num) // den] of videos 0, 2, 4 and 5 - three different true rates"""
    rng = np.random.default_rng(seed)
    sizes = [(16, 16), (32, 24), (64, 48)]
    a = [rng.integers(0, 256, size=(f, sizes[i % 3][1], sizes[i % 3][0]), dtype=np.uint8) for i, f in enumerate((100, 90, 110, 80, 95, 85))]
    cut = lambda v, c, n, rate: np.ascontiguousarray(v[c + (np.arange(n) * rate[0]) // rate[1]])
    plan = {(0, 0): (0, 40, (6, 5)), (2, 1): (7, 36, (2, 1)), (4, 2): (13, 30, (6, 5)), (5, 3): (3, 33, (3, 2))}
    return a, [cut(a[i], c, n, rate) for (i, _), (c, n, rate) in sorted(plan.items(), key=lambda kv: kv[0][1])], plan


def test_end_to_end_one_pass_equals_one_call_per_rate(eng):
    import vid_dup_finder_lib_amd as vdf

    five = [(1, 1), (6, 5), (5, 4), (3, 2), (2, 1)]
    a, b, planted = _excerpts(23)
    pa, pb = [f"/a/{i}.mp4" for i in range(len(a))], [f"/b/{i}.mp4" for i in range(len(b))]
    wa = vdf.hash_frame_windows(a, pa, [len(v) for v in a], engine=eng, rates=five, one_call=True)
    wb = vdf.hash_frame_windows(b, pb, [len(v) for v in b], engine=eng, rates=[(1, 1)], one_call=True)[(1, 1)]
    for tolerance in (0.0, 0.35):
        today = vdf.align_rates(wa, wb, tolerance, 2, engine=eng, native=True, seed=True)
        assert vdf.align_rates(wa, wb, tolerance, 2, engine=eng, native=True, seed=True, one_pass=True) == today
        cand = vdf.candidate_pairs_rates(wa, wb, tolerance, 2, engine=eng)
        assert all({(r.a, r.b) for r in today[rate]} <= set(cand[rate]) for rate in five)
    best = {(r.a, r.b): r for r in vdf.best_rates(today, 0.35)}
    assert set(planted) <= set(best)
    for pair, (c, n, rate) in planted.items():
        assert (best[pair].num, best[pair].den) == rate, (pair, best[pair])
    listed = [(0, 0), (1, 1), (4, 2)]
    assert vdf.align_rates(wa, wb, 0.35, 2, engine=eng, native=True, seed=True, pairs=listed, one_pass=True) == \
        vdf.align_rates(wa, wb, 0.35, 2, engine=eng, native=True, seed=True, pairs=listed)
