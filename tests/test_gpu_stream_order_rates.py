"""vdf_hash_windows_u8_rates_device made while its stream still has work pending: the nine steps of tests/test_gpu_stream_order.py (its _Scenario, its
delay) for the one _device call whose stream travels in a job struct and not in a `void *stream` parameter, so that tests/streamcases.py does not list it.

  1. on st: a delay;                                   5. the library call, job.stream = st;
  2. on st: every output buffer filled with 0xAB;      6. on st: a snapshot of every output;
  3. on st: `real` copied into the input buffer;       7. on st: `decoy2` copied over the input buffer;
  4. st.query() must be False;                         8. st.synchronize();
                                                       9. snapshot and output buffer = the expectation on `real`.

The frames buffer holds `decoy` when the call is made.  Two videos of 40 frames at 64 x 64, rates [1/1, 3/2], the expectation from the oracle; the
HOST rate arrays are overwritten with another list the moment the call returns.  Run as the FIRST call of its frame size on a fresh context - the
cosine and resize tables go up inside the call - and then warm.  The non-gpu test below holds what the gpu test relies on: the expectation on `real`
differs from those on both decoys and from what the fill leaves behind."""
import functools

import numpy as np
import pytest

import streamcases as sc

N, FRAMES, H, W = 2, 40, 64, 64
RATES = [(1, 1), (3, 2)]
N_WIN = [FRAMES - 16 + 1, FRAMES - 23 + 1]
ROWS = N * sum(N_WIN)


@functools.lru_cache(maxsize=None)
def _case() -> sc.Case:
    def run(eng, p, hst, stream):
        from vid_dup_finder_lib_amd import _capi

        num, den = np.array([r[0] for r in RATES], np.uint32), np.array([r[1] for r in RATES], np.uint32)
        job = _capi.VdfWindowsRatesJob(p["frames"], N, FRAMES, W, H, W * H, FRAMES * W * H, 1, len(RATES), num.ctypes.data, den.ctypes.data, p["hashes"],
                                       p["dontcare"], stream)
        eng._check(eng.lib.vdf_hash_windows_u8_rates_device(eng.ctx, job))
        num[:], den[:] = (2, 5), (1, 4)  # the call has returned: its host arrays are the caller's again

    def expect(s):
        blocks = [[sc._oracle_windows(v, 1, rate) for v in s["frames"]] for rate in RATES]  # rate-major, clip by clip inside a rate
        return {"hashes": np.concatenate([x[0] for b in blocks for x in b]), "dontcare": np.concatenate([x[1] for b in blocks for x in b])}
    return sc.Case("hash_windows_rates_64x64", ("vdf_hash_windows_u8_rates_device",), [{"frames": sc._videos(7, k, N, FRAMES, H, W)} for k in range(3)], (),
                   {"hashes": ((ROWS, 16), sc.U64), "dontcare": ((ROWS,), sc.U32)}, (), run, expect, lambda s: None, True, {})


@functools.lru_cache(maxsize=None)
def _expected(k):
    c = _case()
    e = c.expect(c.sets[k])
    return {o: np.ascontiguousarray(e[o], dtype=dtype).reshape(shape) for o, (shape, dtype) in c.outputs.items()}


def test_the_decoys_are_valid_and_give_other_results():
    c = _case()
    assert not any(np.array_equal(c.sets[i]["frames"], c.sets[j]["frames"]) for i, j in ((0, 1), (0, 2), (1, 2)))
    real = _expected(0)
    for k in (1, 2):
        for key in real:
            assert not np.array_equal(real[key], _expected(k)[key]), f"the expected {key} on set {k} is the one on real - the case proves nothing"
    for key, (shape, dtype) in c.outputs.items():
        assert not np.array_equal(real[key], sc.filled(shape, dtype))
    # the blocks are the single-rate expectations one after the other
    plain = [sc._oracle_windows(v, 1, (1, 1)) for v in c.sets[0]["frames"]]
    assert np.array_equal(real["hashes"][:N * N_WIN[0]], np.concatenate([x[0] for x in plain])) and real["hashes"].shape == (ROWS, 16)


def _verdict(key, got):
    for k, what in ((1, "decoy: the call ran ahead of its stream"), (2, "decoy2: work was left behind on another stream")):
        if np.array_equal(got, _expected(k)[key]):
            return f"the result on {what}"
    if np.any(np.ascontiguousarray(got).view(np.uint8) == sc.FILL):
        return "neither real nor a decoy; it holds 0xAB bytes - not written, or not ordered behind the fill?"
    return "neither real nor a decoy"


def _run(eng):
    import torch
    from test_gpu_stream_order import _Scenario

    case, want = _case(), _expected(0)
    sn = _Scenario(case)
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    sn.queue_producers(st)
    case.run(eng, sn.ptrs, {}, st.cuda_stream)
    sn.queue_consumers(st)
    st.synchronize()
    snapshots, finals = sn.results()
    for n in case.outputs:
        assert np.array_equal(snapshots[n], want[n]), f"{n} right behind the call is {_verdict(n, snapshots[n])}"
        assert np.array_equal(finals[n], want[n]), f"{n} after the stream ran dry is {_verdict(n, finals[n])}"


@pytest.mark.gpu
def test_first_call_of_a_frame_size_then_warm():
    import vid_dup_finder_lib_amd as vdf

    eng = vdf.Engine(0)
    try:
        _run(eng)  # cold: the tables of this frame size go up inside the call
        _run(eng)
    finally:
        eng.close()
