"""Stream order is all the ordering there is (include/vdf.h, conventions): every _device call, made while its stream still has work pending.

For every case of tests/streamcases.py, on a fresh non-blocking torch stream `st` (nothing orders a pool stream against the context's own
stream), with every device input buffer holding `decoy` and no host synchronisation from the first step to the last:

  1. on st: a delay;                                   5. the library call, stream = st;
  2. on st: every output buffer filled with 0xAB;      6. on st: a snapshot of every output;
  3. on st: `real` copied into the input buffers;      7. on st: `decoy2` copied over every input buffer;
  4. st.query() must be False: the producers have      8. st.synchronize();
     not run when the call is made;                    9. snapshot, output buffer and what the call returned on the host = the expectation on `real`.

The expectation on `decoy`: the call ran ahead of its stream.  The one on `decoy2`, or a snapshot that differs from the buffer: it left work
behind on another stream.  0xAB: its writes were not ordered behind the fill.  HOST arrays of a call (clip descriptors, frame counts, crop
boxes, pair and triple lists) are overwritten with the decoy's the moment the call returns: "the call returns once the descriptors have
left the host".  The hash family runs twice, first as the FIRST call of its frame size on a fresh context - the uploads of the cosine and
resize tables are then under test too - and then warm.  Nothing is repeated to catch a race: the delay decides.

The delay is torch.cuda._sleep(DELAY_CYCLES).  Measured once on the MI355X with two events: _sleep(1 000 000) lasts 0.42 ms there (4.17 ms for
10 000 000), so DELAY_CYCLES = 48 000 000 is about 20 ms.  The host time from step 4 to the return of a warm call that only queues work was 0.01 to
0.05 ms (1.6 ms for the first vdf_bitmap_or_device of a context); calls that copy something from or to pageable host memory, or end with a wait,
return when the delay is over.  Step 4, not the number, is what the test relies on.

The control: vdf_hash_frames_u8_device at 64 x 64 with stream = 0, the context's own stream, while the producers sit on st.  The header
says that work is not waited for - and the hashes are those of `decoy`: the method sees a call that runs ahead."""
import os

import numpy as np
import pytest

import streamcases as sc

pytestmark = pytest.mark.gpu

DELAY_CYCLES = 48_000_000  # about 20 ms on the MI355X


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class _Scenario:
    """The buffers of one case on the device, every input holding `decoy`, and the steps above."""

    def __init__(self, case):
        import torch

        self.torch, self.case = torch, case
        dev = torch.device("cuda", 0)
        real, decoy, decoy2 = case.sets
        up = lambda a: torch.from_numpy(_bytes(a).copy()).to(dev)
        self.dev_names = [n for n in real if n not in case.host]
        self.inputs = {n: up(decoy[n]) for n in self.dev_names}
        self.stage_real = {n: up(real[n]) for n in self.dev_names}
        self.stage_decoy2 = {n: up(decoy2[n]) for n in self.dev_names if n not in case.inout}
        size = lambda n: int(np.prod(case.outputs[n][0])) * np.dtype(case.outputs[n][1]).itemsize
        self.outputs = {n: (self.inputs[n] if n in case.inout else torch.zeros(size(n), dtype=torch.uint8, device=dev)) for n in case.outputs}
        self.snapshots = {n: torch.zeros(size(n), dtype=torch.uint8, device=dev) for n in case.outputs}
        self.ptrs = {**{n: t.data_ptr() for n, t in self.inputs.items()}, **{n: t.data_ptr() for n, t in self.outputs.items()}}
        torch.cuda.synchronize()  # the uploads: the last host synchronisation before the scenario

    def queue_producers(self, st, fill_outputs=True):
        """steps 1 - 4"""
        torch = self.torch
        with torch.cuda.stream(st):
            torch.cuda._sleep(DELAY_CYCLES)
            if fill_outputs:
                for t in self.outputs.values():
                    t.fill_(sc.FILL)
            for n in self.dev_names:
                self.inputs[n].copy_(self.stage_real[n], non_blocking=True)
        assert not st.query(), "the delay was over before the call was made: the scenario proves nothing"

    def queue_consumers(self, st):
        """steps 6 and 7"""
        with self.torch.cuda.stream(st):
            for n, t in self.outputs.items():
                self.snapshots[n].copy_(t, non_blocking=True)
            for n, t in self.stage_decoy2.items():
                self.inputs[n].copy_(t, non_blocking=True)

    def results(self):
        back = lambda t, n: t.cpu().numpy().view(self.case.outputs[n][1]).reshape(self.case.outputs[n][0])
        return {n: back(t, n) for n, t in self.snapshots.items()}, {n: back(t, n) for n, t in self.outputs.items()}


def _verdict(name, key, got):
    for k, what in ((1, "decoy: the call ran ahead of its stream"), (2, "decoy2: work was left behind on another stream")):
        if sc.same(got, sc.expected(name, k)[key]):
            return f"the result on {what}"
    if isinstance(got, np.ndarray) and np.any(_bytes(got) == sc.FILL):
        return "neither real nor a decoy; it holds 0xAB bytes - not written, or not ordered behind the fill?"
    return "neither real nor a decoy"


def _run(name, eng):
    import torch

    case = sc.case(name)
    want = sc.expected(name, 0)
    sn = _Scenario(case)
    host = {n: case.sets[0][n].copy() for n in case.host}  # arrays this test owns
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    sn.queue_producers(st)
    returned = case.run(eng, sn.ptrs, host, st.cuda_stream)
    for n in case.host:  # the call has returned: its host arrays are the caller's again
        host[n][...] = case.sets[1][n]
    sn.queue_consumers(st)
    st.synchronize()
    snapshots, finals = sn.results()
    for n in case.outputs:
        assert np.array_equal(snapshots[n], want[n]), f"{name}: {n} right behind the call is {_verdict(name, n, snapshots[n])}"
        assert np.array_equal(finals[n], want[n]), f"{name}: {n} after the stream ran dry is {_verdict(name, n, finals[n])}"
    if "host" in want:
        assert sc.same(returned, want["host"]), f"{name}: what the call returned is {_verdict(name, 'host', returned)}"


def _engine(env):
    import vid_dup_finder_lib_amd as vdf

    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return vdf.Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


SEARCH = [n for n in sc.names() if n.startswith("search_")]


@pytest.mark.parametrize("name", [n for n in sc.names() if sc.is_cold(n)])
def test_first_call_of_a_frame_size_then_warm(name):
    eng = _engine(sc.case(name).env)
    try:
        _run(name, eng)  # cold: the tables of this frame size go up inside the call
        _run(name, eng)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def own_engine():
    eng = _engine({})
    yield eng
    eng.close()


@pytest.mark.parametrize("name", [n for n in sc.names() if not sc.is_cold(n) and n not in SEARCH])
def test_call_with_work_pending_on_its_stream(name, own_engine):
    _run(name, own_engine)


@pytest.mark.parametrize("name", SEARCH)
def test_search_with_work_pending_on_its_stream(name, engine):
    _run(name, engine)  # both Hamming backends


def test_control_a_call_on_another_stream_runs_ahead(own_engine):
    """stream = 0 is the context's own stream: the producers on st are not waited for, and the hashes are the decoy's.  (The fill of the
    outputs is made ahead of the scenario: queued on st it would land on the hashes the call has long written.)"""
    import torch

    name = "hash_frames_fused_64x64"
    case = sc.case(name)
    sn = _Scenario(case)
    for t in sn.outputs.values():
        t.fill_(sc.FILL)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=torch.device("cuda", 0))
    sn.queue_producers(st, fill_outputs=False)
    case.run(own_engine, sn.ptrs, {}, 0)
    sn.queue_consumers(st)
    torch.cuda.synchronize()
    _, finals = sn.results()
    for n in case.outputs:
        assert np.array_equal(finals[n], sc.expected(name, 1)[n]), f"{n} is {_verdict(name, n, finals[n])}, not the decoy's"
