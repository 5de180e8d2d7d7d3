"""The several-rates library form of the retimed windows across the boundary, without a GPU: the three entry points and the job struct declared
in include/vdf.h, exported by libvdf_hip.so, bound by _capi.py, present on Engine, in host/vdf.hpp and in the Rust sys crate; null handles refused, not
dereferenced; vdf_hash_windows_clips_first_rates against numpy prefix sums, with its codes; and, against an Engine whose library is a recorder,
hash_frame_windows(list, rates=, one_call=True) making exactly ONE vdf_hash_windows_clips_u8_rates call with the right job, while without one_call it still
makes one uniform call per video and the refused combinations make no library call at all.  (The library's own checks that need a context are held on the GPU:
tests/test_gpu_hash_windows_clips_rates.py; their order without a context by tests/cpp/windows_mixed_rates_plan_main.cpp.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import retimedgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"vdf_hash_windows_clips_first_rates": 8, "vdf_hash_windows_clips_u8_rates": 2, "vdf_hash_windows_clips_u8_rates_device": 2}
FIVE = [(1, 1), (6, 5), (5, 4), (3, 2), (2, 1)]
EIGHT = [(2, 1), (1, 1), (6, 5), (3, 2), (5, 4), (12, 10), (31, 16), (2, 1)]


def test_the_three_symbols_and_the_job_are_declared_exported_and_bound():
    from vid_dup_finder_lib_amd import _capi

    raw = open(os.path.join(ROOT, "include", "vdf.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _capi.load()
    for name, n_args in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
        assert len(_capi.SIGNATURES[name][1]) == n_args, name
    # the job: field for field what the header declares, pointers and scalars only, the stream inside it
    body = re.search(r"typedef\s+struct\s+vdf_windows_clips_rates_job\s*\{(.*?)\}\s*vdf_windows_clips_rates_job\s*;", header, flags=re.S).group(1)
    fields = [re.match(r".*?(\w+)$", " ".join(f.split())).group(1) for f in body.split(";") if f.strip()]
    assert fields == [f for f, _ in _capi.VdfWindowsClipsRatesJob._fields_]
    assert fields == ["buf", "buf_bytes", "clips", "n_frames", "n_videos", "window_stride", "n_rates", "rate_num", "rate_den", "out_hashes", "out_dontcare", "stream"]
    assert C.sizeof(_capi.VdfWindowsClipsRatesJob) == 5 * 8 + 2 * 4 + 5 * 8
    assert not re.search(r"vdf_hash_windows_clips_u8_rates(_device)?\s*\([^)]*void\s*\*\s*stream", header)
    assert "takes one rate" not in raw  # neither parent call lists the combination among what is missing any more ...
    assert raw.count("vdf_hash_windows_clips_u8_rates[_device] below") == 2  # ... both point at the new call
    assert "Not here: zero planes, the batching queue, multi-GPU contexts (VDF_E_INVAL), rates outside [1, 2]" in raw
    hpp = open(os.path.join(ROOT, "vid_dup_finder_lib_amd", "host", "vdf.hpp")).read()
    assert "vdf_hash_windows_clips_u8_rates(" in hpp and "vdf_hash_windows_clips_u8_rates_device(" in hpp and "vdf_hash_windows_clips_first_rates(" in hpp
    assert "hash_windows_clips_rates(" in hpp and "hash_windows_clips_rates_device(" in hpp
    rs = open(os.path.join(ROOT, "rust", "vdf-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert "pub fn " + name in rs, name
    assert "pub struct vdf_windows_clips_rates_job" in rs and "pub clips: *const vdf_clip," in rs
    text = open(os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc", "dct_hash.hip")).read()
    assert "void dct_hash_windows_mixed_rates_kernel(" in text and "// ---- retimed window hashes of a mixed library at several rates in one launch" in text


def test_null_handles_are_refused_not_dereferenced():
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    job = _capi.VdfWindowsClipsRatesJob()
    for fn in (lib.vdf_hash_windows_clips_u8_rates, lib.vdf_hash_windows_clips_u8_rates_device):
        assert fn(None, C.byref(job)) == _capi.VDF_E_INVAL and fn(None, None) == _capi.VDF_E_INVAL


@pytest.mark.parametrize("rates", [[(1, 1), (2, 1)], [(2, 1)], FIVE, EIGHT, [(25, 24), (31, 16)]], ids=["1_1+2_1", "2_1", "five", "eight", "plain+31_16"])
@pytest.mark.parametrize("stride", [1, 7, 33])
def test_first_rates_is_the_prefix_sums_block_by_block(rates, stride):
    import vid_dup_finder_lib_amd as vdf

    nf = [31, 32, 33, 47, 48, 49, 63, 64, 65, 130]
    first, rate_first = vdf.hash_windows_first_rates(nf, rates, stride)
    assert first.dtype == np.uint32 and first.shape == (len(rates), len(nf) + 1) and rate_first.shape == (len(rates) + 1,)
    want = np.stack([np.concatenate([[0], np.cumsum([retimedgen.n_windows(f, stride, r) for f in nf])]) for r in rates])
    assert first.tolist() == want.tolist() and rate_first.tolist() == np.concatenate([[0], np.cumsum(want[:, -1])]).tolist()
    for r, rate in enumerate(rates):  # row r is exactly the single-rate call's first
        assert first[r].tolist() == vdf.hash_windows_first_retimed(nf, rate, stride).tolist()


def test_first_rates_error_codes_come_in_the_stated_order():
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd import _capi

    call = _capi.load().vdf_hash_windows_clips_first_rates
    first, rate_first = np.zeros(3 * 4, np.uint32), np.zeros(4, np.uintp)
    nf = np.array([40, 15, 30], np.uint32)  # video 1 below 16 frames, video 2 below the span of 2/1
    num, den = np.array([1, 5, 2], np.uint32), np.array([1, 2, 1], np.uint32)  # rate 1 is no rate
    p, n, d, f, rf = nf.ctypes.data, num.ctypes.data, den.ctypes.data, first.ctypes.data, rate_first.ctypes.data
    INVAL, SHORT = _capi.VDF_E_INVAL, _capi.VDF_E_NOT_ENOUGH_FRAMES
    assert call(p, 3, 1, 3, n, d, None, rf) == INVAL and call(None, 3, 1, 3, n, d, f, rf) == INVAL and call(p, 3, 0, 3, n, d, f, rf) == INVAL
    assert call(p, 3, 1, 0, n, d, f, rf) == INVAL and call(p, 3, 1, 9, n, d, f, rf) == INVAL
    assert call(p, 3, 1, 3, None, d, f, rf) == INVAL and call(p, 3, 1, 3, n, None, f, rf) == INVAL
    assert call(p, 3, 1, 3, n, d, f, rf) == SHORT  # below 16 frames: the plain rule, in front of the bad rate
    nf[1] = 31
    assert call(p, 3, 1, 3, n, d, f, rf) == INVAL  # the bad rate in front of the too-short video
    num[1], den[1] = 6, 5
    assert call(p, 3, 1, 3, n, d, f, rf) == SHORT  # 30 < span 31 of rate 2
    assert call(p, 3, 1, 2, n, d, f, rf) == _capi.VDF_OK and first[:8].tolist() == [0, 25, 41, 56, 0, 22, 35, 47] and rate_first[:3].tolist() == [0, 56, 103]
    nf[2] = 31
    assert call(p, 3, 1, 3, n, d, f, None) == _capi.VDF_OK and first.tolist() == [0, 25, 41, 57, 0, 22, 35, 48, 0, 10, 11, 12]  # rate_first may be null
    assert call(None, 0, 1, 3, n, d, f, rf) == _capi.VDF_OK and rate_first.tolist() == [0, 0, 0, 0]
    big = np.array([2**31 + 30], np.uint32)  # 2^31 + 15 plain windows: one block fits, two do not
    one = np.array([1, 1], np.uint32)
    assert call(big.ctypes.data, 1, 1, 1, one.ctypes.data, one.ctypes.data, f, rf) == _capi.VDF_OK and rate_first[1] == 2**31 + 15
    assert call(big.ctypes.data, 1, 1, 2, one.ctypes.data, one.ctypes.data, f, rf) == INVAL
    for rates, code in (([(1, 1), (5, 2)], INVAL), ([], INVAL), ([(1, 1)] * 9, INVAL), ([(1, 1), (2, 1)], SHORT)):
        with pytest.raises(vdf.VdfError) as ei:
            vdf.hash_windows_first_rates([40, 30], rates)
        assert ei.value.code == code
    for bad in (0, -1, 2**32, 1.5):
        with pytest.raises(ValueError):
            vdf.hash_windows_first_rates([40], FIVE, bad)
    for bad in ([(6,)], ["x"], [(1.5, 1)], [(-1, 1)], [(2**32, 1)]):
        with pytest.raises(ValueError):
            vdf.hash_windows_first_rates([40], bad)


def test_engine_has_the_new_surface():
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd.engine import Engine

    assert list(inspect.signature(Engine.hash_windows_clips_rates).parameters)[1:] == ["stacks", "rates", "stride", "crops", "want_dontcare"]
    assert callable(Engine.hash_windows_clips_rates_device) and callable(vdf.hash_windows_first_rates) and "hash_windows_first_rates" in vdf.__all__


def test_without_a_gpu_the_python_call_fails_loudly():
    import torch

    import vid_dup_finder_lib_amd as vdf

    if torch.cuda.is_available():
        return  # (tests/test_gpu_hash_windows_clips_rates.py is this call's test there)
    vids = [np.zeros((40, 8, 8), np.uint8), np.zeros((31, 4, 12), np.uint8)]
    with pytest.raises(vdf.VdfError) as ei:
        vdf.hash_frame_windows(vids, ["a", "b"], [1, 1], rates=FIVE, one_call=True)
    assert ei.value.code == -3  # VDF_E_HIP: no context, no fall-back


class _Lib:
    """Stands in for the library behind an Engine without a context: records the hash calls - with what the job's pointers hold at the time of the call - and
    answers `rc`.  Any other entry point is an error."""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def vdf_hash_windows_clips_u8_rates(self, ctx, job):
        from vid_dup_finder_lib_amd.engine import CLIP_DTYPE

        j = job._obj
        n, nr = j.n_videos, j.n_rates
        c = np.frombuffer((C.c_char * (n * CLIP_DTYPE.itemsize)).from_address(j.clips), CLIP_DTYPE).copy() if n else np.zeros(0, CLIP_DTYPE)
        f = np.frombuffer((C.c_char * (4 * n)).from_address(j.n_frames), np.uint32).copy() if n else np.zeros(0, np.uint32)
        num = np.frombuffer((C.c_char * (4 * nr)).from_address(j.rate_num), np.uint32).tolist()
        den = np.frombuffer((C.c_char * (4 * nr)).from_address(j.rate_den), np.uint32).tolist()
        self.calls.append(dict(kind="library", buf=j.buf, buf_bytes=j.buf_bytes, clips=c, n_frames=f.tolist(), n=n, stride=j.window_stride, rates=list(zip(num, den)),
                               out=j.out_hashes, dc=j.out_dontcare, stream=j.stream))
        return self.rc

    def vdf_hash_windows_u8_rates(self, ctx, job):
        j = job._obj
        num = np.frombuffer((C.c_char * (4 * j.n_rates)).from_address(j.rate_num), np.uint32).tolist()
        den = np.frombuffer((C.c_char * (4 * j.n_rates)).from_address(j.rate_den), np.uint32).tolist()
        self.calls.append(dict(kind="uniform", n=j.n_clips, n_frames=j.frames_per_clip, w=j.w, h=j.h, stride=j.window_stride, rates=list(zip(num, den))))
        return self.rc

    def vdf_last_error(self, ctx):
        return b"refused"

    def __getattr__(self, name):
        raise AssertionError("another entry point was called: " + name)


def _engine(rc=0):
    from vid_dup_finder_lib_amd.engine import Engine

    eng = Engine.__new__(Engine)
    eng.lib, eng.ctx = _Lib(rc), None
    return eng


VIDS = [np.zeros((40, 8, 8), np.uint8), np.zeros((31, 4, 12), np.uint8), np.zeros((65, 6, 6), np.uint8)]


@pytest.mark.parametrize("rates,stride", [(FIVE, 1), ([(2, 1), (1, 1)], 3), (EIGHT, 33), ([(3, 2)], 2)], ids=["five", "2_1+1_1", "eight", "3_2"])
def test_one_call_makes_exactly_one_library_call_with_the_right_job(rates, stride):
    import vid_dup_finder_lib_amd as vdf

    eng = _engine()
    by_rate = vdf.hash_frame_windows(VIDS, ["a", "b", "c"], [5, 6, 7], stride=stride, engine=eng, rates=rates, one_call=True)
    assert list(by_rate) == list(dict.fromkeys(rates))
    counts = {r: [retimedgen.n_windows(len(v), stride, r) for v in VIDS] for r in rates}
    for r in rates:
        wins = by_rate[r]
        assert [len(w) for w in wins] == counts[r] and wins[2][0].src_path() == "c" and wins[1][0].duration() == 6 and wins[0][0].zero is None
    assert len(eng.lib.calls) == 1
    c = eng.lib.calls[0]
    assert (c["kind"], c["n"], c["stride"], c["rates"], c["n_frames"], c["stream"]) == ("library", 3, stride, rates, [40, 31, 65], None)
    assert c["clips"]["offset"].tolist() == [0, 2560, 2560 + 1536] and c["clips"]["frame_stride"].tolist() == [64, 48, 36]
    assert c["clips"]["w"].tolist() == [8, 12, 6] and c["clips"]["h"].tolist() == [8, 4, 6] and not c["clips"]["crop"].any()
    assert c["buf_bytes"] == 2560 + 1536 + 2368 and c["buf"] and c["out"] and c["dc"] is None
    # the Engine call itself: the outputs sized by rate_first, cut into blocks, the don't-care counts on request, the boxes in the records
    words, first, dc = eng.hash_windows_clips_rates(VIDS, rates, stride, crops=[(1, 2, 0, 0), (0, 0, 1, 1), (0, 0, 0, 0)], want_dontcare=True)
    want_first, want_rate_first = vdf.hash_windows_first_rates([40, 31, 65], rates, stride)
    assert first.tolist() == want_first.tolist() == [np.concatenate([[0], np.cumsum(counts[r])]).tolist() for r in rates]
    assert [w.shape for w in words] == [(sum(counts[r]), 16) for r in rates] and [x.shape for x in dc] == [(sum(counts[r]),) for r in rates]
    assert all(w.dtype == np.uint64 for w in words) and all(x.dtype == np.uint32 for x in dc)
    c = eng.lib.calls[-1]
    assert c["out"] == words[0].ctypes.data and c["dc"] == dc[0].ctypes.data and c["clips"]["crop"].tolist() == [[1, 2, 0, 0], [0, 0, 1, 1], [0, 0, 0, 0]]
    for r in range(1, len(rates)):  # the blocks are one buffer, rate-major
        assert words[r].ctypes.data == words[0].ctypes.data + 128 * int(want_rate_first[r]) and dc[r].ctypes.data == dc[0].ctypes.data + 4 * int(want_rate_first[r])
    eng.lib.calls.clear()
    eng.lib.vdf_hash_windows_clips_u8_rates_device = lambda ctx, job: eng.lib.calls.append(job._obj) or 0
    eng.hash_windows_clips_rates_device(4096, 10000, c["clips"], [40, 31, 65], stride, rates, 8192, stream=7)
    j = eng.lib.calls[-1]
    assert (j.buf, j.buf_bytes, j.n_videos, j.window_stride, j.n_rates, j.out_hashes, j.out_dontcare, j.stream) == (4096, 10000, 3, stride, len(rates), 8192, None, 7)


def test_without_one_call_it_is_still_one_uniform_call_per_video():
    import vid_dup_finder_lib_amd as vdf

    eng = _engine()
    rates = [(2, 1), (1, 1)]
    by_rate = vdf.hash_frame_windows(VIDS, ["a", "b", "c"], [5, 6, 7], stride=3, engine=eng, rates=rates)
    assert [len(w) for w in by_rate[(2, 1)]] == [4, 1, 12] and [len(w) for w in by_rate[(1, 1)]] == [9, 6, 17]
    assert [(c["kind"], c["n"], c["n_frames"], c["w"], c["h"], c["stride"], c["rates"]) for c in eng.lib.calls] == [
        ("uniform", 1, 40, 8, 8, 3, rates), ("uniform", 1, 31, 12, 4, 3, rates), ("uniform", 1, 65, 6, 6, 3, rates)]


class _Stand:
    """A stand-in engine for the boxes: two videos of 3 and 2 windows at the first rate, 2 and 1 at the second."""

    def __init__(self):
        self.calls = []

    def hash_windows_clips_rates(self, stacks, rates, stride=1, crops=None, want_dontcare=False):
        self.calls.append(("library", [np.shape(s) for s in stacks], [tuple(r) for r in rates], stride, None if crops is None else np.asarray(crops).tolist()))
        return [np.arange(80, dtype=np.uint64).reshape(5, 16), 100 + np.arange(48, dtype=np.uint64).reshape(3, 16)], np.array([[0, 3, 5], [0, 2, 3]], np.uint32)

    def hash_clips_letterbox(self, stacks, want_dontcare=False):
        self.calls.append(("letterbox", [np.shape(s) for s in stacks]))
        return np.zeros((2, 16), np.uint64), np.array([[1, 1, 0, 0], [0, 0, 2, 1]], np.uint32)


def test_one_call_takes_crops_and_letterbox_as_the_plain_list_form_does():
    import vid_dup_finder_lib_amd as vdf

    vids = [np.zeros((40, 8, 8), np.uint8), np.zeros((33, 6, 10), np.uint8)]
    rates = [(6, 5), (2, 1)]
    eng = _Stand()
    got = vdf.hash_frame_windows(vids, ["a", "b"], [1, 2], stride=2, engine=eng, rates=rates, one_call=True, crops=[vdf.Crop((8, 8), 1, 0, 0, 2), (0, 1, 0, 0)])
    assert eng.calls == [("library", [(40, 8, 8), (33, 6, 10)], rates, 2, [[1, 0, 0, 2], [0, 1, 0, 0]])]
    assert [len(w) for w in got[(6, 5)]] == [3, 2] and [len(w) for w in got[(2, 1)]] == [2, 1]
    assert got[(6, 5)][1][0].hash[0] == 48 and got[(2, 1)][1][0].hash[0] == 132 and got[(2, 1)][1][0].src_path() == "b"
    eng.calls.clear()
    vdf.hash_frame_windows(vids, ["a", "b"], [1, 2], engine=eng, rates=rates, one_call=True, letterbox=True)
    assert eng.calls == [("letterbox", [(40, 8, 8), (33, 6, 10)]), ("library", [(40, 8, 8), (33, 6, 10)], rates, 1, [[1, 1, 0, 0], [0, 0, 2, 1]])]
    eng.calls.clear()
    with pytest.raises(ValueError):
        vdf.hash_frame_windows(vids, ["a", "b"], [1, 2], engine=eng, rates=rates, one_call=True, crops=[(0, 0, 0, 0)] * 2, letterbox=True)
    with pytest.raises(ValueError):
        vdf.hash_frame_windows(vids, ["a", "b"], [1, 2], engine=eng, rates=rates, one_call=True, crops=[(0, 0, 0, 0)])  # a Crop per video
    assert eng.calls == []


def test_the_refused_combinations_make_no_library_call():
    import vid_dup_finder_lib_amd as vdf

    eng = _Stand()
    vids = [np.zeros((40, 8, 8), np.uint8), np.zeros((33, 6, 10), np.uint8)]
    arr = np.zeros((2, 40, 8, 8), np.uint8)
    for frames, bad in ((arr, dict(one_call=True)), (arr, dict(crops=[(0, 0, 0, 0)] * 2)), (arr, dict(letterbox=True)), (arr, dict(one_call=True, letterbox=True)),
                        (vids, dict(one_call=True, rate=(2, 1))), (vids, dict(one_call=True, zero_plane=True)), (vids, dict(rate=(2, 1))), (vids, dict(zero_plane=True)),
                        (vids, dict(crops=[(0, 0, 0, 0)] * 2)), (vids, dict(letterbox=True)), (arr, dict(rate=(2, 1))), (arr, dict(zero_plane=True))):
        with pytest.raises(ValueError):
            vdf.hash_frame_windows(frames, ["a", "b"], [1, 2], engine=eng, rates=FIVE, **bad)
    assert eng.calls == []
    # a library error code reaches the caller as the exception the other forms raise
    with pytest.raises(vdf.NotEnoughFrames):
        vdf.hash_frame_windows(VIDS, ["a", "b", "c"], [5, 6, 7], engine=_engine(rc=-1), rates=FIVE, one_call=True)
    with pytest.raises(vdf.VdfError):
        vdf.hash_frame_windows(VIDS, ["a", "b", "c"], [5, 6, 7], engine=_engine(rc=-5), rates=FIVE, one_call=True)
