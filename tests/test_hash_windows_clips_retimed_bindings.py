"""The library form of the retimed windows across the boundary, without a GPU: the three entry points declared in include/vdf.h, exported by
libvdf_hip.so, bound by _capi.py, present on Engine, in host/vdf.hpp and in the Rust sys crate; null contexts refused, not dereferenced;
vdf_hash_windows_clips_first_retimed against the per-video counts, with its error codes; and, against an Engine whose library is a recorder,
hash_frame_windows(list, rate=, one_call=True) making exactly ONE vdf_hash_windows_clips_u8_retimed call with the right descriptors, rate and output sizes, while
one_call=False still makes one uniform call per video and the refused combinations make no call at all.  (The library's own checks that need a context are
held on the GPU: tests/test_gpu_hash_windows_clips_retimed.py; their order without a context by tests/cpp/windows_mixed_retimed_plan_main.cpp.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import retimedgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"vdf_hash_windows_clips_first_retimed": 6, "vdf_hash_windows_clips_u8_retimed": 11, "vdf_hash_windows_clips_u8_retimed_device": 12}


def test_the_three_symbols_are_declared_exported_and_bound():
    from vid_dup_finder_lib_amd import _capi

    raw = open(os.path.join(ROOT, "include", "vdf.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _capi.load()
    for name, n_args in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
        assert len(_capi.SIGNATURES[name][1]) == n_args, name
    assert "the mixed-library form" not in raw  # the uniform retimed calls no longer list it among what is missing ...
    assert raw.count("Not here: zero planes of retimed windows") == 2  # ... and both forms still say what they leave out
    hpp = open(os.path.join(ROOT, "vid_dup_finder_lib_amd", "host", "vdf.hpp")).read()
    assert "vdf_hash_windows_clips_u8_retimed(" in hpp and "vdf_hash_windows_clips_u8_retimed_device(" in hpp and "vdf_hash_windows_clips_first_retimed(" in hpp
    assert "hash_windows_clips_retimed(" in hpp and "hash_windows_clips_retimed_device(" in hpp
    rs = open(os.path.join(ROOT, "rust", "vdf-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert "pub fn " + name in rs, name


def test_null_contexts_are_refused_not_dereferenced():
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    out = np.zeros(16, np.uint64)
    px = np.zeros(31 * 64, np.uint8)
    assert lib.vdf_hash_windows_clips_u8_retimed(None, px.ctypes.data, px.size, None, None, 0, 1, 2, 1, out.ctypes.data, None) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_windows_clips_u8_retimed_device(None, None, 0, None, None, 0, 1, 2, 1, None, None, None) == _capi.VDF_E_INVAL


@pytest.mark.parametrize("rate", retimedgen.RATES + [(1, 1), (25, 24)])
@pytest.mark.parametrize("stride", [1, 7, 33])
def test_first_retimed_matches_the_per_video_counts(rate, stride):
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    nf = [retimedgen.span(rate), retimedgen.span(rate) + 1, 31, 32, 33, 47, 48, 63, 64, 65, 130]
    first = vdf.hash_windows_first_retimed(nf, rate, stride)
    assert first.dtype == np.uint32 and first[0] == 0 and len(first) == len(nf) + 1
    for i, f in enumerate(nf):
        assert int(first[i + 1]) - int(first[i]) == lib.vdf_hash_window_count_retimed(f, stride, *rate) == retimedgen.n_windows(f, stride, rate) >= 1


def test_first_retimed_error_codes_come_in_the_stated_order():
    from vid_dup_finder_lib_amd import _capi

    call = _capi.load().vdf_hash_windows_clips_first_retimed
    first = np.zeros(4, np.uint32)
    nf = np.array([40, 15, 30], np.uint32)  # video 1 below 16 frames, video 2 below the span of 2/1
    p = nf.ctypes.data
    assert call(None, 3, 1, 5, 2, first.ctypes.data) == _capi.VDF_E_INVAL and call(p, 3, 1, 5, 2, None) == _capi.VDF_E_INVAL
    assert call(p, 3, 0, 5, 2, first.ctypes.data) == _capi.VDF_E_INVAL
    assert call(p, 3, 1, 5, 2, first.ctypes.data) == _capi.VDF_E_NOT_ENOUGH_FRAMES  # below 16 frames: the plain rule, in front of the bad rate
    nf[1] = 31
    assert call(p, 3, 1, 5, 2, first.ctypes.data) == _capi.VDF_E_INVAL  # the bad rate in front of the too-short video
    assert call(p, 3, 1, 2, 0, first.ctypes.data) == _capi.VDF_E_INVAL
    assert call(p, 3, 1, 2, 1, first.ctypes.data) == _capi.VDF_E_NOT_ENOUGH_FRAMES
    nf[2] = 31
    assert call(p, 3, 1, 2, 1, first.ctypes.data) == _capi.VDF_OK and first.tolist() == [0, 10, 11, 12]


def test_engine_has_the_new_surface():
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd.engine import Engine

    assert list(inspect.signature(Engine.hash_windows_clips_retimed).parameters)[1:] == ["stacks", "rate", "stride", "crops", "want_dontcare"]
    assert callable(Engine.hash_windows_clips_retimed_device) and callable(vdf.hash_windows_first_retimed)
    assert "one_call" in inspect.signature(vdf.hash_frame_windows).parameters
    assert inspect.signature(vdf.hash_frame_windows).parameters["one_call"].default is False


def test_without_a_gpu_the_python_call_fails_loudly():
    import torch

    import vid_dup_finder_lib_amd as vdf

    if torch.cuda.is_available():
        return  # (tests/test_gpu_hash_windows_clips_retimed.py is this call's test there)
    vids = [np.zeros((40, 8, 8), np.uint8), np.zeros((31, 4, 12), np.uint8)]
    with pytest.raises(vdf.VdfError) as ei:
        vdf.hash_frame_windows(vids, ["a", "b"], [1, 1], rate=(6, 5), one_call=True)
    assert ei.value.code == -3  # VDF_E_HIP: no context, no fall-back


class _Lib:
    """Stands in for the library behind an Engine without a context: records the hash calls - with what the pointers hold at the time of the call - and
    answers `rc`.  Any other entry point is an error."""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def vdf_hash_windows_clips_u8_retimed(self, ctx, buf, buf_bytes, clips, n_frames, n, stride, num, den, out, dc):
        from vid_dup_finder_lib_amd.engine import CLIP_DTYPE

        c = np.frombuffer((C.c_char * (n * CLIP_DTYPE.itemsize)).from_address(clips), CLIP_DTYPE).copy() if n else np.zeros(0, CLIP_DTYPE)
        f = np.frombuffer((C.c_char * (4 * n)).from_address(n_frames), np.uint32).copy() if n else np.zeros(0, np.uint32)
        self.calls.append(dict(kind="library", buf_bytes=buf_bytes, clips=c, n_frames=f.tolist(), n=n, stride=stride, rate=(num, den), out=out, dc=dc))
        return self.rc

    def vdf_hash_window_count_retimed(self, *a):
        from vid_dup_finder_lib_amd import _capi

        return _capi.load().vdf_hash_window_count_retimed(*a)

    def vdf_hash_windows_u8_retimed(self, ctx, p, nc, nf, w, h, fs, cs, stride, num, den, out, dc):
        self.calls.append(dict(kind="uniform", n=nc, n_frames=nf, w=w, h=h, stride=stride, rate=(num, den)))
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


@pytest.mark.parametrize("rate,stride", [((6, 5), 1), ((2, 1), 3), ((3, 2), 33), ((25, 24), 2)])
def test_one_call_makes_exactly_one_library_call_with_the_right_descriptors(rate, stride):
    import vid_dup_finder_lib_amd as vdf

    eng = _engine()
    wins = vdf.hash_frame_windows(VIDS, ["a", "b", "c"], [5, 6, 7], stride=stride, engine=eng, rate=rate, one_call=True)
    counts = [retimedgen.n_windows(len(v), stride, rate) for v in VIDS]
    assert [len(w) for w in wins] == counts and wins[2][0].src_path() == "c" and wins[1][0].duration() == 6 and wins[0][0].zero is None
    assert len(eng.lib.calls) == 1
    c = eng.lib.calls[0]
    assert (c["kind"], c["n"], c["stride"], c["rate"], c["n_frames"]) == ("library", 3, stride, rate, [40, 31, 65])
    assert c["clips"]["offset"].tolist() == [0, 2560, 2560 + 1536] and c["clips"]["frame_stride"].tolist() == [64, 48, 36]
    assert c["clips"]["w"].tolist() == [8, 12, 6] and c["clips"]["h"].tolist() == [8, 4, 6] and not c["clips"]["crop"].any()
    assert c["buf_bytes"] == 2560 + 1536 + 2368 and c["out"] and c["dc"] is None
    # the Engine call itself: the output sized by first[n], the don't-care counts on request, the boxes in the records
    words, first, dc = eng.hash_windows_clips_retimed(VIDS, rate, stride, crops=[(1, 2, 0, 0), (0, 0, 1, 1), (0, 0, 0, 0)], want_dontcare=True)
    assert first.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist() == vdf.hash_windows_first_retimed([40, 31, 65], rate, stride).tolist()
    assert words.shape == (sum(counts), 16) and words.dtype == np.uint64 and dc.shape == (sum(counts),) and dc.dtype == np.uint32
    c = eng.lib.calls[-1]
    assert c["out"] == words.ctypes.data and c["dc"] == dc.ctypes.data and c["clips"]["crop"].tolist() == [[1, 2, 0, 0], [0, 0, 1, 1], [0, 0, 0, 0]]
    eng.lib.calls.clear()
    eng.lib.vdf_hash_windows_clips_u8_retimed_device = lambda *a: eng.lib.calls.append(a) or 0
    eng.hash_windows_clips_retimed_device(4096, 10000, c["clips"], [40, 31, 65], stride, rate, 8192, stream=7)
    a = eng.lib.calls[-1]
    assert a[:3] == (None, 4096, 10000) and a[5:] == (3, stride) + rate + (8192, None, 7)


def test_one_call_false_still_makes_one_uniform_call_per_video():
    import vid_dup_finder_lib_amd as vdf

    eng = _engine()
    wins = vdf.hash_frame_windows(VIDS, ["a", "b", "c"], [5, 6, 7], stride=3, engine=eng, rate=(2, 1))
    assert [len(w) for w in wins] == [4, 1, 12]
    assert [(c["kind"], c["n"], c["n_frames"], c["w"], c["h"], c["stride"], c["rate"]) for c in eng.lib.calls] == [
        ("uniform", 1, 40, 8, 8, 3, (2, 1)), ("uniform", 1, 31, 12, 4, 3, (2, 1)), ("uniform", 1, 65, 6, 6, 3, (2, 1))]


class _Stand:
    """A stand-in engine for the boxes: two videos of 3 and 2 retimed windows."""

    def __init__(self):
        self.calls = []

    def hash_windows_clips_retimed(self, stacks, rate, stride=1, crops=None, want_dontcare=False):
        self.calls.append(("library", [np.shape(s) for s in stacks], tuple(rate), stride, None if crops is None else np.asarray(crops).tolist()))
        return np.arange(80, dtype=np.uint64).reshape(5, 16), np.array([0, 3, 5], np.uint32)

    def hash_clips_letterbox(self, stacks, want_dontcare=False):
        self.calls.append(("letterbox", [np.shape(s) for s in stacks]))
        return np.zeros((2, 16), np.uint64), np.array([[1, 1, 0, 0], [0, 0, 2, 1]], np.uint32)


def test_one_call_takes_crops_and_letterbox_as_the_plain_list_form_does():
    import vid_dup_finder_lib_amd as vdf

    vids = [np.zeros((33, 8, 8), np.uint8), np.zeros((32, 4, 12), np.uint8)]
    st = _Stand()
    wins = vdf.hash_frame_windows(vids, ["a", "b"], [7, 9], engine=st, rate=(2, 1), one_call=True, crops=[vdf.Crop.from_abi((8, 8), (1, 2, 0, 3)), (0, 0, 1, 1)])
    assert st.calls == [("library", [(33, 8, 8), (32, 4, 12)], (2, 1), 1, [[1, 2, 0, 3], [0, 0, 1, 1]])]
    assert [len(w) for w in wins] == [3, 2] and np.array_equal(wins[1][0].hash, np.arange(48, 64, dtype=np.uint64))
    st = _Stand()
    vdf.hash_frame_windows(vids, ["a", "b"], [7, 9], stride=2, engine=st, rate=(6, 5), one_call=True, letterbox=True)
    assert st.calls == [("letterbox", [(33, 8, 8), (32, 4, 12)]), ("library", [(33, 8, 8), (32, 4, 12)], (6, 5), 2, [[1, 1, 0, 0], [0, 0, 2, 1]])]


def test_the_refused_combinations_make_no_call():
    import vid_dup_finder_lib_amd as vdf

    eng = _engine()
    arr = np.zeros((2, 40, 8, 8), np.uint8)
    vids = VIDS[:2]
    two = (["a", "b"], [1, 1])
    refused = [
        (vids, dict(rate=(6, 5), zero_plane=True)), (vids, dict(rate=(6, 5), zero_plane=True, one_call=True)),  # zero planes together with a rate
        (arr, dict(crops=[(0, 0, 0, 0)] * 2)), (arr, dict(letterbox=True)),                                      # boxes with an ndarray
        (arr, dict(rate=(6, 5), crops=[(0, 0, 0, 0)] * 2, one_call=True)), (arr, dict(rate=(6, 5), letterbox=True)),
        (vids, dict(rate=(6, 5), crops=[(0, 0, 0, 0)] * 2)), (vids, dict(rate=(6, 5), letterbox=True)),        # boxes with a rate but without one_call
        (arr, dict(rate=(6, 5), one_call=True)), (vids, dict(one_call=True)), (arr, dict(one_call=True)),        # one_call with an ndarray or without a rate
        (vids, dict(rate=(6, 5), one_call=True, crops=[(0, 0, 0, 0)] * 2, letterbox=True)),                      # two sources of the same boxes
        (vids, dict(rate=(6, 5), one_call=True, crops=[(0, 0, 0, 0)])),                                          # a box per video
    ]
    for frames, kw in refused:
        with pytest.raises(ValueError):
            vdf.hash_frame_windows(frames, *two, engine=eng, **kw)
    # a bad rate or stride: before anything is sized or called
    for bad in ((-1, 1), (2**32, 1), (6, 5.5), (6,), 1.2, "65", (5, 2), (4, 5), (1, 0), (0, 0), (65536, 65536)):
        with pytest.raises(ValueError):
            vdf.hash_frame_windows(vids, *two, engine=eng, rate=bad, one_call=True)
        with pytest.raises(ValueError):
            eng.hash_windows_clips_retimed(vids, bad)
    for bad in (0, -1, 2**32, 1.5):
        with pytest.raises(ValueError):
            vdf.hash_frame_windows(vids, *two, stride=bad, engine=eng, rate=(6, 5), one_call=True)
    with pytest.raises(ValueError):
        eng.hash_windows_clips_retimed_device(0, 0, np.zeros(2, eng_clip_dtype()), [40], 1, (6, 5), 0)
    assert eng.lib.calls == []


def eng_clip_dtype():
    from vid_dup_finder_lib_amd.engine import CLIP_DTYPE

    return CLIP_DTYPE


def test_the_library_errors_are_mapped():
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd import _capi

    with pytest.raises(vdf.NotEnoughFrames):  # a video shorter than the span: the library names it
        vdf.hash_frame_windows([VIDS[0], np.zeros((30, 8, 8), np.uint8)], ["a", "b"], [1, 1], engine=_engine(_capi.VDF_E_NOT_ENOUGH_FRAMES), rate=(2, 1), one_call=True)
    with pytest.raises(vdf.VidProc):
        vdf.hash_frame_windows(VIDS[:2], ["a", "b"], [1, 1], engine=_engine(_capi.VDF_E_BAD_DIMS), rate=(2, 1), one_call=True)
    with pytest.raises(vdf.VdfError):
        vdf.hash_frame_windows(VIDS[:2], ["a", "b"], [1, 1], engine=_engine(_capi.VDF_E_INVAL), rate=(2, 1), one_call=True)
