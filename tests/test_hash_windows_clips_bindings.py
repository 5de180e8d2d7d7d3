"""The mixed windows entry points across the boundary, without a GPU: declared in include/vdf.h, exported by libvdf_hip.so, bound by _capi.py, present on
Engine, in host/vdf.hpp and in the Rust sys crate; a null context is refused, not dereferenced; without a GPU the python calls fail loudly instead of
computing anything on the CPU; the packing of a list of videos; and hash_frame_windows on a list of stacks - what it passes on, how it cuts the rows into
per-video lists, how it maps the library's errors - against a stand-in engine.  (The order of the library's own argument checks is held by
tests/cpp/windows_mixed_plan_main.cpp for the checks that need no context, and on the GPU by tests/test_gpu_hash_windows_clips.py.)"""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"vdf_hash_windows_clips_first": 4, "vdf_hash_windows_clips_u8": 9, "vdf_hash_windows_clips_u8_device": 10, "vdf_hash_windows_clips_u8_planes": 10,
       "vdf_hash_windows_clips_u8_planes_device": 11}


def test_the_five_symbols_are_declared_exported_and_bound():
    from vid_dup_finder_lib_amd import _capi

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vdf.h")).read(), flags=re.S)
    lib = _capi.load()
    for name, n_args in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
        assert len(_capi.SIGNATURES[name][1]) == n_args, name
    hpp = open(os.path.join(ROOT, "vid_dup_finder_lib_amd", "host", "vdf.hpp")).read()
    assert "vdf_hash_windows_clips_u8(" in hpp and "vdf_hash_windows_clips_u8_device(" in hpp and "hash_windows_clips_device" in hpp
    rs = open(os.path.join(ROOT, "rust", "vdf-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert "pub fn " + name in rs, name


def test_null_contexts_are_refused_not_dereferenced():
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    out = np.zeros(16, np.uint64)
    px = np.zeros(16 * 64, np.uint8)
    assert lib.vdf_hash_windows_clips_u8(None, px.ctypes.data, px.size, None, None, 0, 1, out.ctypes.data, None) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_windows_clips_u8_device(None, None, 0, None, None, 0, 1, None, None, None) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_windows_clips_u8_planes(None, px.ctypes.data, px.size, None, None, 0, 1, out.ctypes.data, None, out.ctypes.data) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_windows_clips_u8_planes_device(None, None, 0, None, None, 0, 1, None, None, None, None) == _capi.VDF_E_INVAL


def test_engine_has_the_new_surface_and_packs_whole_videos():
    from vid_dup_finder_lib_amd.engine import Engine

    for name in ("hash_windows_clips", "hash_windows_clips_planes", "hash_windows_clips_device", "hash_windows_clips_planes_device"):
        assert callable(getattr(Engine, name)), name
    assert list(inspect.signature(Engine.hash_windows_clips).parameters)[1:] == ["stacks", "stride", "crops", "want_dontcare"]
    assert list(inspect.signature(Engine.hash_windows_clips_planes).parameters)[1:] == ["stacks", "stride", "crops", "want_dontcare"]
    # ALL frames of every video, every video on a 64-byte boundary, the boxes in the records
    buf, clips, nf = Engine._pack_videos([np.full((17, 5, 7), 3, np.uint8), np.full((40, 4, 12), 9, np.uint8)], crops=[(1, 2, 0, 0), (0, 0, 1, 1)])
    assert nf.tolist() == [17, 40] and list(clips["offset"]) == [0, 640] and list(clips["frame_stride"]) == [35, 48]
    assert clips["crop"].tolist() == [[1, 2, 0, 0], [0, 0, 1, 1]]
    assert len(buf) == 640 + 1920 and (buf[:595] == 3).all() and (buf[595:640] == 0).all() and (buf[640:] == 9).all()
    with pytest.raises(ValueError):
        Engine._pack_videos([np.zeros((16, 8), np.uint8)])


def test_without_a_gpu_the_python_calls_fail_loudly():
    import torch

    import vid_dup_finder_lib_amd as vdf

    if torch.cuda.is_available():
        return  # (tests/test_gpu_hash_windows_clips.py is this call's test there)
    with pytest.raises(vdf.VdfError) as ei:
        vdf.Engine(0).hash_windows_clips([np.zeros((20, 8, 8), np.uint8)])
    assert ei.value.code == -3  # VDF_E_HIP: no context, no fall-back
    with pytest.raises(vdf.VdfError) as ei:  # ... and not numpy's ValueError for a ragged list
        vdf.hash_frame_windows([np.zeros((20, 8, 8), np.uint8), np.zeros((31, 4, 12), np.uint8)], ["a", "b"], [1, 1])
    assert ei.value.code == -3


class Recorder:
    """A stand-in engine: two videos of 3 and 2 windows."""

    def __init__(self, fail=None):
        self.calls, self.fail = [], fail

    def _words(self):
        if self.fail is not None:
            import vid_dup_finder_lib_amd as vdf

            raise vdf.VdfError(self.fail, "refused")
        return np.arange(80, dtype=np.uint64).reshape(5, 16), np.array([0, 3, 5], np.uint32)

    def hash_windows_clips(self, stacks, stride=1, crops=None, want_dontcare=False):
        self.calls.append(("plain", [np.shape(s) for s in stacks], stride, None if crops is None else np.asarray(crops).tolist()))
        return self._words()

    def hash_windows_clips_planes(self, stacks, stride=1, crops=None, want_dontcare=False):
        self.calls.append(("planes", [np.shape(s) for s in stacks], stride, None if crops is None else np.asarray(crops).tolist()))
        words, first = self._words()
        return words, words + np.uint64(1000), first

    def hash_clips_letterbox(self, stacks, want_dontcare=False):
        self.calls.append(("letterbox", [np.shape(s) for s in stacks]))
        return np.zeros((2, 16), np.uint64), np.array([[1, 1, 0, 0], [0, 0, 2, 1]], np.uint32)

    def hash_windows(self, *a, **k):
        raise AssertionError("a list of stacks is not a uniform batch")

    hash_windows_planes = hash_windows


def test_hash_frame_windows_on_a_list_cuts_the_rows_at_first():
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd import _capi

    vids = [np.zeros((18, 8, 8), np.uint8), np.zeros((17, 4, 12), np.uint8)]
    rec = Recorder()
    wins = vdf.hash_frame_windows(vids, ["a", "b"], [7, 9], stride=1, engine=rec)
    assert rec.calls == [("plain", [(18, 8, 8), (17, 4, 12)], 1, None)]
    assert [len(w) for w in wins] == [3, 2] and np.array_equal(wins[1][0].hash, np.arange(48, 64, dtype=np.uint64)) and wins[1][1].src_path() == "b"
    assert wins[0][0].zero is None
    # crops: a Crop or four edge offsets per video, in the C ABI's order
    rec = Recorder()
    vdf.hash_frame_windows(vids, ["a", "b"], [7, 9], stride=2, engine=rec, crops=[vdf.Crop.from_abi((8, 8), (1, 2, 0, 3)), (0, 0, 1, 1)])
    assert rec.calls == [("plain", [(18, 8, 8), (17, 4, 12)], 2, [[1, 2, 0, 3], [0, 0, 1, 1]])]
    # letterbox: the mixed letterbox call's boxes, passed in; with zero_plane the planes form
    rec = Recorder()
    wins = vdf.hash_frame_windows(vids, ["a", "b"], [7, 9], engine=rec, letterbox=True, zero_plane=True)
    assert rec.calls == [("letterbox", [(18, 8, 8), (17, 4, 12)]), ("planes", [(18, 8, 8), (17, 4, 12)], 1, [[1, 1, 0, 0], [0, 0, 2, 1]])]
    assert np.array_equal(wins[0][2].zero, np.arange(32, 48, dtype=np.uint64) + np.uint64(1000))
    # what is refused before the library is asked, and how the library's errors are mapped
    with pytest.raises(ValueError):
        vdf.hash_frame_windows(vids, ["a", "b"], [7, 9], engine=Recorder(), crops=[(0, 0, 0, 0)] * 2, letterbox=True)
    with pytest.raises(ValueError):
        vdf.hash_frame_windows(vids, ["a", "b"], [7, 9], engine=Recorder(), crops=[(0, 0, 0, 0)])
    with pytest.raises(ValueError):
        vdf.hash_frame_windows(vids, ["a"], [7, 9], engine=Recorder())
    with pytest.raises(ValueError):
        vdf.hash_frame_windows(np.zeros((2, 16, 8, 8), np.uint8), ["a", "b"], [7, 9], engine=Recorder(), letterbox=True)
    with pytest.raises(vdf.NotEnoughFrames):
        vdf.hash_frame_windows(vids, ["a", "b"], [7, 9], engine=Recorder(_capi.VDF_E_NOT_ENOUGH_FRAMES))
    with pytest.raises(vdf.VidProc):
        vdf.hash_frame_windows(vids, ["a", "b"], [7, 9], engine=Recorder(_capi.VDF_E_BAD_DIMS), zero_plane=True)
    with pytest.raises(vdf.VdfError):
        vdf.hash_frame_windows(vids, ["a", "b"], [7, 9], engine=Recorder(_capi.VDF_E_INVAL))


def test_the_mirror_refuses_what_ctypes_would_wrap():
    from vid_dup_finder_lib_amd.engine import Engine

    class NoContext(Engine):
        def __init__(self):  # no library call is reached below
            pass

    e = NoContext()
    for bad in (0, -1, 2**32, 1.5):
        with pytest.raises(ValueError):
            e.hash_windows_clips([np.zeros((16, 8, 8), np.uint8)], stride=bad)
    with pytest.raises(ValueError):
        e.hash_windows_clips_device(0, 0, np.zeros(2, [("offset", "<u8"), ("frame_stride", "<u8"), ("w", "<u4"), ("h", "<u4"), ("crop", "<u4", (4,))]), [16], 1, 0)
