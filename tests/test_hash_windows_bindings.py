"""The window-hash entry points across the boundary, without a GPU: declared in include/vdf.h, exported by libvdf_hip.so, bound by _capi.py, refusing null
handles, counting windows on the host - and, without a GPU, refusing loudly instead of computing anything on the CPU."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vdf_hash_windows_u8", "vdf_hash_windows_u8_device", "vdf_hash_window_count"]
COUNTS = [((15, 1), 0), ((16, 1), 1), ((17, 1), 2), ((33, 1), 18), ((48, 3), 11), ((40, 7), 4), ((50, 16), 3), ((60, 17), 3), ((100, 40), 3), ((16, 0), 0)]


def test_new_symbols_are_declared_exported_and_bound():
    from vid_dup_finder_lib_amd import _capi

    header = open(os.path.join(ROOT, "include", "vdf.h")).read()
    lib = _capi.load()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    assert "Not here: zero planes of window hashes" in header  # the header says what the windows calls leave out


def test_null_handles_are_refused_not_dereferenced():
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    out = np.zeros(16, np.uint64)
    px = np.zeros(16 * 16 * 16, np.uint8)
    assert lib.vdf_hash_windows_u8(None, px.ctypes.data, 1, 16, 16, 16, 256, 4096, 1, out.ctypes.data, None) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_windows_u8_device(None, None, 0, 16, 16, 16, 256, 4096, 1, None, None, None) == _capi.VDF_E_INVAL


@pytest.mark.parametrize("args,want", COUNTS)
def test_window_count(args, want):
    from vid_dup_finder_lib_amd import _capi

    assert _capi.load().vdf_hash_window_count(*args) == want


def test_without_a_gpu_the_python_call_fails_loudly():
    import torch

    import vid_dup_finder_lib_amd as vdf

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(vdf.VdfError) as ei:
        vdf.hash_frame_windows(np.zeros((1, 20, 8, 8), np.uint8), ["a"], [1])
    assert ei.value.code == -3  # VDF_E_HIP: no context, no fall-back
    with pytest.raises(vdf.VdfError):
        vdf.Engine(0).hash_windows(np.zeros((1, 20, 8, 8), np.uint8))


def test_a_bad_stride_or_short_lists_are_refused_before_anything_is_sized_or_called():
    """ctypes wraps an out-of-range stride into uint32_t without a word (-1 -> 2^32 - 1, 2^32 + 1 -> 1): the library would then write a different
    number of windows than the output was sized for.  The Python mirror refuses such a stride - and path / duration lists shorter than the
    videos - before it touches the library: the engine here has no context and a library that fails the test when called."""
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd.engine import Engine

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)

    eng = Engine.__new__(Engine)
    eng.lib, eng.ctx = NoLib(), None
    frames = np.zeros((1, 20, 8, 8), np.uint8)
    for bad in (0, -1, 2**32, 2**32 + 1, 1.5):
        with pytest.raises(ValueError):
            eng.hash_windows(frames, bad)
        with pytest.raises(ValueError):
            eng.hash_windows_device(0, 1, 20, 8, 8, bad, 0)
        with pytest.raises(ValueError):
            vdf.hash_frame_windows(frames, ["a"], [1], stride=bad, engine=eng)
    for paths, durations in (([], [1]), (["a"], [])):
        with pytest.raises(ValueError):
            vdf.hash_frame_windows(frames, paths, durations, engine=eng)
