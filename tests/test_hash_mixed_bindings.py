"""The mixed-size entry points across the boundary, without a GPU: declared in include/vdf.h, exported by libvdf_hip.so, bound by _capi.py with the record
layout the header gives (40 bytes), and - without a GPU - refusing loudly instead of computing anything on the CPU."""
import ctypes as C

import numpy as np
import pytest

NEW = ["vdf_hash_clips_u8", "vdf_hash_clips_u8_device", "vdf_hash_queue_create_mixed", "vdf_hash_queue_mixed_submit", "vdf_hash_queue_mixed_stats",
       "vdf_hash_queue_mixed_in_flight_max", "vdf_hash_queue_mixed_destroy"]


def test_new_symbols_are_exported_and_bound():
    from vid_dup_finder_lib_amd import _capi
    from vid_dup_finder_lib_amd.engine import CLIP_DTYPE

    lib = _capi.load()
    for name in NEW:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    assert C.sizeof(_capi.VdfClip) == 40 == CLIP_DTYPE.itemsize
    assert [CLIP_DTYPE.fields[f][1] for f in ("offset", "frame_stride", "w", "h", "crop")] == [0, 8, 16, 20, 24]
    assert [getattr(_capi.VdfClip, f).offset for f in ("offset", "frame_stride", "w", "h", "crop_left", "crop_bottom")] == [0, 8, 16, 20, 24, 36]


def test_null_handles_are_refused_not_dereferenced():
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    out = np.zeros(16, np.uint64)
    px = np.zeros(16, np.uint8)
    q = C.c_void_p()
    assert lib.vdf_hash_clips_u8(None, px.ctypes.data, 16, None, 0, 16, out.ctypes.data, None) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_clips_u8_device(None, None, 0, None, 0, 16, None, None, None) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_queue_create_mixed(None, 4096, 4, 0, 0, C.byref(q)) == _capi.VDF_E_INVAL and not q.value
    assert lib.vdf_hash_queue_mixed_submit(None, px.ctypes.data, 1, 1, out.ctypes.data) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_queue_mixed_stats(None, None, None) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_queue_mixed_in_flight_max(None, None) == _capi.VDF_E_INVAL
    lib.vdf_hash_queue_mixed_destroy(None)


def test_without_a_gpu_the_python_calls_fail_loudly():
    import torch

    import vid_dup_finder_lib_amd as vdf

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    clips = [np.zeros((16, 8, 8), np.uint8), np.zeros((16, 4, 12), np.uint8)]
    with pytest.raises(vdf.VdfError) as ei:
        vdf.hash_frame_stacks(clips, ["a", "b"], [1, 1])
    assert ei.value.code == -3  # VDF_E_HIP: no context, no fall-back
    with pytest.raises(vdf.VdfError):
        vdf.Engine(0).hash_clips(clips)
