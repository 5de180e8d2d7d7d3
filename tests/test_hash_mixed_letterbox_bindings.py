"""The mixed letterbox entry points across the boundary, without a GPU: declared in include/vdf.h, exported by libvdf_hip.so, bound by _capi.py, present on Engine
and MixedHashQueue, and - without a GPU - refusing loudly instead of computing anything on the CPU.  gen_hashes on a list of stacks with its default cropdetect
reaches the library (before the mixed letterbox call it raised a numpy ValueError on the ragged list)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vdf_cropdetect_letterbox_clips_device", "vdf_hash_clips_u8_letterbox_device", "vdf_hash_clips_u8_letterbox", "vdf_hash_queue_create_mixed_letterbox",
       "vdf_hash_queue_mixed_submit_crop"]


def test_the_five_symbols_are_declared_exported_and_bound():
    from vid_dup_finder_lib_amd import _capi

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vdf.h")).read(), flags=re.S)
    lib = _capi.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    n_args = {name: len(_capi.SIGNATURES[name][1]) for name in NEW}
    assert n_args == {"vdf_cropdetect_letterbox_clips_device": 8, "vdf_hash_clips_u8_letterbox_device": 10, "vdf_hash_clips_u8_letterbox": 9,
                      "vdf_hash_queue_create_mixed_letterbox": 6, "vdf_hash_queue_mixed_submit_crop": 6}
    hpp = open(os.path.join(ROOT, "vid_dup_finder_lib_amd", "host", "vdf.hpp")).read()
    assert "vdf_hash_clips_u8_letterbox(" in hpp and "from_frame_stacks_letterbox" in hpp
    rs = open(os.path.join(ROOT, "rust", "vdf-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert "pub fn " + name in rs, name


def test_null_handles_are_refused_not_dereferenced():
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    out = np.zeros(16, np.uint64)
    crop = np.zeros(4, np.uint32)
    px = np.zeros(16, np.uint8)
    q = C.c_void_p()
    assert lib.vdf_cropdetect_letterbox_clips_device(None, None, 0, None, 0, 16, None, None) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_clips_u8_letterbox_device(None, None, 0, None, 0, 16, None, None, None, None) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_clips_u8_letterbox(None, px.ctypes.data, 16, None, 0, 16, out.ctypes.data, crop.ctypes.data, None) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_queue_create_mixed_letterbox(None, 4096, 4, 0, 0, C.byref(q)) == _capi.VDF_E_INVAL and not q.value
    assert lib.vdf_hash_queue_mixed_submit_crop(None, px.ctypes.data, 1, 1, out.ctypes.data, crop.ctypes.data) == _capi.VDF_E_INVAL


def test_engine_and_queue_have_the_new_surface():
    from vid_dup_finder_lib_amd.engine import Engine, MixedHashQueue

    for name in ("hash_clips_letterbox", "hash_clips_letterbox_device", "cropdetect_letterbox_clips_device"):
        assert callable(getattr(Engine, name)), name
    assert list(inspect.signature(Engine.hash_clips_letterbox).parameters)[1:] == ["stacks", "want_dontcare"]
    assert inspect.signature(MixedHashQueue.__init__).parameters["letterbox"].default is False
    assert callable(MixedHashQueue.submit_crop)
    # the packing of a list of stacks: every clip on a 64-byte boundary, whole frames, no box
    buf, clips, nf = Engine._pack_stacks([np.full((17, 5, 7), 3, np.uint8), np.full((16, 4, 12), 9, np.uint8)])
    assert nf == 16 and list(clips["offset"]) == [0, 576] and list(clips["frame_stride"]) == [35, 48] and not clips["crop"].any()
    assert len(buf) == 576 + 768 and (buf[:560] == 3).all() and (buf[560:576] == 0).all() and (buf[576:] == 9).all()


def test_without_a_gpu_the_python_calls_fail_loudly():
    import torch

    import vid_dup_finder_lib_amd as vdf

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(vdf.VdfError) as ei:
        vdf.Engine(0).hash_clips_letterbox([np.zeros((16, 8, 8), np.uint8)])
    assert ei.value.code == -3  # VDF_E_HIP: no context, no fall-back


def test_gen_hashes_on_a_list_with_the_default_cropdetect_reaches_the_library():
    """A stand-in engine records the call: the list goes to hash_clips_letterbox as it is (no numpy stacking of ragged clips), the words come back as VideoHashes
    and the boxes as Crops of each clip's own resolution; the library's errors keep their mapping."""
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd import _capi

    clips = [np.zeros((16, 8, 8), np.uint8), np.zeros((16, 4, 12), np.uint8)]

    class Recorder:
        def __init__(self, fail=None):
            self.calls, self.fail = [], fail

        def hash_clips_letterbox(self, stacks, want_dontcare=False):
            self.calls.append([np.shape(s) for s in stacks])
            if self.fail is not None:
                raise vdf.VdfError(self.fail, "refused")
            return np.arange(32, dtype=np.uint64).reshape(2, 16), np.array([[1, 2, 3, 4], [0, 0, 1, 0]], np.uint32)

        def hash_frames_letterbox(self, frames, want_dontcare=False):
            raise AssertionError("a list of stacks is not a uniform batch")

    rec = Recorder()
    vhs = vdf.gen_hashes(clips, ["a", "b"], [1, 2], engine=rec)  # default cropdetect: Letterbox
    assert rec.calls == [[(16, 8, 8), (16, 4, 12)]] and len(vhs) == 2 and np.array_equal(vhs[1].hash, np.arange(16, 32, dtype=np.uint64))
    crops = vdf.cropdetect_letterbox(clips, engine=rec)
    assert crops == [vdf.Crop.from_abi((8, 8), (1, 2, 3, 4)), vdf.Crop.from_abi((12, 4), (0, 0, 1, 0))]
    with pytest.raises(vdf.NotEnoughFrames):
        vdf.gen_hashes(clips, ["a", "b"], [1, 2], engine=Recorder(_capi.VDF_E_NOT_ENOUGH_FRAMES))
    with pytest.raises(vdf.VidProc):
        vdf.gen_hashes(clips, ["a", "b"], [1, 2], engine=Recorder(_capi.VDF_E_BAD_DIMS))
    with pytest.raises(vdf.VdfError):
        vdf.cropdetect_letterbox(clips, engine=Recorder(_capi.VDF_E_INVAL))


def test_gen_hashes_on_a_list_without_a_gpu_is_the_librarys_refusal():
    import torch

    import vid_dup_finder_lib_amd as vdf

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    clips = [np.zeros((16, 8, 8), np.uint8), np.zeros((16, 4, 12), np.uint8)]
    with pytest.raises(vdf.VdfError) as ei:  # not numpy's ValueError for a ragged list
        vdf.gen_hashes(clips, ["a", "b"], [1, 1])
    assert ei.value.code == -3
