"""The planner behind vdf_hash_windows_clips_u8* (csrc/windows_mixed_plan.h) on the CPU: tests/cpp/windows_mixed_plan_main.cpp, a stand-alone program built
with -fsanitize=address,undefined, walks random sets of 1 .. 40 videos (F in 16 .. 100, six frame sizes, boxes, padded strides) at every stride 1 .. 40: first is
the prefix sums of the window counts, every segment maps back to its video by the lookup the kernel runs, every window has exactly one segment, no frame index
reaches F_i, every frame the windows kernel can address in `small` is written by exactly one pseudo-clip frame and no pseudo-clip names a frame past the video's
last; the uniform rule; the argument checks in the header's order.  Then vdf_hash_windows_clips_first itself against numpy."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts(n_frames, stride):
    return np.array([(int(f) - 16) // stride + 1 for f in n_frames], np.int64)


def test_mixed_windows_planner_segments_lookup_and_pseudo_clips():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "windows_mixed_plan")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "windows_mixed_plan_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "windows mixed plan ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    # the first arrays the program printed are the library's and numpy's
    import vid_dup_finder_lib_amd as vdf

    seen = 0
    for line in out.stdout.splitlines():
        if line.startswith("first "):
            head, tail = line[6:].split(":")
            stride, *nf = (int(x) for x in head.split())
            want = np.concatenate([[0], np.cumsum(_counts(nf, stride))])
            assert [int(x) for x in tail.split()] == want.tolist(), line
            assert vdf.hash_windows_first(nf, stride).tolist() == want.tolist(), line
            seen += 1
    assert seen == 40


def test_first_is_the_prefix_sums_of_the_window_counts():
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    rng = np.random.default_rng(3)
    for stride in (1, 2, 7, 16, 17, 40, 1000):
        nf = rng.integers(16, 5000, size=200)
        first = vdf.hash_windows_first(nf, stride)
        assert first.dtype == np.uint32 and first.tolist() == np.concatenate([[0], np.cumsum(_counts(nf, stride))]).tolist()
        assert all(int(first[i + 1] - first[i]) == lib.vdf_hash_window_count(int(nf[i]), stride) for i in range(len(nf)))
    assert vdf.hash_windows_first([], 1).tolist() == [0]  # n_videos == 0
    assert vdf.hash_windows_first([16], 2**32 - 1).tolist() == [0, 1]
    # a total of 2^32 - 1 windows fits, 2^32 does not
    big = [2**31 + 15, 2**31 + 14]
    assert vdf.hash_windows_first(big, 1).tolist() == [0, 2**31, 2**32 - 1]
    with pytest.raises(vdf.VdfError) as ei:
        vdf.hash_windows_first([2**31 + 15, 2**31 + 15], 1)
    assert ei.value.code == _capi.VDF_E_INVAL
    assert vdf.hash_windows_first([2**31 + 15, 2**31 + 15], 2).tolist() == [0, 2**30, 2**31]  # (2^31 - 1) // 2 + 1 each
    with pytest.raises(vdf.VdfError) as ei:
        vdf.hash_windows_first([40, 15, 40], 1)  # F = 15
    assert ei.value.code == _capi.VDF_E_NOT_ENOUGH_FRAMES
    for bad in (0, -1, 2**32, 1.5):
        with pytest.raises(ValueError):
            vdf.hash_windows_first([40], bad)
    with pytest.raises(ValueError):
        vdf.hash_windows_first([2**32], 1)
    # the C entry point itself: null pointers and a zero stride
    nf = np.array([40, 50], np.uint32)
    first = np.zeros(3, np.uint32)
    assert lib.vdf_hash_windows_clips_first(nf.ctypes.data, 2, 0, first.ctypes.data) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_windows_clips_first(None, 2, 1, first.ctypes.data) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_windows_clips_first(nf.ctypes.data, 2, 1, None) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_windows_clips_first(None, 0, 1, first.ctypes.data) == _capi.VDF_OK and first[0] == 0
    assert lib.vdf_hash_windows_clips_first(nf.ctypes.data, 2, 1, first.ctypes.data) == _capi.VDF_OK and first.tolist() == [0, 25, 60]
