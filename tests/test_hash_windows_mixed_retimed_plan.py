"""The planner behind vdf_hash_windows_clips_u8_retimed* (csrc/windows_mixed_retimed_plan.h) on the CPU: tests/cpp/windows_mixed_retimed_plan_main.cpp, a
stand-alone program built with -fsanitize=address,undefined, walks libraries of 1 .. 6 videos (frame counts from {span, span + 1, 31, 32, 33, 47, 48, 63, 64, 65,
130}, widths on both sides of 192, with and without boxes) at strides 1, 2, 7, 16, 17, 33, 40 and rates 6/5, 5/4, 3/2, 31/16, 2/1: first is the prefix sums of the
retimed window counts, every segment maps back to its video by the lookup the kernel runs, every window has exactly one segment, every frame a segment walks is
below F_i and inside the planned `small`, a replay of the ring finds every tap resident when pass t reads it; the check codes in the header's order; the uniform
and plain-tap routes.  Then vdf_hash_windows_clips_first_retimed itself against numpy and against the per-video count."""
import os
import subprocess

import numpy as np
import pytest

import retimedgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _first(n_frames, stride, rate):
    return np.concatenate([[0], np.cumsum([retimedgen.n_windows(int(f), stride, rate) for f in n_frames])]).astype(np.int64)


def test_mixed_retimed_planner_segments_lookup_frames_and_ring():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "windows_mixed_retimed_plan")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "windows_mixed_retimed_plan_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "windows mixed retimed plan ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    # the first arrays the program printed are the library's and numpy's
    import vid_dup_finder_lib_amd as vdf

    seen = 0
    for line in out.stdout.splitlines():
        if line.startswith("first "):
            head, tail = line[6:].split(":")
            stride, num, den, *nf = (int(x) for x in head.split())
            want = _first(nf, stride, (num, den))
            assert [int(x) for x in tail.split()] == want.tolist(), line
            assert vdf.hash_windows_first_retimed(nf, (num, den), stride).tolist() == want.tolist(), line
            seen += 1
    assert seen == 5 * 7


def test_first_retimed_is_the_prefix_sums_of_the_retimed_counts_and_its_error_codes():
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    rng = np.random.default_rng(418)
    for rate in retimedgen.RATES:
        for stride in (1, 2, 7, 16, 17, 40, 1000):
            nf = rng.integers(retimedgen.span(rate), 5000, size=100)
            first = vdf.hash_windows_first_retimed(nf, rate, stride)
            assert first.dtype == np.uint32 and first.tolist() == _first(nf, stride, rate).tolist()
            assert all(int(first[i + 1] - first[i]) == lib.vdf_hash_window_count_retimed(int(nf[i]), stride, *rate) for i in range(len(nf)))
    assert vdf.hash_windows_first_retimed([], (6, 5)).tolist() == [0]
    # plain taps: the plain call's first
    assert vdf.hash_windows_first_retimed([16, 40, 33], (25, 24), 3).tolist() == vdf.hash_windows_first([16, 40, 33], 3).tolist()
    nf = np.array([40, 50], np.uint32)
    first = np.zeros(3, np.uint32)
    call = lib.vdf_hash_windows_clips_first_retimed
    assert call(nf.ctypes.data, 2, 1, 2, 1, first.ctypes.data) == _capi.VDF_OK and first.tolist() == [0, 10, 30]
    # _first's rules: null pointers, a zero stride, a video below 16 frames, 2^32 windows
    assert call(nf.ctypes.data, 2, 0, 2, 1, first.ctypes.data) == _capi.VDF_E_INVAL
    assert call(None, 2, 1, 2, 1, first.ctypes.data) == _capi.VDF_E_INVAL
    assert call(nf.ctypes.data, 2, 1, 2, 1, None) == _capi.VDF_E_INVAL
    assert call(None, 0, 1, 2, 1, first.ctypes.data) == _capi.VDF_OK
    short = np.array([40, 15], np.uint32)
    assert call(short.ctypes.data, 2, 1, 5, 2, first.ctypes.data) == _capi.VDF_E_NOT_ENOUGH_FRAMES  # below 16 frames: in front of the bad rate
    big = np.array([2**31 + 30, 2**31 + 30], np.uint32)
    assert call(big.ctypes.data, 2, 1, 2, 1, first.ctypes.data) == _capi.VDF_E_INVAL
    assert call(big.ctypes.data, 2, 2, 2, 1, first.ctypes.data) == _capi.VDF_OK and first.tolist() == [0, 2**30, 2**31]
    # ... plus the two of the retimed call, the rate in front of the span
    short = np.array([40, 30], np.uint32)
    for bad in ((5, 2), (1, 0), (0, 0), (4, 5), (65536, 65536)):
        assert call(short.ctypes.data, 2, 1, *bad, first.ctypes.data) == _capi.VDF_E_INVAL
    assert call(short.ctypes.data, 2, 1, 2, 1, first.ctypes.data) == _capi.VDF_E_NOT_ENOUGH_FRAMES  # 30 < span 31
    assert call(short.ctypes.data, 2, 1, 31, 16, first.ctypes.data) == _capi.VDF_OK and first.tolist() == [0, 11, 12]  # span 30
    with pytest.raises(vdf.VdfError) as ei:
        vdf.hash_windows_first_retimed([40, 30], (2, 1))
    assert ei.value.code == _capi.VDF_E_NOT_ENOUGH_FRAMES
    with pytest.raises(vdf.VdfError) as ei:
        vdf.hash_windows_first_retimed([40, 30], (5, 2))
    assert ei.value.code == _capi.VDF_E_INVAL
    for bad in (0, -1, 2**32, 1.5):
        with pytest.raises(ValueError):
            vdf.hash_windows_first_retimed([40], (6, 5), bad)
    for bad in ((6,), "x", (1.5, 1), (-1, 1), (2**32, 1)):
        with pytest.raises(ValueError):
            vdf.hash_windows_first_retimed([40], bad)
