"""The planner behind vdf_hash_windows_u8_rates[_device] (csrc/windows_rates_plan.h) on the CPU: tests/cpp/windows_rates_plan_main.cpp, a stand-alone
program built with -fsanitize=address,undefined, walks every F in 16 .. 140 x stride {1, 2, 3, 16, 17, 40} x every subset of {1/1, 6/5, 5/4, 3/2, 31/16,
2/1} plus one list of 8 rates, and replays dct_hash_windows_rates_kernel's walk with the header's own functions: every window of every rate is hashed
exactly once and in its segment, every tap is resident in the ring of 64 slots when pass t reads it, no frame at or past f_end <= F is touched, no rate
is hashed while have < span.  The out_first it prints are the library's vdf_hash_window_count_rates; and the calls' error codes, in their order, as far
as they can be had without a GPU (a multi-GPU context cannot)."""
import ctypes as C
import os
import subprocess

import numpy as np

import retimedgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _count(lib, n_clips, f, stride, rates, want_first=True):
    num, den = np.array([r[0] for r in rates], np.uint32), np.array([r[1] for r in rates], np.uint32)
    first = np.full(len(rates) + 1, 12345, np.uintp)
    total = lib.vdf_hash_window_count_rates(n_clips, f, stride, len(rates), num.ctypes.data, den.ctypes.data, first.ctypes.data if want_first else None)
    return total, first.tolist()


def test_rates_planner_walk_ring_replay_and_row_offsets():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "windows_rates_plan")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "windows_rates_plan_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "windows rates plan ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    seen = 0
    for line in out.stdout.splitlines():
        if line.startswith("first "):
            p = line.split()
            f, stride, n_clips = int(p[1]), int(p[2]), int(p[3])
            rates = [tuple(int(x) for x in r.split("/")) for r in p[4].split(",")]
            firsts, total = [int(x) for x in p[5:-1]], int(p[-1])
            assert len(firsts) == len(rates)
            assert _count(lib, n_clips, f, stride, rates) == (total, firsts + [total]), line
            want = np.concatenate([[0], np.cumsum([n_clips * retimedgen.n_windows(f, stride, r) for r in rates])])  # the definition
            assert firsts + [total] == want.tolist(), line
            seen += 1
    assert seen >= 400


def test_window_count_rates_against_the_definition_and_its_refusals():
    from vid_dup_finder_lib_amd import _capi, engine

    lib = _capi.load()
    five = [(1, 1), (6, 5), (5, 4), (3, 2), (2, 1)]
    for f in (31, 47, 100):
        for stride in (1, 3, 17):
            n = [retimedgen.n_windows(f, stride, r) for r in five]
            assert _count(lib, 7, f, stride, five) == (7 * sum(n), np.concatenate([[0], 7 * np.cumsum(n)]).tolist())
            assert _count(lib, 7, f, stride, five, want_first=False)[0] == 7 * sum(n)
            total, first = engine.hash_window_count_rates(7, f, stride, five)
            assert total == 7 * sum(n) and first.tolist() == np.concatenate([[0], 7 * np.cumsum(n)]).tolist()
    assert _count(lib, 0, 40, 1, five) == (0, [0] * 6)
    assert _count(lib, 3, 30, 1, five) == (0, [0] * 6)            # 2/1 spans 31 frames: no window, no rows
    assert _count(lib, 3, 40, 1, [(1, 1), (5, 2)]) == (0, [0] * 3)  # a rate outside the range
    assert _count(lib, 3, 40, 0, five) == (0, [0] * 6)
    assert lib.vdf_hash_window_count_rates(3, 40, 1, 2, None, None, None) == 0
    assert _count(lib, 3, 40, 1, [(1, 1)] * 9)[0] == 0 and _count(lib, 3, 40, 1, [(1, 1)] * 8)[0] == 8 * 3 * 25
    assert lib.vdf_hash_window_count_rates(3, 40, 1, 0, None, None, None) == 0


def test_error_codes_that_need_no_context():
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    job = _capi.VdfWindowsRatesJob()
    for call in (lib.vdf_hash_windows_u8_rates, lib.vdf_hash_windows_u8_rates_device):
        assert call(None, C.byref(job)) == _capi.VDF_E_INVAL
        assert call(None, None) == _capi.VDF_E_INVAL
    assert _capi.WINDOWS_MAX_RATES == 8 and C.sizeof(_capi.VdfWindowsRatesJob) == 96
