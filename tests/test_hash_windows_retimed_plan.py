"""The planner behind vdf_hash_windows_u8_retimed[_device] (csrc/windows_retimed_plan.h) on the CPU: tests/cpp/windows_retimed_plan_main.cpp, a stand-alone
program built with -fsanitize=address,undefined, walks every F in 16 .. 130 x stride 1 .. 40 x rate {1/1, 25/24, 6/5, 5/4, 3/2, 31/16, 2/1}: the window count
is the definition's, the segments tile the windows, no frame >= F is walked, and a replay of the kernel's ring of 64 slots finds every tap of every window
resident in its slot when pass t reads it.  The counts it prints are the library's vdf_hash_window_count_retimed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_retimed_planner_counts_segments_walk_and_ring_replay():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "windows_retimed_plan")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "windows_retimed_plan_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "windows retimed plan ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    seen = 0
    for line in out.stdout.splitlines():
        if line.startswith("count "):
            f, s, num, den, n = (int(x) for x in line.split()[1:])
            assert lib.vdf_hash_window_count_retimed(f, s, num, den) == n, line
            span = (15 * num) // den + 1
            assert n == (0 if f < span else (f - span) // s + 1), line
            seen += 1
    assert seen == (130 - 16 + 1) * 40 * 7
