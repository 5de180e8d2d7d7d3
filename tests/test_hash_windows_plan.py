"""The planner behind vdf_hash_windows_u8[_device] (csrc/windows_plan.h) on the CPU: tests/cpp/windows_plan_main.cpp, a stand-alone program built with
-fsanitize=address,undefined, walks every (F, stride) with F in 16 .. 200 and stride in 1 .. 40: each window belongs to exactly one segment, a segment's frame
range holds all 16 frames of each of its windows, no frame index reaches F, the lead-in is at most 15 frames, and the window count is vdf_hash_window_count's.
It also replays the kernel's own walk (chunks of 16 into a ring of 32) per segment, and the resize stage's pseudo-clips."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_windows_planner_segments_walk_and_pseudo_clips():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "windows_plan")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "windows_plan_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "windows plan ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    # the counts the program printed per (F, stride) are the library's
    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    seen = 0
    for line in out.stdout.splitlines():
        if line.startswith("count "):
            _, f, s, n = line.split()
            assert lib.vdf_hash_window_count(int(f), int(s)) == int(n), line
            seen += 1
    assert seen == (200 - 16 + 1) * 40
