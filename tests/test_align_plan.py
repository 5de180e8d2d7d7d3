"""The planner and the lane-ownership rules behind vdf_align_windows[_device] (csrc/align_plan.h) on the CPU: tests/cpp/align_plan_main.cpp, a
stand-alone program built with -fsanitize=address,undefined, replays the band kernel's walk with the header's own functions for every (Na, Nb) in
0 .. 140 x 0 .. 140 - every cell visited by exactly one (band, lane, step), no band outside its ka range, every diagonal's state where the kernel
looks for it after each rotation, each row loaded once - and walks pair lists of mixed lengths in both modes through the chunks and launch cuts."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_align_planner_cells_states_rows_and_units():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "align_plan")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "align_plan_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "align plan ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
