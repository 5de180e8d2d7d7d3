"""The planner behind vdf_align_windows_stretches[_device] (csrc/align_plan.h: AlignRect, align_rect_of, align_cell_masked, align_next_round) on the
CPU: tests/cpp/align_stretch_plan_main.cpp, a stand-alone program built with -fsanitize=address,undefined, replays for every (Na, Nb) in 0 .. 140 x
0 .. 140 the rectangle rule in every corner, on every edge and with guards that clamp nowhere, somewhere and everywhere, the masked band walk of the
kernel against a direct walk of every diagonal, and the round builder's survivors, unit offsets and rectangles over pair lists of mixed lengths."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_align_stretch_planner_rectangles_masked_walk_and_rounds():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "align_stretch_plan")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "align_stretch_plan_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "align stretch plan ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
