"""The planner behind vdf_align_windows_retimed* (csrc/align_retimed_plan.h) on the CPU: tests/cpp/align_retimed_plan_main.cpp, a
stand-alone program built with -fsanitize=address,undefined, walks every (phase, band) unit of every pair of 0 .. 140 x 0 .. 140 windows at seven
rates lane by lane with the header's own functions - every cell of every phase visited exactly once, no row index at or behind Na or Nb, the
two-level reduction of the band records equal to a brute-force twin's record - and walks lists of videos of mixed lengths through the chunks."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_align_retimed_planner_cells_rows_reduction_and_chunks():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "align_retimed_plan")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "align_retimed_plan_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "align retimed plan ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
