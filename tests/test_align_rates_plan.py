"""The planner behind vdf_align_windows_rates* (csrc/align_rates_plan.h) on the CPU: tests/cpp/align_rates_plan_main.cpp, a
stand-alone program built with -fsanitize=address,undefined, walks every (triple, phase, band) unit of one call - videos of 0 .. 70 x 0 .. 70
windows, seven rates in one list, other window counts of A in every rate's block - lane by lane with the headers' own functions: every cell visited
exactly once, no row at or behind Na or Nb, a_rate_first and the rate's row of a_first applied, the reduced records equal to a brute-force twin's,
and the chunks inside both bounds, closing inside a rate and across a rate boundary."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_align_rates_planner_cells_rows_reduction_and_chunks():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "align_rates_plan")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "align_rates_plan_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "align rates plan ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
