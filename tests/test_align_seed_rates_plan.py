"""The planner behind vdf_align_seed_pairs_rates* (csrc/align_seed_rates_plan.h) on the CPU: tests/cpp/align_seed_rates_plan_main.cpp,
a stand-alone program built with -fsanitize=address,undefined, walks the units of the plan as the seed kernel walks them for window counts 0 .. 140
per video and seven rates in one list: every (seed, row) cell of the definition is visited by exactly one (unit, lane, k), no gathered row lies at or
behind its video's end, no chunk straddles a class, and sentinels appear only in a class's last tile."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_align_seed_rates_planner_seeds_rows_chunks_and_units():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "align_seed_rates_plan")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "align_seed_rates_plan_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "align seed rates plan ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
