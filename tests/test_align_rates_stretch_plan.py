"""The planner behind vdf_align_windows_rates_stretches* (csrc/align_rates_stretch_plan.h) on the CPU:
tests/cpp/align_rates_stretch_plan_main.cpp, a stand-alone program built with -fsanitize=address,undefined, runs rounds 0 .. 3 of every chunk of one
call - 40 x 40 videos of 0 .. 70 windows, five rates in one list, another window count per rate - lane by lane with the headers' own functions, the
rectangles read from the round's sealed upload: every cell visited once per round, a cell masked in exactly the rounds behind its rectangle, the
reduced records equal to a brute-force twin's rank by rank, the survivors of round k the triples with a record in round k - 1, chunks that close
inside a rate and across a rate boundary - and NO round behind a round without a record: the condition under which a call whose triples have no
record launches nothing but what vdf_align_windows_rates* launches."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_align_rates_stretch_planner_rounds_masks_and_survivors():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "align_rates_stretch_plan")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "align_rates_stretch_plan_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "align rates stretch plan ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
