"""The index rule of vdf_window_variants_* (csrc/window_variant.h: ONE function for the kernel and its host twin) on the CPU:
tests/cpp/window_variant_main.cpp, a stand-alone program built with -fsanitize=address,undefined, replays it over first arrays with empty
videos in every position, one-window videos, sets that begin behind row 0 and the last video of the set - every source row inside its
video, every video's rows mapped onto themselves one to one, no read outside the first array."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_variant_rule_under_the_sanitizers():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "window_variant")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "window_variant_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "window variant rule ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
