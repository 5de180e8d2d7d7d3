"""The class-major layout of the seeded alignment against the variants (csrc/window_class_layout.h: ONE statement for the kernels and their
host twin) on the CPU: tests/cpp/window_class_layout_main.cpp, a stand-alone program built with -fsanitize=address,undefined,
checks that the permutation is one to one on the 1024 bits of a hash, that the classes are where the header says and that every variant mask
is constant on them, that the distance identity equals the brute-force distance to the row vdf_window_variants_host derives - over random and
adversarial words: padding bits set, bits set in Z, H & Z != 0 - and that the bound the seed kernel exits on never exceeds a distance."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_class_layout_under_the_sanitizers():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "window_class_layout")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "window_class_layout_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "window class layout ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
