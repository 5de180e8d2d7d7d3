"""host/vdf.hpp: VideoHash::align_seed_pairs_rates_host compiled with g++ against libvdf_hip.so and run on the CPU
(tests/cpp/align_seed_rates_mirror_main.cpp): the job is built from hash_windows' lists, rate-major, and vdf_align_seed_pairs_rates_host answers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_seeds_the_retimed_alignment_on_the_cpu():
    lib = os.path.join(ROOT, "vid_dup_finder_lib_amd")
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "align_seed_rates_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(lib, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "align_seed_rates_mirror_main.cpp"), "-L" + lib, "-lvdf_hip", "-Wl,-rpath," + lib,
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "align seed rates mirror ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
