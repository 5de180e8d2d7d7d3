"""host/vdf.hpp: VideoHash::align_windows_retimed[_pairs] compiled with g++ against libvdf_hip.so and run on the CPU
(tests/cpp/align_retimed_mirror_main.cpp): tiny inputs without a context take vdf_align_windows_retimed[_pairs]_host, the definition in plain C++."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_aligns_retimed_windows_on_the_cpu():
    lib = os.path.join(ROOT, "vid_dup_finder_lib_amd")
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "align_retimed_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(lib, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "align_retimed_mirror_main.cpp"), "-L" + lib, "-lvdf_hip", "-Wl,-rpath," + lib,
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "align retimed mirror ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
