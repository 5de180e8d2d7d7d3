"""The planner behind vdf_hash_clips_u8[_device] (csrc/resize_dispatch.cpp: check_mixed, plan_mixed) on the CPU: tests/cpp/mixed_plan_main.cpp, compiled with
g++ from resize_dispatch.cpp and resize_tables.cpp alone (no HIP, no GPU), walks the partition into kernel parts, the uniform shortcut, the launch cuts, every
validation error with the clip it names, and - before any GPU run - the address envelope of every descriptor against the kernels' own careful-loader test."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mixed_planner_partition_envelope_and_errors():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "mixed_plan")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror=switch", "-o", exe, os.path.join(ROOT, "tests", "cpp", "mixed_plan_main.cpp"),
                           os.path.join(csrc, "resize_dispatch.cpp"), os.path.join(csrc, "resize_tables.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "mixed plan ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


def test_the_descriptor_the_kernels_read_is_the_one_the_planner_asserts():
    """MixedClipDesc is defined once (resize_dispatch.h, with static_asserts on its size and on every field offset) and the kernels name no other layout."""
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    hdr = open(os.path.join(csrc, "resize_dispatch.h")).read()
    assert hdr.count("struct MixedClipDesc {") == 1 and "sizeof(MixedClipDesc) == 48" in hdr and "offsetof(MixedClipDesc, pitch) == 44" in hdr
    for f in ("dct_hash.hip", "api.cpp", "vdf_internal.h"):
        assert "struct MixedClipDesc {" not in open(os.path.join(csrc, f)).read(), f
