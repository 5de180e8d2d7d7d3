"""The planner behind the mixed letterbox calls (csrc/resize_dispatch.cpp: plan_letterbox_mixed) on the CPU: tests/cpp/mixed_letterbox_plan_main.cpp, compiled
with g++ from resize_dispatch.cpp and resize_tables.cpp alone (no HIP, no GPU), walks the partition into detect classes on both sides of h = 256 and 512, the cover
of every clip by one launch with both probes, the uniform shortcut, the launch cuts, the work lists' sizes against what the kernels index, both probed frames of
every descriptor against the buffer, and the place of the non-zero-crop error behind every error of check_mixed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")


def test_mixed_letterbox_planner_classes_cover_work_lists_and_errors():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "mixed_letterbox_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror=switch", "-o", exe, os.path.join(ROOT, "tests", "cpp", "mixed_letterbox_plan_main.cpp"),
                           os.path.join(CSRC, "resize_dispatch.cpp"), os.path.join(CSRC, "resize_tables.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "mixed letterbox plan ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


def test_the_probe_descriptor_is_defined_once_and_the_hash_descriptor_is_untouched():
    hdr = open(os.path.join(CSRC, "resize_dispatch.h")).read()
    assert hdr.count("struct LetterboxProbeDesc {") == 1 and "sizeof(LetterboxProbeDesc) == 32" in hdr and "offsetof(LetterboxProbeDesc, slot) == 24" in hdr
    assert "sizeof(MixedClipDesc) == 48" in hdr and "offsetof(MixedClipDesc, pitch) == 44" in hdr
    for f in ("cropdetect.hip", "api.cpp", "vdf_internal.h"):
        assert "struct LetterboxProbeDesc {" not in open(os.path.join(CSRC, f)).read(), f


def test_uniform_and_mixed_detect_kernels_share_their_bodies():
    """One copy of the walkers, the work-list append and the union: both pass-1 kernels call letterbox_frame_pass1, both pass-2 kernels letterbox_frame_sides."""
    src = open(os.path.join(CSRC, "cropdetect.hip")).read()
    assert src.count("void letterbox_frame_pass1(") == 1 and src.count("letterbox_frame_pass1(") == 3
    assert src.count("void letterbox_frame_sides(") == 1 and src.count("letterbox_frame_sides<kColumnBatch>(") == 2
    for once in ("bool strip_is_letterbox(", "uint32_t row_strips4(", "bool columns_narrow(", "uint32_t column_strips(", "atomicAdd(&work[k], 1u)"):
        assert src.count(once) == 1, once
