"""csrc/hash_queue_mixed.cpp with Cropdetect::Letterbox under ThreadSanitizer, the GPU behind it replaced by stand-ins for both batch calls
(tests/cpp/queue_mixed_letterbox_tsan_main.cpp), built with the flags of tests/test_hash_queue_mixed_tsan.py: 48 callers with five clip sizes against a
letterbox queue and a plain queue alive together, every caller's box a function of its clip, an oversize clip refused while others are in flight.  A lost
wake-up is a hang (the timeout), a wrong hand-over a wrong value, an unlocked access a TSan report."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")


def test_mixed_letterbox_queue_logic_is_clean_under_tsan(tmp_path):
    exe = str(tmp_path / "queue_mixed_letterbox_tsan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-DVDF_QUEUE_SYSTEM_CLOCK", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "queue_mixed_letterbox_tsan_main.cpp"),
                           os.path.join(CSRC, "hash_queue_mixed.cpp"), "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "queue mixed letterbox tsan ok" in out.stdout and "ThreadSanitizer" not in out.stderr, (out.stdout[-1500:], out.stderr[-3000:])


def test_the_queue_sources_keep_their_rules():
    """hash_queue_mixed.cpp reads no environment and reaches the letterbox call through a weak declaration (the plain queue's stand-alone program stubs
    vdf_hash_clips_u8 only and must keep linking); hash_queue.cpp knows nothing of the mixed queue."""
    src = open(os.path.join(CSRC, "hash_queue_mixed.cpp")).read()
    assert "getenv" not in src and "__attribute__((weak))" in src
    assert "mixed" not in open(os.path.join(CSRC, "hash_queue.cpp")).read()
