"""csrc/hash_queue_mixed.cpp (the batching queue for clips of any frame size) under ThreadSanitizer with the GPU behind it replaced by stand-ins
(tests/cpp/queue_mixed_tsan_main.cpp), built with the flags of the uniform queue's test (tests/test_host_sanitizers.py): 48 callers with five clip
sizes against batches of 4, a byte budget that closes batches before the count does, batches that never fill, an oversize clip refused while
others are in flight.  A lost wake-up is a hang (the timeout), a wrong hand-over a wrong checksum, an unlocked access a TSan report."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mixed_batching_queue_logic_is_clean_under_tsan(tmp_path):
    exe = str(tmp_path / "queue_mixed_tsan")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-DVDF_QUEUE_SYSTEM_CLOCK", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "queue_mixed_tsan_main.cpp"),
                           os.path.join(csrc, "hash_queue_mixed.cpp"), "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "queue mixed tsan ok" in out.stdout and "ThreadSanitizer" not in out.stderr, (out.stdout[-1500:], out.stderr[-3000:])


def test_the_mixed_queue_reads_no_environment_and_leaves_the_uniform_queue_alone():
    """slots_per_gpu is a parameter: tests/test_knob_coverage.py pins one getenv in hash_queue.cpp and none in any new file."""
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    assert "getenv" not in open(os.path.join(csrc, "hash_queue_mixed.cpp")).read()
    assert "mixed" not in open(os.path.join(csrc, "hash_queue.cpp")).read()
