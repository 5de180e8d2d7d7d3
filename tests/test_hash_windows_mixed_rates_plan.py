"""The planner behind vdf_hash_windows_clips_u8_rates* (csrc/windows_mixed_rates_plan.h) on the CPU: tests/cpp/windows_mixed_rates_plan_main.cpp, a
stand-alone program built with -fsanitize=address,undefined, walks libraries of 1 .. 6 videos (frame counts from {31, 32, 33, 47, 48, 49, 63, 64, 65, 130},
widths on both sides of 192, with and without boxes) at strides 1, 2, 7, 16, 17, 33, 40 and every subset of the rates {1/1, 6/5, 5/4, 3/2, 31/16, 2/1} plus one
8-rate list with a duplicate and an unreduced rate: every segment maps back to its video, every window of every rate is hashed once in the segment that owns
its start, a replay of the ring finds every tap resident when pass t reads it, nothing is read at or past frame_end <= F_i, no rate is served while
have < span_r, row0 is rate_first[r] + windows_first_retimed at rate r, the resize stage is plan_windows_mixed's descriptor for descriptor; the check codes
in the header's order (a bad rate behind an out-of-buffer video and in front of a too-short one); the uniform rule.  Then the first / rate_first arrays the
program printed against numpy and against vdf_hash_windows_clips_first_rates."""
import os
import subprocess

import numpy as np

import retimedgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _first(n_frames, stride, rates):
    first = np.stack([np.concatenate([[0], np.cumsum([retimedgen.n_windows(int(f), stride, r) for f in n_frames])]) for r in rates]).astype(np.int64)
    return first, np.concatenate([[0], np.cumsum(first[:, -1])])


def test_mixed_rates_planner_segments_lookup_frames_ring_rows_and_codes():
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "windows_mixed_rates_plan")
    csrc = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "windows_mixed_rates_plan_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "windows mixed rates plan ok" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    # the arrays the program printed are numpy's and the library's
    import vid_dup_finder_lib_amd as vdf

    seen = 0
    for line in out.stdout.splitlines():
        if line.startswith("first "):
            head, first_txt, rate_first_txt = line[6:].split(":")
            args, nf = head.split("|")
            stride, *rates = args.split()
            stride, rates, nf = int(stride), [tuple(int(x) for x in r.split("/")) for r in rates], [int(x) for x in nf.split()]
            want, want_rate_first = _first(nf, stride, rates)
            assert [int(x) for x in first_txt.split()] == want.reshape(-1).tolist(), line
            assert [int(x) for x in rate_first_txt.split()] == want_rate_first.tolist(), line
            got, got_rate_first = vdf.hash_windows_first_rates(nf, rates, stride)
            assert got.dtype == np.uint32 and got.tolist() == want.tolist() and got_rate_first.tolist() == want_rate_first.tolist(), line
            seen += 1
    assert seen == 9 * 7  # masks 8, 16, ... 64 and 63, at every stride
