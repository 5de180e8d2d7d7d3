"""dct_hash_windows_retimed_kernel's own source text run on the CPU (tests/cpp/windows_retimed_kernel_host_main.cpp): 256 host threads per workgroup, real
barriers, wave ballots.  Under AddressSanitizer / UBSan every index the kernel forms is checked - the ring of 64 slots, the frames, the outputs - under
ThreadSanitizer a barrier missing between a write and a read of LDS is a data race, and the words and don't-care counts must be the oracle's hash of the
16 frames k * stride + tap(i) gathered into a stack.  No GPU: what can be known about the kernel before it runs on one."""
import os
import subprocess

import numpy as np
import pytest

import windowgen
from oracle import vdf_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
CSRC = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")


def _cut(lines, first, last):
    i = next(k for k, ln in enumerate(lines) if first in ln)
    j = next(k for k in range(i + 1, len(lines)) if last in lines[k])
    return lines[i:j]


@pytest.fixture(scope="module")
def programs():
    os.makedirs(BUILD, exist_ok=True)
    lines = open(os.path.join(CSRC, "dct_hash.hip")).read().split("\n")
    text = _cut(lines, "struct DctTw {", "constexpr int kPadY") + [ln for ln in lines if ln.startswith("constexpr int kPadY") or ln.startswith("constexpr int kStrideT")]
    text += _cut(lines, "struct WindowsSource {", "// The zero planes of the pair of windows in hand")  # where a frame is: shared with the plain kernel
    text += _cut(lines, "struct WindowsRetimedShared {", "hipError_t launch_dct_hash_windows_retimed")
    assert any("void dct_hash_windows_retimed_kernel(" in ln for ln in text) and not any("void dct_hash_windows_kernel(" in ln for ln in text)
    with open(os.path.join(BUILD, "windows_retimed_kernel.inc"), "w") as f:
        f.write("\n".join(text) + "\n")
    out = {}
    for name, san in (("asan", "address,undefined"), ("tsan", "thread")):
        exe = os.path.join(BUILD, "windows_retimed_kernel_host_" + name)
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fsanitize=" + san, "-fno-sanitize-recover=all", "-I", CSRC, "-I", BUILD,
                               "-o", exe, os.path.join(ROOT, "tests", "cpp", "windows_retimed_kernel_host_main.cpp")])
        out[name] = exe
    return out


def _taps(rate):
    return [(i * rate[0]) // rate[1] for i in range(16)]


def _run(exe, videos, stride, rate, frame_pad=0, clip_pad=0):
    n, nf = videos.shape[:2]
    fs = 256 + frame_pad
    cs = nf * fs + clip_pad
    buf = np.full(n * cs, 0xAA, np.uint8)
    for c in range(n):
        for f in range(nf):
            buf[c * cs + f * fs:c * cs + f * fs + 256] = videos[c, f].reshape(-1)
    buf = buf[:(n - 1) * cs + (nf - 1) * fs + 256]  # to the last byte of the last frame: a read past it is a heap overflow in the program
    src, dst = os.path.join(BUILD, "windows_retimed_kernel_in.bin"), os.path.join(BUILD, "windows_retimed_kernel_out.bin")
    buf.tofile(src)
    dwords = int(frame_pad % 4 == 0 and clip_pad % 4 == 0)
    r = subprocess.run([exe, src, str(n), str(nf), str(stride), str(rate[0]), str(rate[1]), str(fs), str(cs), str(dwords), dst], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "data race" not in r.stderr, r.stderr[-3000:]
    n_win = (nf - (_taps(rate)[15] + 1)) // stride + 1
    raw = open(dst, "rb").read()
    assert len(raw) == n * n_win * 132
    return np.frombuffer(raw[:n * n_win * 128], np.uint64).reshape(n, n_win, 16), np.frombuffer(raw[n * n_win * 128:], np.uint32).reshape(n, n_win)


def _check(exe, n, nf, stride, rate, **pads):
    rng = np.random.default_rng(nf * 131 + stride * 7 + rate[0])
    videos = np.stack([windowgen.video(rng, nf, 16, 16, lead=(0, 5, 3)[c % 3]) for c in range(n)])
    got, dc = _run(exe, videos, stride, rate, **pads)
    taps = np.array(_taps(rate))
    assert got.shape[1] >= 1
    for c in range(n):
        for k in range(got.shape[1]):
            rc, words, coefs = orc.hash_clip(np.ascontiguousarray(videos[c, k * stride + taps]), want_coefs=True)
            assert rc == 0 and np.array_equal(got[c, k], words), f"clip {c} window {k}: words differ from the oracle's on the gathered frames"
            assert dc[c, k] == int((np.abs(coefs) < 1e-6).sum()), f"clip {c} window {k}: don't-care count"


CASES = [(19, 1, (6, 5)), (31, 1, (2, 1)), (32, 1, (2, 1)), (47, 1, (2, 1)), (49, 3, (3, 2)), (65, 1, (31, 16)), (70, 16, (5, 4)), (80, 17, (2, 1))]


@pytest.mark.parametrize("n_frames,stride,rate", CASES)
def test_retimed_kernel_text_on_the_cpu_matches_the_oracle_and_stays_in_bounds(programs, n_frames, stride, rate):
    _check(programs["asan"], 1, n_frames, stride, rate)


def test_two_clips_at_padded_strides_read_by_bytes(programs):
    _check(programs["asan"], 2, 47, 3, (3, 2), frame_pad=3, clip_pad=5)


@pytest.mark.parametrize("n_frames,stride,rate", CASES)
def test_every_lds_reuse_of_the_retimed_kernel_is_ordered_by_a_barrier(programs, n_frames, stride, rate):
    _check(programs["tsan"], 1, n_frames, stride, rate)
