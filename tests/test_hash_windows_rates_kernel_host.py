"""dct_hash_windows_rates_kernel's own source text run on the CPU (tests/cpp/windows_rates_kernel_host_main.cpp): 256 host threads per workgroup, real
barriers, wave ballots.  Under AddressSanitizer / UBSan every index the kernel forms is checked - the ring of 64 slots, the frames, the rate-major
outputs - under ThreadSanitizer a barrier missing between a write and a read of LDS is a data race, and block r of the words and don't-care counts must be
the oracle's hash of the 16 frames k * stride + tap_r(i) gathered into a stack (retimedgen.oracle_windows).  No GPU: what can be known about the kernel
before it runs on one.  The first case is the one the retimed kernel never meets: a span of 31 behind a first chunk of 16 frames."""
import os
import subprocess

import numpy as np
import pytest

import retimedgen
import windowgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
CSRC = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")

FIVE = [(1, 1), (6, 5), (5, 4), (3, 2), (2, 1)]
EIGHT = [(2, 1), (1, 1), (6, 5), (3, 2), (5, 4), (12, 10), (31, 16), (2, 1)]  # 12/10 is 6/5 unreduced, 2/1 is listed twice


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
    text += _cut(lines, "struct WindowsRetimedShared {", "// DWORDS: every frame starts on a dword boundary")  # the LDS layout: the retimed kernel's
    text += _cut(lines, "// ---- retimed window hashes at several rates from one read of the frames", "hipError_t launch_dct_hash_windows_rates")
    assert any("void dct_hash_windows_rates_kernel(" in ln for ln in text)
    assert not any("void dct_hash_windows_retimed_kernel(" in ln for ln in text) and not any("void dct_hash_windows_kernel(" in ln for ln in text)
    with open(os.path.join(BUILD, "windows_rates_kernel.inc"), "w") as f:
        f.write("\n".join(text) + "\n")
    out = {}
    for name, san in (("asan", "address,undefined"), ("tsan", "thread")):
        exe = os.path.join(BUILD, "windows_rates_kernel_host_" + name)
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fsanitize=" + san, "-fno-sanitize-recover=all", "-I", CSRC, "-I", BUILD,
                               "-o", exe, os.path.join(ROOT, "tests", "cpp", "windows_rates_kernel_host_main.cpp")])
        out[name] = exe
    return out


def _run(exe, videos, stride, rates, frame_pad=0, clip_pad=0):
    n, nf = videos.shape[:2]
    fs = 256 + frame_pad
    cs = nf * fs + clip_pad
    buf = np.full(n * cs, 0xAA, np.uint8)
    for c in range(n):
        for f in range(nf):
            buf[c * cs + f * fs:c * cs + f * fs + 256] = videos[c, f].reshape(-1)
    buf = buf[:(n - 1) * cs + (nf - 1) * fs + 256]  # to the last byte of the last frame: a read past it is a heap overflow in the program
    src, dst = os.path.join(BUILD, "windows_rates_kernel_in.bin"), os.path.join(BUILD, "windows_rates_kernel_out.bin")
    buf.tofile(src)
    dwords = int(frame_pad % 4 == 0 and clip_pad % 4 == 0)
    r = subprocess.run([exe, src, str(n), str(nf), str(stride), ",".join("%d/%d" % x for x in rates), str(fs), str(cs), str(dwords), dst], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "data race" not in r.stderr, r.stderr[-3000:]
    n_win = [retimedgen.n_windows(nf, stride, x) for x in rates]
    total = n * sum(n_win)
    raw = open(dst, "rb").read()
    assert len(raw) == total * 132
    words, dc = np.frombuffer(raw[:total * 128], np.uint64).reshape(total, 16), np.frombuffer(raw[total * 128:], np.uint32)
    first = np.concatenate([[0], np.cumsum([n * x for x in n_win])])
    return [(words[first[i]:first[i + 1]].reshape(n, n_win[i], 16), dc[first[i]:first[i + 1]].reshape(n, n_win[i])) for i in range(len(rates))]


def _check(exe, n, nf, stride, rates, **pads):
    rng = np.random.default_rng(nf * 131 + stride * 7 + len(rates))
    videos = np.stack([windowgen.video(rng, nf, 16, 16, lead=(0, 5, 3)[c % 3]) for c in range(n)])
    blocks = _run(exe, videos, stride, rates, **pads)
    want = {}
    for r, (got, dc) in zip(rates, blocks):
        assert got.shape[1] >= 1
        for c in range(n):
            if (r, c) not in want:
                want[r, c] = retimedgen.oracle_windows(videos[c], r, stride)
            words, counts = want[r, c]
            assert np.array_equal(got[c], words), f"rate {r} clip {c}: words differ from the oracle's on the gathered frames"
            assert np.array_equal(dc[c], counts), f"rate {r} clip {c}: don't-care counts"


CASES = [(47, 1, [(1, 1), (2, 1)]), (31, 1, [(2, 1), (1, 1)]), (49, 3, [(6, 5), (3, 2), (2, 1)]), (65, 1, FIVE), (80, 17, [(5, 4), (2, 1)]), (70, 16, EIGHT)]


@pytest.mark.parametrize("n_frames,stride,rates", CASES)
def test_rates_kernel_text_on_the_cpu_matches_the_oracle_and_stays_in_bounds(programs, n_frames, stride, rates):
    _check(programs["asan"], 1, n_frames, stride, rates)


def test_two_clips_at_padded_strides_read_by_bytes(programs):
    _check(programs["asan"], 2, 47, 3, [(3, 2), (1, 1), (2, 1)], frame_pad=3, clip_pad=5)


@pytest.mark.parametrize("n_frames,stride,rates", CASES)
def test_every_lds_reuse_of_the_rates_kernel_is_ordered_by_a_barrier(programs, n_frames, stride, rates):
    _check(programs["tsan"], 1, n_frames, stride, rates)
