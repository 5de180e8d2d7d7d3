"""dct_hash_windows_mixed_retimed_kernel's own source text run on the CPU (tests/cpp/windows_mixed_retimed_kernel_host_main.cpp): 256 host threads per
workgroup, real barriers, wave ballots, in the manner of tests/test_hash_windows_mixed_kernel_host.py.  Five 16 x 16 videos of 31, 32, 33, 48 and 65 frames in ONE
call, planned by csrc/windows_mixed_retimed_plan.h as api.cpp plans them: under AddressSanitizer / UBSan every index the kernel forms is checked - the segment
table its binary search reads, the video's record, the frame addresses in a `small` of exactly the planned size, the ring of 64 slots, the output rows
first[i] + k - and under ThreadSanitizer a barrier missing between a write and a read of LDS is a data race.  Words and don't-care counts must be
oracle.hash_clip's of each window's gathered frames k * stride + tap(t), at the rows the align calls read.  No GPU: this runs before the kernel goes to one."""
import os
import subprocess

import numpy as np
import pytest

import retimedgen
import windowgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
CSRC = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
FRAMES = (31, 32, 33, 48, 65)
CASES = [((6, 5), 1), ((3, 2), 7), ((2, 1), 1), ((2, 1), 16), ((31, 16), 17)]


def _cut(lines, first, last):
    i = next(k for k, ln in enumerate(lines) if first in ln)
    j = next(k for k in range(i + 1, len(lines)) if last in lines[k])
    return lines[i:j]


@pytest.fixture(scope="module")
def programs():
    os.makedirs(BUILD, exist_ok=True)
    lines = open(os.path.join(CSRC, "dct_hash.hip")).read().split("\n")
    text = _cut(lines, "struct DctTw {", "constexpr int kPadY") + [ln for ln in lines if ln.startswith("constexpr int kPadY") or ln.startswith("constexpr int kStrideT")]
    text += _cut(lines, "struct WindowsRetimedShared {", "// DWORDS: every frame starts on a dword boundary, as in dct_hash_windows_kernel")  # the LDS layout both retimed kernels share
    text += _cut(lines, "// ---- retimed window hashes of videos of different sizes and lengths in one launch", "hipError_t launch_dct_hash_windows_mixed_retimed")
    assert any("void dct_hash_windows_mixed_retimed_kernel(" in ln for ln in text)
    assert not any("void dct_hash_windows_retimed_kernel(" in ln or "void dct_hash_windows_mixed_kernel(" in ln for ln in text)
    with open(os.path.join(BUILD, "windows_mixed_retimed_kernel.inc"), "w") as f:
        f.write("\n".join(text) + "\n")
    out = {}
    for name, san in (("asan", "address,undefined"), ("tsan", "thread")):
        exe = os.path.join(BUILD, "windows_mixed_retimed_kernel_host_" + name)
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fsanitize=" + san, "-fno-sanitize-recover=all", "-I", CSRC, "-I", BUILD,
                               "-o", exe, os.path.join(ROOT, "tests", "cpp", "windows_mixed_retimed_kernel_host_main.cpp")])
        out[name] = exe
    return out


@pytest.fixture(scope="module")
def videos():
    rng = np.random.default_rng(418)
    return [windowgen.video(rng, nf, 16, 16, lead=(0, 5, 3)[c % 3]) for c, nf in enumerate(FRAMES)]


_WANT = {}


def _oracle(videos, rate, stride):
    """(words [rows, 16], don't-care counts [rows], first) of the call, computed once per (rate, stride) and shared by the two sanitizer builds."""
    if (rate, stride) not in _WANT:
        per = [retimedgen.oracle_windows(v, rate, stride) for v in videos]
        first = np.concatenate([[0], np.cumsum([len(w) for w, _ in per])]).tolist()
        _WANT[rate, stride] = (np.concatenate([w for w, _ in per]), np.concatenate([d for _, d in per]), first)
    return _WANT[rate, stride]


def _run(exe, videos, rate, stride):
    src, dst = os.path.join(BUILD, "windows_mixed_retimed_kernel_in.bin"), os.path.join(BUILD, "windows_mixed_retimed_kernel_out.bin")
    np.concatenate([v.reshape(-1) for v in videos]).tofile(src)
    r = subprocess.run([exe, src, str(stride), str(rate[0]), str(rate[1]), dst] + [str(len(v)) for v in videos], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "data race" not in r.stderr, r.stderr[-3000:]
    rows = sum(retimedgen.n_windows(len(v), stride, rate) for v in videos)
    raw = open(dst, "rb").read()
    assert len(raw) == rows * 132
    return np.frombuffer(raw[:rows * 128], np.uint64).reshape(rows, 16), np.frombuffer(raw[rows * 128:], np.uint32)


def _check(exe, videos, rate, stride):
    import vid_dup_finder_lib_amd as vdf

    want, want_dc, first = _oracle(videos, rate, stride)
    assert vdf.hash_windows_first_retimed([len(v) for v in videos], rate, stride).tolist() == first
    assert all(first[i + 1] > first[i] for i in range(len(videos)))  # every video has a window: 31 frames are the span of 2/1
    got, dc = _run(exe, videos, rate, stride)
    for i in range(len(videos)):
        for k in range(first[i + 1] - first[i]):
            row = first[i] + k
            assert np.array_equal(got[row], want[row]), f"video {i} window {k} (row {row}): words differ from the oracle's on the gathered frames"
            assert dc[row] == want_dc[row], f"video {i} window {k}: don't-care count"


@pytest.mark.parametrize("rate,stride", CASES)
def test_kernel_text_on_the_cpu_matches_the_oracle_and_stays_in_bounds(programs, videos, rate, stride):
    _check(programs["asan"], videos, rate, stride)


@pytest.mark.parametrize("rate,stride", CASES)
def test_every_lds_reuse_is_ordered_by_a_barrier(programs, videos, rate, stride):
    _check(programs["tsan"], videos, rate, stride)
