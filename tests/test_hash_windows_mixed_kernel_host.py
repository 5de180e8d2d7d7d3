"""dct_hash_windows_mixed_kernel's own source text run on the CPU (tests/cpp/windows_mixed_kernel_host_main.cpp): 256 host threads per workgroup, real
barriers, wave ballots, in the manner of tests/test_hash_windows_kernel_host.py.  Five 16 x 16 videos of 16, 17, 33, 48 and 65 frames in ONE call, planned by
csrc/windows_mixed_plan.h as api.cpp plans them: under AddressSanitizer / UBSan every index the kernel forms is checked - the segment table its binary search
reads, the video's record, the frame addresses in a `small` of exactly the planned size, LDS, the output rows first[i] + k - and under ThreadSanitizer a barrier
missing between a write and a read of LDS is a data race.  Words and don't-care counts must be oracle.hash_clip's of each window's 16 frames, at the rows the
align calls read.  No GPU: this runs before the kernel goes to one."""
import os
import subprocess

import numpy as np
import pytest

import planegen
import windowgen
from oracle import vdf_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
CSRC = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
FRAMES = (16, 17, 33, 48, 65)
STRIDES = (1, 7, 16, 17)


def _cut(lines, first, last):
    i = next(k for k, ln in enumerate(lines) if first in ln)
    j = next(k for k in range(i + 1, len(lines)) if last in lines[k])
    return lines[i:j]


@pytest.fixture(scope="module")
def programs():
    os.makedirs(BUILD, exist_ok=True)
    lines = open(os.path.join(CSRC, "dct_hash.hip")).read().split("\n")
    text = _cut(lines, "struct DctTw {", "constexpr int kPadY") + [ln for ln in lines if ln.startswith("constexpr int kPadY") or ln.startswith("constexpr int kStrideT")]
    text += _cut(lines, "struct WindowsShared {", "struct WindowsSource {")  # the LDS layout both windows kernels share
    text += _cut(lines, "__device__ __forceinline__ uint32_t *windows_zero_words()", "// DWORDS: every frame starts on a dword boundary")
    text += _cut(lines, "// ---- window hashes of videos of different sizes and lengths in one launch", "hipError_t launch_dct_hash_windows_mixed")
    assert any("void dct_hash_windows_mixed_kernel(" in ln for ln in text) and not any("void dct_hash_windows_kernel(" in ln for ln in text)
    with open(os.path.join(BUILD, "windows_mixed_kernel.inc"), "w") as f:
        f.write("\n".join(text) + "\n")
    out = {}
    for name, san in (("asan", "address,undefined"), ("tsan", "thread")):
        exe = os.path.join(BUILD, "windows_mixed_kernel_host_" + name)
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fsanitize=" + san, "-fno-sanitize-recover=all", "-I", CSRC, "-I", BUILD,
                               "-o", exe, os.path.join(ROOT, "tests", "cpp", "windows_mixed_kernel_host_main.cpp")])
        out[name] = exe
    return out


@pytest.fixture(scope="module")
def videos():
    rng = np.random.default_rng(415)
    return [windowgen.video(rng, nf, 16, 16, lead=(0, 5, 3)[c % 3]) for c, nf in enumerate(FRAMES)]


_WANT = {}


def _oracle(videos, stride):
    """(words [rows, 16], zero planes [rows, 16], don't-care counts [rows], first) of the call, computed once per stride."""
    if stride not in _WANT:
        words, zero, dc, first = [], [], [], [0]
        for v in videos:
            for k in range(windowgen.n_windows(len(v), stride)):
                win = np.ascontiguousarray(v[k * stride:k * stride + 16])
                rc, w, coefs = orc.hash_clip(win, want_coefs=True)
                assert rc == 0
                w2, z, _ = planegen.oracle_planes(win)
                assert np.array_equal(w, w2)
                words.append(w)
                zero.append(z)
                dc.append(int((np.abs(coefs) < 1e-6).sum()))
            first.append(len(words))
        _WANT[stride] = (np.stack(words), np.stack(zero), np.array(dc, np.uint32), first)
    return _WANT[stride]


def _run(exe, videos, stride, planes):
    src, dst = os.path.join(BUILD, "windows_mixed_kernel_in.bin"), os.path.join(BUILD, "windows_mixed_kernel_out.bin")
    np.concatenate([v.reshape(-1) for v in videos]).tofile(src)
    r = subprocess.run([exe, src, str(stride), str(int(planes)), dst] + [str(len(v)) for v in videos], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "data race" not in r.stderr, r.stderr[-3000:]
    rows = sum(windowgen.n_windows(len(v), stride) for v in videos)
    raw = open(dst, "rb").read()
    assert len(raw) == rows * (128 * (2 if planes else 1) + 4)
    words = np.frombuffer(raw[:rows * 128], np.uint64).reshape(rows, 16)
    zero = np.frombuffer(raw[rows * 128:rows * 256], np.uint64).reshape(rows, 16) if planes else None
    return words, zero, np.frombuffer(raw[-rows * 4:], np.uint32)


def _check(exe, videos, stride, planes=False):
    import vid_dup_finder_lib_amd as vdf

    want, want_zero, want_dc, first = _oracle(videos, stride)
    assert vdf.hash_windows_first([len(v) for v in videos], stride).tolist() == first
    got, zero, dc = _run(exe, videos, stride, planes)
    for i in range(len(videos)):
        for k in range(first[i + 1] - first[i]):
            row = first[i] + k
            assert np.array_equal(got[row], want[row]), f"video {i} window {k} (row {row}): words differ from the oracle's"
            assert dc[row] == want_dc[row], f"video {i} window {k}: don't-care count"
            if planes:
                assert np.array_equal(zero[row], want_zero[row]), f"video {i} window {k}: zero plane"


@pytest.mark.parametrize("stride", STRIDES)
def test_kernel_text_on_the_cpu_matches_the_oracle_and_stays_in_bounds(programs, videos, stride):
    _check(programs["asan"], videos, stride)


def test_planes_form_on_the_cpu(programs, videos):
    _check(programs["asan"], videos, 7, planes=True)


@pytest.mark.parametrize("stride", STRIDES)
def test_every_lds_reuse_is_ordered_by_a_barrier(programs, videos, stride):
    _check(programs["tsan"], videos, stride)


def test_every_lds_reuse_of_the_planes_form_is_ordered_by_a_barrier(programs, videos):
    _check(programs["tsan"], videos, 17, planes=True)
