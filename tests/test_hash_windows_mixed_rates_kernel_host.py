"""dct_hash_windows_mixed_rates_kernel's own source text run on the CPU (tests/cpp/windows_mixed_rates_kernel_host_main.cpp): 256 host threads per
workgroup, real barriers, wave ballots, in the manner of tests/test_hash_windows_mixed_retimed_kernel_host.py and tests/test_hash_windows_rates_kernel_host.py.
Five 16 x 16 videos of 31, 47, 49, 33 and 65 frames in ONE call at several rates, planned by csrc/windows_mixed_rates_plan.h as api.cpp plans them: under
AddressSanitizer / UBSan every index the kernel forms is checked - the segment table its binary search reads, the video's record, row0, the frame
addresses in a `small` of exactly the planned size, the ring of 64 slots, the output rows - and under ThreadSanitizer a barrier missing between a write and
a read of LDS is a data race.  Every block must be oracle.hash_clip's of each window's gathered frames k * stride + tap_r(t) at the rows
rate_first[r] + first[r][i] + k, and the WHOLE prefilled buffer is compared: a row nobody wrote keeps its ones.  No GPU: this runs before the kernel goes
to one.  The first case is the trap: F = 47 has have = 16 < span = 31 behind its first chunk, F = 49 has a last segment that owns nothing of 2/1, F = 31
has exactly one 2/1 window."""
import os
import subprocess

import numpy as np
import pytest

import retimedgen
import windowgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
CSRC = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
FRAMES = (31, 47, 49, 33, 65)
FIVE = [(1, 1), (6, 5), (5, 4), (3, 2), (2, 1)]
EIGHT = [(2, 1), (1, 1), (6, 5), (3, 2), (5, 4), (12, 10), (31, 16), (2, 1)]  # 12/10 is 6/5 unreduced, 2/1 is listed twice
CASES = [([(1, 1), (2, 1)], 1), ([(2, 1), (1, 1)], 1), ([(6, 5), (3, 2), (2, 1)], 3), (FIVE, 1), ([(5, 4), (2, 1)], 17), (EIGHT, 16)]


def _cut(lines, first, last):
    i = next(k for k, ln in enumerate(lines) if first in ln)
    j = next(k for k in range(i + 1, len(lines)) if last in lines[k])
    return lines[i:j]


@pytest.fixture(scope="module")
def programs():
    os.makedirs(BUILD, exist_ok=True)
    lines = open(os.path.join(CSRC, "dct_hash.hip")).read().split("\n")
    text = _cut(lines, "struct DctTw {", "constexpr int kPadY") + [ln for ln in lines if ln.startswith("constexpr int kPadY") or ln.startswith("constexpr int kStrideT")]
    text += _cut(lines, "struct WindowsRetimedShared {", "// DWORDS: every frame starts on a dword boundary, as in dct_hash_windows_kernel")  # the LDS layout of all retimed kernels
    text += _cut(lines, "// ---- retimed window hashes of a mixed library at several rates in one launch", "hipError_t launch_dct_hash_windows_mixed_rates")
    assert any("void dct_hash_windows_mixed_rates_kernel(" in ln for ln in text)
    assert not any("void dct_hash_windows_rates_kernel(" in ln or "void dct_hash_windows_mixed_retimed_kernel(" in ln or "void dct_hash_windows_retimed_kernel(" in ln
                   for ln in text)
    assert not any("asm" in ln for ln in text)  # ordinary stores: no inline assembly in the kernel's text
    with open(os.path.join(BUILD, "windows_mixed_rates_kernel.inc"), "w") as f:
        f.write("\n".join(text) + "\n")
    out = {}
    for name, san in (("asan", "address,undefined"), ("tsan", "thread")):
        exe = os.path.join(BUILD, "windows_mixed_rates_kernel_host_" + name)
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fsanitize=" + san, "-fno-sanitize-recover=all", "-I", CSRC, "-I", BUILD,
                               "-o", exe, os.path.join(ROOT, "tests", "cpp", "windows_mixed_rates_kernel_host_main.cpp")])
        out[name] = exe
    return out


@pytest.fixture(scope="module")
def videos():
    rng = np.random.default_rng(421)
    return [windowgen.video(rng, nf, 16, 16, lead=(0, 5, 3)[c % 3]) for c, nf in enumerate(FRAMES)]


_ORACLE = {}


def _want(videos, rates, stride):
    """(words [rows, 16], don't-care counts [rows], first [n_rates][n + 1], rate_first) of the call; the oracle of a (video, rate, stride) runs once for
    all cases and both sanitizer builds."""
    words, counts, first = [], [], []
    for r in rates:
        per = []
        for i, v in enumerate(videos):
            if (i, r, stride) not in _ORACLE:
                _ORACLE[i, r, stride] = retimedgen.oracle_windows(v, r, stride)
            per.append(_ORACLE[i, r, stride])
        first.append(np.concatenate([[0], np.cumsum([len(w) for w, _ in per])]))
        words += [w for w, _ in per]
        counts += [d for _, d in per]
    rate_first = np.concatenate([[0], np.cumsum([f[-1] for f in first])])
    return np.concatenate(words), np.concatenate(counts), np.stack(first), rate_first


def _run(exe, videos, rates, stride, rows):
    src, dst = os.path.join(BUILD, "windows_mixed_rates_kernel_in.bin"), os.path.join(BUILD, "windows_mixed_rates_kernel_out.bin")
    np.concatenate([v.reshape(-1) for v in videos]).tofile(src)
    r = subprocess.run([exe, src, str(stride), ",".join("%d/%d" % x for x in rates), dst] + [str(len(v)) for v in videos], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and "data race" not in r.stderr, r.stderr[-3000:]
    raw = open(dst, "rb").read()
    assert len(raw) == rows * 132
    return np.frombuffer(raw[:rows * 128], np.uint64).reshape(rows, 16), np.frombuffer(raw[rows * 128:], np.uint32)


def _check(exe, videos, rates, stride):
    import vid_dup_finder_lib_amd as vdf

    want, want_dc, first, rate_first = _want(videos, rates, stride)
    lib_first, lib_rate_first = vdf.hash_windows_first_rates([len(v) for v in videos], rates, stride)
    assert np.array_equal(lib_first, first) and np.array_equal(lib_rate_first, rate_first)
    assert np.all(first[:, 1:] > first[:, :-1])  # every video has a window at every rate: 31 frames are the span of 2/1
    got, dc = _run(exe, videos, rates, stride, int(rate_first[-1]))
    for r, rate in enumerate(rates):
        for i in range(len(videos)):
            for k in range(int(first[r, i + 1] - first[r, i])):
                row = int(rate_first[r] + first[r, i] + k)
                assert np.array_equal(got[row], want[row]), f"rate {rate} (block {r}) video {i} window {k} (row {row}): words differ from the oracle's"
                assert dc[row] == want_dc[row], f"rate {rate} (block {r}) video {i} window {k}: don't-care count"
    assert np.array_equal(got, want) and np.array_equal(dc, want_dc)  # the whole prefilled buffer: every row was written


def test_the_trap_case_is_the_trap():
    n2 = [retimedgen.n_windows(f, 1, (2, 1)) for f in FRAMES]
    assert n2[0] == 1 and n2[2] == 19  # F = 31: exactly one 2/1 window; F = 49: 19 of 2/1 but 34 of 1/1 - its second segment owns nothing of 2/1
    assert retimedgen.n_windows(49, 1, (1, 1)) == 34 and retimedgen.n_windows(47, 1, (2, 1)) == 17


@pytest.mark.parametrize("rates,stride", CASES)
def test_kernel_text_on_the_cpu_matches_the_oracle_and_stays_in_bounds(programs, videos, rates, stride):
    _check(programs["asan"], videos, rates, stride)


@pytest.mark.parametrize("rates,stride", CASES)
def test_every_lds_reuse_is_ordered_by_a_barrier(programs, videos, rates, stride):
    _check(programs["tsan"], videos, rates, stride)
