"""The PLANES form of dct_hash_windows_kernel from its own source text on the CPU (tests/cpp/windows_planes_kernel_host_main.cpp), as
tests/test_hash_windows_kernel_host.py runs the plain form: under AddressSanitizer / UBSan every index it forms is checked - the second set of
LDS words and the zero-plane buffer among them -, under ThreadSanitizer a barrier missing between a write and a read of LDS is a data race,
and words, planes and don't-care counts must be the oracle's for every window.  That the ThreadSanitizer run can see such a race is shown:
with the pair barrier cut out of the text it reports one.  Stand-alone programs; no GPU."""
import os
import subprocess

import numpy as np
import pytest

import planegen
import windowgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build", "planes")
CSRC = os.path.join(ROOT, "vid_dup_finder_lib_amd", "csrc")
PAIR_BARRIER_BEHIND = "if (lane == 0) sh.dc[parity][half][wv] = dc;"


def _cut(lines, first, last):
    i = next(k for k, ln in enumerate(lines) if first in ln)
    j = next(k for k in range(i + 1, len(lines)) if last in lines[k])
    return lines[i:j]


def _kernel_text():
    lines = open(os.path.join(CSRC, "dct_hash.hip")).read().split("\n")
    text = _cut(lines, "struct DctTw {", "constexpr int kPadY") + [ln for ln in lines if ln.startswith("constexpr int kPadY") or ln.startswith("constexpr int kStrideT")]
    text += _cut(lines, "struct WindowsShared {", "hipError_t launch_dct_hash_windows")
    assert any("void dct_hash_windows_kernel(" in ln for ln in text) and any("windows_zero_words()" in ln for ln in text)
    return text


def _without_pair_barrier(text):
    """The text with the ONE barrier between a pair's ballots and its read-out taken out: the first __syncthreads() behind the don't-care store."""
    at = next(k for k, ln in enumerate(text) if PAIR_BARRIER_BEHIND in ln)
    k = next(k for k in range(at, len(text)) if text[k].strip() == "__syncthreads();")
    assert k - at <= 3, "the pair barrier is no longer where this test cuts it"
    return text[:k] + text[k + 1:]


def _build(tag, text, san):
    inc_dir = os.path.join(BUILD, tag)
    os.makedirs(inc_dir, exist_ok=True)
    with open(os.path.join(inc_dir, "windows_kernel.inc"), "w") as f:
        f.write("\n".join(text) + "\n")
    exe = os.path.join(inc_dir, "windows_planes_kernel_host_" + tag)
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fsanitize=" + san, "-fno-sanitize-recover=all", "-I", CSRC, "-I", inc_dir,
                           "-I", os.path.join(ROOT, "tests", "cpp"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "windows_planes_kernel_host_main.cpp")])
    return exe


@pytest.fixture(scope="module")
def programs():
    text = _kernel_text()
    return {"asan": _build("asan", text, "address,undefined"), "tsan": _build("tsan", text, "thread"),
            "tsan_no_pair_barrier": _build("tsan_no_pair_barrier", _without_pair_barrier(text), "thread")}


def _run(exe, videos, stride, frame_pad=0, clip_pad=0, expect_race=False):
    n, nf = videos.shape[:2]
    fs = 256 + frame_pad
    cs = nf * fs + clip_pad
    buf = np.full(n * cs, 0xAA, np.uint8)
    for c in range(n):
        for f in range(nf):
            buf[c * cs + f * fs:c * cs + f * fs + 256] = videos[c, f].reshape(-1)
    src, dst = os.path.join(os.path.dirname(exe), "in.bin"), os.path.join(os.path.dirname(exe), "out.bin")
    buf.tofile(src)
    dwords = int(frame_pad % 4 == 0 and clip_pad % 4 == 0)
    r = subprocess.run([exe, src, str(n), str(nf), str(stride), str(fs), str(cs), str(dwords), dst], capture_output=True, text=True, timeout=300)
    if expect_race:
        return r
    assert r.returncode == 0 and "data race" not in r.stderr, r.stderr[-3000:]
    n_win = windowgen.n_windows(nf, stride)
    raw = open(dst, "rb").read()
    nb = n * n_win * 128
    return (np.frombuffer(raw[:nb], np.uint64).reshape(n, n_win, 16), np.frombuffer(raw[nb:2 * nb], np.uint64).reshape(n, n_win, 16),
            np.frombuffer(raw[2 * nb:], np.uint32).reshape(n, n_win))


def _videos(n, nf, stride):
    rng = np.random.default_rng(nf * 131 + stride)
    return np.stack([windowgen.video(rng, nf, 16, 16, lead=(0, 5, 3)[c % 3]) for c in range(n)])


def _check(exe, n, nf, stride, **pads):
    from oracle import vdf_oracle as orc

    videos = _videos(n, nf, stride)
    got, zero, dc = _run(exe, videos, stride, **pads)
    kinds = set()
    for c in range(n):
        for k in range(got.shape[1]):
            frames = np.ascontiguousarray(videos[c, k * stride:k * stride + 16])
            words, plane, n_zero = planegen.oracle_planes(frames)
            _, _, coefs = orc.hash_clip(frames, want_coefs=True)
            assert np.array_equal(got[c, k], words), f"clip {c} window {k}: words differ from the oracle's"
            assert np.array_equal(zero[c, k], plane), f"clip {c} window {k}: zero plane differs from the oracle's coefs == 0.0"
            assert not np.any(got[c, k] & zero[c, k]) and int(zero[c, k, 15]) >> 40 == 0
            assert dc[c, k] == int((np.abs(coefs) < 1e-6).sum()), f"clip {c} window {k}: don't-care count"
            kinds.add(n_zero)
    return kinds


# the plain harness's geometries
@pytest.mark.parametrize("n_frames,stride", [(16, 1), (33, 1), (48, 3), (40, 7), (50, 16), (60, 17), (65, 1)])
def test_planes_kernel_text_on_the_cpu_matches_the_oracle_and_stays_in_bounds(programs, n_frames, stride):
    kinds = _check(programs["asan"], 1, n_frames, stride)
    # lead 0: 17 static frames, 16 constant ones, then noise - windows 0 and 1 are static (900 exact zeros), window 17 is constant (999), the
    # windows between straddle, and from frame 33 on there is noise (none)
    if (n_frames, stride) == (33, 1):
        assert {900, 999} <= kinds and len(kinds) > 2, kinds
    if (n_frames, stride) == (65, 1):
        assert {900, 999, 0} <= kinds, kinds


def test_two_clips_at_padded_strides_read_by_bytes(programs):
    _check(programs["asan"], 2, 35, 5, frame_pad=3, clip_pad=5)


@pytest.mark.parametrize("n,n_frames,stride", [(1, 40, 1), (2, 36, 3), (1, 60, 17)])
def test_every_lds_reuse_is_ordered_by_a_barrier(programs, n, n_frames, stride):
    _check(programs["tsan"], n, n_frames, stride)


def test_without_the_pair_barrier_the_race_is_reported(programs):
    r = _run(programs["tsan_no_pair_barrier"], _videos(1, 40, 1), 1, expect_race=True)
    assert "data race" in r.stderr and r.returncode != 0, (r.returncode, r.stderr[-2000:])
