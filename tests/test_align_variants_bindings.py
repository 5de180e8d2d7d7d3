"""The mirrors of the flipped-stretch calls without a GPU: the ctypes signatures against the header, host/vdf.hpp's
VideoHash::align_windows_variants compiled with g++ against libvdf_hip.so and run on the CPU (tests/cpp/align_variants_mirror_main.cpp), and
align_flipped's frame arithmetic on hand-made hashes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import planegen

import vid_dup_finder_lib_amd as vdf
from vid_dup_finder_lib_amd import Flip, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vdf_hash_windows_u8_planes", "vdf_hash_windows_u8_planes_device", "vdf_window_variants_host", "vdf_window_variants_device",
       "vdf_align_windows_variants_host", "vdf_align_windows_variants", "vdf_align_windows_variants_device")


def test_ctypes_signatures_have_the_headers_arity_and_the_record_its_size():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vdf.h")).read(), flags=re.S)
    lib = _capi.load()
    for name in NEW:
        args = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S).group(1)
        restype, argtypes = _capi.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(args.split(",")), name
        assert getattr(lib, name).argtypes == argtypes
    # plain forms + the zero plane in front of the stream / at the end; the align forms + two planes and the mask
    assert len(_capi.SIGNATURES["vdf_hash_windows_u8_planes"][1]) == len(_capi.SIGNATURES["vdf_hash_windows_u8"][1]) + 1
    assert len(_capi.SIGNATURES["vdf_align_windows_variants_device"][1]) == len(_capi.SIGNATURES["vdf_align_windows_device"][1]) + 3
    assert C.sizeof(_capi.VdfAlignmentVariant) == 28 == vdf.ALIGN_VARIANT_DTYPE.itemsize
    assert vdf.ALIGN_VARIANT_DTYPE.names == tuple(f for f, _ in _capi.VdfAlignmentVariant._fields_)
    assert all(vdf.ALIGN_VARIANT_DTYPE.fields[f][1] == getattr(_capi.VdfAlignmentVariant, f).offset for f in vdf.ALIGN_VARIANT_DTYPE.names)


def test_cpp_mirror_aligns_flipped_stretches_on_the_cpu():
    lib = os.path.join(ROOT, "vid_dup_finder_lib_amd")
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "align_variants_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(lib, "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "align_variants_mirror_main.cpp"), "-L" + lib, "-lvdf_hip", "-Wl,-rpath," + lib,
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "align variants mirror ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def _hand_made(rng, n, path):
    """n window hashes with sparse zero planes (H & Z == 0)"""
    out = []
    for _ in range(n):
        z = planegen.pack_bits((rng.random(1000) < 0.1).astype(np.uint8))
        h = planegen.pack_bits(rng.integers(0, 2, size=1000).astype(np.uint8)) & ~z
        out.append(vdf.VideoHash(h, path, n, z))
    return out


@pytest.mark.parametrize("stride", [1, 3])
def test_align_flipped_frame_arithmetic(stride):
    rng = np.random.default_rng(9)
    b = _hand_made(rng, 20, "b")      # Nb = 20 windows
    c = _hand_made(rng, 7, "c")
    a = _hand_made(rng, 30, "a")
    # a's windows 8 ... 17 = b's windows 16 ... 7 (backwards), mirrored and reversed: derived rows 3 ... 12 of the X | T set of b
    for i in range(10):
        src = b[19 - (3 + i)]
        a[8 + i] = vdf.VideoHash(vdf.engine.hash_variant(src.hash, src.zero, 5), "a", 30, a[8 + i].zero)
    # and a's windows 20 ... 25 = c's windows 1 ... 6 mirrored only
    for i in range(6):
        a[20 + i] = vdf.VideoHash(vdf.engine.hash_variant(c[1 + i].hash, c[1 + i].zero, 1), "a", 30, a[20 + i].zero)
    got = vdf.align_flipped([a], [b, c, []], tolerance=0.35, min_run=2, stride=stride, flips=[Flip.X, Flip.Y, Flip.X | Flip.T])
    assert set(got) == {Flip.X, Flip.Y, Flip.X | Flip.T} and got[Flip.Y] == []
    (t,) = got[Flip.X | Flip.T]
    # C ABI record: offset = 3 - 8, start_a = 8, n_windows = 10 -> first window of b in its own order: Nb - 1 - (start_a + offset + n_windows - 1) = 7
    assert (t.a, t.b, t.n_windows, t.mean_distance, t.flip, t.path_a, t.path_b) == (0, 0, 10, 0.0, Flip.X | Flip.T, "a", "b")
    assert t.first_frame_a == 8 * stride and t.first_frame_b == (20 - 1 - (8 - 5 + 10 - 1)) * stride == 7 * stride
    assert t.n_frames == 9 * stride + 16 and t.offset_frames == t.first_frame_b - t.first_frame_a
    (x,) = got[Flip.X]
    assert (x.a, x.b, x.first_frame_a, x.first_frame_b, x.n_frames, x.n_windows, x.mean_distance, x.flip) == (0, 1, 20 * stride, 1 * stride, 5 * stride + 16, 6, 0.0, Flip.X)
    assert isinstance(t, vdf.FlippedAlignment) and not isinstance(t, vdf.Alignment) and len(t) == len(vdf.Alignment._fields) + 1
    # self mode: the pairs a < b, the flipped side is windows_a itself
    self_mode = vdf.align_flipped([a, b, c], tolerance=0.35, min_run=2, stride=stride, flips=[Flip.X | Flip.T, Flip.X])
    assert [(r.a, r.b, r.first_frame_b) for r in self_mode[Flip.X | Flip.T]] == [(0, 1, 7 * stride)]
    assert [(r.a, r.b, r.first_frame_b) for r in self_mode[Flip.X]] == [(0, 2, stride)]
    # align sees neither; a flipped side without planes is refused; flips outside 1 ... 7 are refused
    assert vdf.align([a], [b, c], tolerance=0.35, min_run=2, stride=stride) == []
    with pytest.raises(vdf.VidProc):
        vdf.align_flipped([a], [[vdf.VideoHash(h.hash, "b", 1) for h in b]], flips=[Flip.X])
    with pytest.raises(ValueError):
        vdf.align_flipped([a], [b], flips=[0])
    assert vdf.align_flipped([a], [b], flips=[]) == {}
