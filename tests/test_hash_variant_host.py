"""vdf_hash_variant (host only, no context; include/vdf.h) against the CPU oracle: with H and Z taken from oracle.hash_clip(..., want_coefs=True),
the derived hash of every variant v = 1 ... 7 must equal - every word - the oracle's hash of the actually flipped frames.  Sizes and contents are the issue's:
clips with 0, 360, 500, 900 and 999 exact zero coefficients are among them, which is what the zero plane is for."""
import ctypes as C

import numpy as np
import pytest

import planegen
from oracle import vdf_oracle as orc

SIZES = [(16, 16), (64, 64), (34, 48), (96, 160), (128, 18)]  # h x w


def _lib():
    from vid_dup_finder_lib_amd import _capi

    return _capi.load()


def _variant(h, z, v):
    out = np.zeros(16, np.uint64)
    rc = _lib().vdf_hash_variant(h.ctypes.data, z.ctypes.data, v, out.ctypes.data)
    return rc, out


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_every_variant_of_every_content_equals_the_oracle_hash_of_the_flipped_frames(size):
    h, w = size
    rng = np.random.default_rng(h * 1000 + w)
    zeros = {}
    for kind in planegen.HOST_KINDS:
        frames = planegen.clip(kind, rng, h, w)
        words, zero, nz = planegen.oracle_planes(frames)
        zeros[kind] = nz
        assert not (words & zero).any(), (kind, "H & Z != 0")
        bits = np.unpackbits(zero.view(np.uint8), bitorder="little")
        assert not bits[1000:].any(), (kind, "zero plane bits 1000 ... 1023")
        rc, same = _variant(words, zero, 0)
        assert rc == 0 and np.array_equal(same, words), (kind, "variant 0 is the identity")
        for v in range(1, 8):
            rc, got = _variant(words, zero, v)
            want = planegen.oracle_variant(frames, v)
            assert rc == 0 and np.array_equal(got, want), (kind, v, int(np.unpackbits((got ^ want).view(np.uint8)).sum()), "bits differ")
            assert np.array_equal(got, (words ^ planegen.variant_mask(v)) & ~zero), (kind, v, "the formula")
            assert not np.unpackbits(got.view(np.uint8), bitorder="little")[1000:].any(), (kind, v, "padding bits")
    print(f"{h} x {w}: exact zeros {zeros}")
    assert zeros["static"] == 900 and zeros["constant"] == 999 and zeros["x_symmetric"] >= 500 and zeros["t_symmetric"] >= 500, zeros


def test_a_variant_above_7_and_null_pointers_are_refused():
    from vid_dup_finder_lib_amd import _capi

    h, z = np.zeros(16, np.uint64), np.zeros(16, np.uint64)
    assert _variant(h, z, 8)[0] == _capi.VDF_E_INVAL and _variant(h, z, 0xFFFFFFFF)[0] == _capi.VDF_E_INVAL
    out = np.zeros(16, np.uint64)
    lib = _lib()
    assert lib.vdf_hash_variant(None, z.ctypes.data, 1, out.ctypes.data) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_variant(h.ctypes.data, None, 1, out.ctypes.data) == _capi.VDF_E_INVAL
    assert lib.vdf_hash_variant(h.ctypes.data, z.ctypes.data, 1, None) == _capi.VDF_E_INVAL


def test_the_masks_have_125_bits_per_parity_class_and_compose():
    """M_a ^ M_b == M_(a ^ b) (flipping twice), and the 8 sign patterns split the 1000 bits into 8 classes of exactly 125."""
    zero = np.zeros(16, np.uint64)
    m = [_variant(zero, zero, v)[1] for v in range(8)]
    for a in range(8):
        assert np.array_equal(m[a], planegen.variant_mask(a))
        for b in range(8):
            assert np.array_equal(m[a] ^ m[b], m[a ^ b])
    bits = np.stack([np.unpackbits(x.view(np.uint8), bitorder="little")[:1000] for x in (m[1], m[2], m[4])])
    cls, counts = np.unique(bits[0] + 2 * bits[1] + 4 * bits[2], return_counts=True)
    assert list(cls) == list(range(8)) and (counts == 125).all()


def test_python_mirror_flipped_needs_a_plane_and_matches():
    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(7)
    frames = planegen.clip("static", rng, 34, 48)
    words, zero, _ = planegen.oracle_planes(frames)
    with pytest.raises(vdf.VidProc):
        vdf.VideoHash(words, "a", 3).flipped(vdf.Flip.X)
    vh = vdf.VideoHash(words, "a", 3, zero=zero)
    assert vdf.VideoHash(words, "a", 3).zero is None and vh == vdf.VideoHash(words, "a", 3)  # the plane takes no part in comparisons
    for flip in (vdf.Flip.X, vdf.Flip.Y, vdf.Flip.T, vdf.Flip.X | vdf.Flip.Y, vdf.Flip.X | vdf.Flip.Y | vdf.Flip.T):
        f = vh.flipped(flip)
        assert np.array_equal(f.hash, planegen.oracle_variant(frames, int(flip))) and f.src_path() == "a" and f.duration() == 3
        assert np.array_equal(f.flipped(flip).hash, vh.hash)  # a flip is its own inverse
    assert vh.with_duration(5).zero is not None and vh.with_src_path("b").zero is not None
    with pytest.raises(vdf.VidProc):
        vdf.search_flipped([vdf.VideoHash(words, "a", 3)], 0.3)


def test_the_new_calls_refuse_a_null_context_and_bad_arguments_without_a_gpu():
    from vid_dup_finder_lib_amd import _capi

    lib = _lib()
    buf = np.zeros(16 * 16 * 16, np.uint8)
    out, zero = np.zeros(16, np.uint64), np.zeros(16, np.uint64)
    groups = (_capi.VdfGroups * 8)()
    inval = _capi.VDF_E_INVAL
    assert lib.vdf_hash_frames_u8_planes(None, buf.ctypes.data, 1, 16, 16, 16, 256, 4096, out.ctypes.data, None, zero.ctypes.data) == inval
    assert lib.vdf_hash_frames_u8_planes_device(None, buf.ctypes.data, 1, 16, 16, 16, 256, 4096, out.ctypes.data, None, zero.ctypes.data, None) == inval
    assert lib.vdf_hash_clips_u8_planes(None, buf.ctypes.data, buf.size, None, 0, 16, out.ctypes.data, None, zero.ctypes.data) == inval
    assert lib.vdf_hash_clips_u8_planes_device(None, buf.ctypes.data, buf.size, None, 0, 16, out.ctypes.data, None, zero.ctypes.data, None) == inval
    assert lib.vdf_hash_variants_device(None, out.ctypes.data, zero.ctypes.data, 1, 1, out.ctypes.data, None) == inval
    dur = np.zeros(1, np.uint32)
    assert lib.vdf_search_variants(None, out.ctypes.data, zero.ctypes.data, dur.ctypes.data, 1, 350, 2, groups) == inval
    assert lib.vdf_search_variants_device(None, out.ctypes.data, zero.ctypes.data, dur.ctypes.data, 1, 350, 2, groups, None) == inval
    assert lib.vdf_search_variants(None, out.ctypes.data, zero.ctypes.data, dur.ctypes.data, 1, 350, 2, None) == inval
