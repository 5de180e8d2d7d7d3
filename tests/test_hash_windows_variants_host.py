"""The identity DESIGN.md 4.11 rests on, on the CPU with the oracle alone: with H[k], Z[k] the oracle's hash and `coefs == 0.0` plane of
window k of a video, vdf_window_variants_host on (H, Z) gives the oracle's window hashes of the actually flipped video, word for word -
in the same order without Flip.T, in reversed order with it; and where (F - 16) % stride != 0, the Flip.T rows are those of the reversed
video with its first (F - 16) % stride frames dropped, NOT those of the reversed video."""
import numpy as np
import pytest

import variantgen as vg
import windowgen

import vid_dup_finder_lib_amd as vdf


def _video_and_planes(F, stride, h, w):
    rng = np.random.default_rng([F, stride, h, w])
    video = windowgen.video(rng, F, h, w, lead=3)
    H, Z, zeros = vg.oracle_windows_planes(video, stride)
    return video, H, Z, zeros


@pytest.mark.parametrize("F,stride,h,w", [(41, 5, 16, 16), (33, 1, 24, 40), (40, 3, 16, 16)])
def test_variant_rows_are_the_window_hashes_of_the_flipped_video(F, stride, h, w):
    video, H, Z, zeros = _video_and_planes(F, stride, h, w)
    assert (F - 16) % stride == 0
    assert 100 in zeros and 0 in zeros, zeros  # a window that straddles into a static stretch, and noise; the static ones: the test below
    assert not np.any(H & Z)
    first = np.array([0, len(H)], np.uint32)
    for v in vg.ALL_VARIANTS:
        want, _ = windowgen.oracle_windows(vg.flip_video(video, v), stride)
        got = vdf.window_variants_host(H, Z, first, v)
        assert np.array_equal(got, want), f"variant {v}"
        assert np.array_equal(got, vg.variant_twin(H, Z, first, v))


def test_the_sets_hold_static_straddling_and_noisy_windows():
    """Windows with 900 exact zeros (inside the static stretch), with 100 (straddling) and with none are all in the sets above."""
    assert _video_and_planes(33, 1, 24, 40)[3].count(900) == 2 and _video_and_planes(40, 3, 16, 16)[3].count(900) == 1
    assert _video_and_planes(41, 5, 16, 16)[3] == [0, 0, 100, 0, 999, 0]
    for geometry in ((41, 5, 16, 16), (33, 1, 24, 40), (40, 3, 16, 16)):
        zeros = _video_and_planes(*geometry)[3]
        assert 100 in zeros and 0 in zeros, zeros


def test_reversed_rows_off_the_window_grid_are_those_of_the_trimmed_reversed_video():
    F, stride = 43, 5
    video, H, Z, _ = _video_and_planes(F, stride, 16, 16)
    assert (F - 16) % stride == 2
    first = np.array([0, len(H)], np.uint32)
    for v in vg.ALL_VARIANTS:
        got = vdf.window_variants_host(H, Z, first, v)
        if not v & 4:
            assert np.array_equal(got, windowgen.oracle_windows(vg.flip_video(video, v), stride)[0]), f"variant {v}"
            continue
        flipped = vg.flip_video(video, v)  # reversed (and mirrored / flipped)
        assert np.array_equal(got, windowgen.oracle_windows(flipped[2:], stride)[0]), f"variant {v}: the reversed video less its first 2 frames"
        assert not np.array_equal(got, windowgen.oracle_windows(flipped, stride)[0]), f"variant {v}: NOT the reversed video's own windows"


def test_sets_of_several_videos_with_empty_and_one_window_videos_and_skip_bytes():
    rng = np.random.default_rng(5)
    vids = [windowgen.video(rng, F, 16, 16, lead=3) for F in (40, 16, 31)]
    parts = [vg.oracle_windows_planes(v, 3)[:2] for v in vids]
    H = np.concatenate([p[0] for p in parts])
    Z = np.concatenate([p[1] for p in parts])
    counts = [len(parts[0][0]), 0, len(parts[1][0]), 0, 0, len(parts[2][0])]
    assert counts[2] == 1
    first = np.zeros(len(counts) + 1, np.uint32)
    first[1:] = np.cumsum(counts)
    skip = rng.integers(0, 256, size=len(H)).astype(np.uint8)
    for v in vg.ALL_VARIANTS:
        got, got_skip = vdf.window_variants_host(H, Z, first, v, skip)
        want = np.concatenate([windowgen.oracle_windows(vg.flip_video(x, v), 3)[0] for x in vids])
        assert np.array_equal(got, want), f"variant {v}"
        want_twin, want_skip = vg.variant_twin(H, Z, first, v, skip)
        assert np.array_equal(got, want_twin) and np.array_equal(got_skip, want_skip)
    # a set that begins behind row 0: rows in front of first[0] are neither read nor written
    got = vdf.window_variants_host(H, Z, first[2:], 5)
    assert not got[:first[2]].any() and np.array_equal(got[first[2]:], vg.variant_twin(H, Z, first, 5)[first[2]:])


def test_window_variants_host_errors_in_their_order():
    import ctypes as C

    from vid_dup_finder_lib_amd import _capi

    lib = _capi.load()
    h = np.zeros((4, 16), np.uint64)
    z = np.zeros((4, 16), np.uint64)
    out = np.zeros((4, 16), np.uint64)
    k = np.zeros(4, np.uint8)
    ok = np.zeros(4, np.uint8)
    f = np.array([0, 3, 4], np.uint32)
    bad = np.array([0, 3, 2], np.uint32)
    E = _capi.VDF_E_INVAL
    call = lib.vdf_window_variants_host
    p = lambda a: a.ctypes.data
    assert call(None, None, None, 2, None, 0, None, None) == E and call(p(h), p(z), p(f), 2, None, 8, p(out), None) == E   # the variant first
    assert call(None, None, None, 0, None, 3, None, None) == _capi.VDF_OK                                                # no videos: nothing is read
    for args in ((None, p(z), p(f), 2, None, 3, p(out), None), (p(h), None, p(f), 2, None, 3, p(out), None), (p(h), p(z), None, 2, None, 3, p(out), None),
                 (p(h), p(z), p(f), 2, None, 3, None, None), (p(h), p(z), p(f), 2, p(k), 3, p(out), None), (p(h), p(z), p(f), 2, None, 3, p(out), p(ok))):
        assert call(*args) == E
    assert call(p(h), p(z), p(bad), 2, None, 3, p(h), None) == E     # in place: reported before the first array is looked at
    assert call(p(h), p(z), p(f), 2, None, 3, p(z), None) == E and call(p(h), p(z), p(f), 2, p(k), 3, p(out), p(k)) == E
    assert call(p(h), p(z), p(bad), 2, None, 3, p(out), None) == E
    assert call(p(h), p(z), p(f), 2, p(k), 3, p(out), p(ok)) == _capi.VDF_OK
    with pytest.raises(vdf.VdfError):
        vdf.window_variants_host(h, z, bad, 3)
    with pytest.raises(ValueError):
        vdf.window_variants_host(h, z, np.array([0, 5], np.uint32), 3)
