"""Flipped and reversed stretches on the GPU: vdf_window_variants_device (csrc/dct_hash.hip: window_variants_kernel) against
its host twin, vdf_align_windows_variants[_device] against the host form record for record on the problems of tests/test_align_variants_host.py
and on 20 random ones, and the whole chain end to end: hash_frame_windows(zero_plane=True) -> align_flipped finds a stretch that is mirrored,
reversed and trimmed, which align does not see."""
import numpy as np
import pytest

import variantgen as vg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import vid_dup_finder_lib_amd as vdf

    e = vdf.Engine(0)
    yield e
    e.close()


def _dev(x, dtype):
    import torch

    return None if x is None else torch.from_numpy(np.ascontiguousarray(x).view(dtype).copy()).cuda()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def test_window_variants_kernel_equals_the_host_twin(eng):
    import torch

    import vid_dup_finder_lib_amd as vdf

    rng = np.random.default_rng(7)
    counts = [0, 5, 0, 0, 1, 70, 2, 0, 33, 0]  # empty videos in front, in a run, at the end; a one-window video; more rows than a workgroup's 16
    first = np.zeros(len(counts) + 1, np.uint32)
    first[1:] = np.cumsum(counts)
    n = int(first[-1])
    h = rng.integers(0, 2**64, size=(n, 16), dtype=np.uint64)
    z = vg.random_planes(rng, h, 0.3)
    skip = rng.integers(0, 256, size=n).astype(np.uint8)
    dh, dz, df, dk = _dev(h, np.int64), _dev(z, np.int64), _dev(first, np.int32), _dev(skip, np.uint8)
    guard = 64
    for v in vg.ALL_VARIANTS:
        for lo in (0, 4):  # the whole set, and a set that begins behind row 0 (videos 4 ...): rows in front of it stay untouched
            out = torch.full((n + guard, 16), -1, dtype=torch.int64, device="cuda")
            out_k = torch.full((n + guard,), 255, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            eng.window_variants(dh.data_ptr(), dz.data_ptr(), df.data_ptr() + 4 * lo, len(counts) - lo, v, out.data_ptr(), dk.data_ptr(), out_k.data_ptr())
            torch.cuda.synchronize()
            want, want_k = vdf.window_variants_host(h, z, first[lo:], v, skip)
            r0 = int(first[lo])
            got, got_k = out.cpu().numpy().view(np.uint64), out_k.cpu().numpy()
            assert np.array_equal(got[r0:n], want[r0:]) and np.array_equal(got_k[r0:n], want_k[r0:]), (v, lo)
            ones = np.uint64(2**64 - 1)
            assert (got[:r0] == ones).all() and (got[n:] == ones).all() and (got_k[:r0] == 255).all() and (got_k[n:] == 255).all(), (v, lo)
    # without skip bytes, and the argument checks: nothing of out is written by a refused call
    out = torch.full((n, 16), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.window_variants(dh.data_ptr(), dz.data_ptr(), df.data_ptr(), len(counts), 6, out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), vdf.window_variants_host(h, z, first, 6))
    call = eng.lib.vdf_window_variants_device
    for args in ((dh.data_ptr(), dz.data_ptr(), df.data_ptr(), 10, None, 0, out.data_ptr(), None, None),       # variant outside 1 ... 7
                 (dh.data_ptr(), dz.data_ptr(), df.data_ptr(), 10, None, 8, out.data_ptr(), None, None),
                 (None, dz.data_ptr(), df.data_ptr(), 10, None, 1, out.data_ptr(), None, None),                 # null pointers
                 (dh.data_ptr(), dz.data_ptr(), df.data_ptr(), 10, dk.data_ptr(), 1, out.data_ptr(), None, None),
                 (dh.data_ptr(), dz.data_ptr(), df.data_ptr(), 10, None, 1, dh.data_ptr(), None, None)):        # in place
        assert call(eng.ctx, *args) == -5
    assert call(eng.ctx, None, None, None, 0, None, 3, None, None, None) == 0
    dec = _dev(np.array([0, 5, 3], np.uint32), np.int32)
    assert call(eng.ctx, dh.data_ptr(), dz.data_ptr(), dec.data_ptr(), 2, None, 1, out.data_ptr(), None, None) == -5
    assert "decreases" in eng.lib.vdf_last_error(eng.ctx).decode()
    multi = vdf.Engine(devices=[0, 0])
    try:
        assert call(multi.ctx, dh.data_ptr(), dz.data_ptr(), df.data_ptr(), 10, None, 1, out.data_ptr(), None, None) == -5
        assert "single-device" in multi.lib.vdf_last_error(multi.ctx).decode()
    finally:
        multi.close()


def device_form(eng, vp, capacity=4096):
    import torch

    p = vp.p
    ah, az, af, ak = _dev(p.a_hashes, np.int64), _dev(vp.a_zero, np.int64), _dev(p.a_first, np.int32), _dev(p.a_skip, np.uint8)
    bh, bz, bf, bk = _dev(p.b_hashes, np.int64), _dev(vp.b_zero, np.int64), _dev(p.b_first, np.int32), _dev(p.b_skip, np.uint8)
    torch.cuda.synchronize()
    rec, found = eng.align_windows_variants_device(_ptr(ah), _ptr(af), len(p.a_first) - 1, _ptr(az), _ptr(bh), _ptr(bf), 0 if bf is None else len(p.b_first) - 1,
                                                   _ptr(bz), tol_int=p.tol, min_run=p.min_run, variant_mask=vp.mask, d_a_skip=_ptr(ak), d_b_skip=_ptr(bk),
                                                   capacity=capacity)
    return vg.records(rec), found


def host_array_form(eng, vp, capacity=4096):
    rec, found = eng.align_windows_variants(capacity=capacity, **vg.call_args(vp))
    return vg.records(rec), found


def host_form(vp, capacity=4096):
    import vid_dup_finder_lib_amd as vdf

    rec, found = vdf.align_windows_variants_host(capacity=capacity, **vg.call_args(vp))
    return vg.records(rec), found


@pytest.mark.parametrize("name", sorted(vg.CASES))
def test_device_forms_equal_the_host_form(eng, name):
    vp = vg.case(name)
    want = host_form(vp)
    assert want == (list(vg.expected(name)), len(vg.expected(name)))
    assert device_form(eng, vp) == want
    assert host_array_form(eng, vp) == want


def test_twenty_random_problems(eng):
    rng = np.random.default_rng(2024)
    for i in range(20):
        vp = vg.random_problem(rng)
        want = host_form(vp)
        assert device_form(eng, vp) == want, i
        assert host_array_form(eng, vp) == want, i


def test_capacity_smaller_than_the_result(eng):
    vp = vg.case("all_variants_order")
    vp = vp._replace(p=vp.p._replace(tol=1024))  # every cell matches: a record per (variant, pair), 7 x 4
    want, found = host_form(vp)
    assert found == 28
    for form in (device_form, host_array_form):
        for cap in (0, 3, 4, 5, 27, 28):
            got, n = form(eng, vp, capacity=cap)
            assert n == found and got == want[:cap], (form.__name__, cap)


def test_argument_checks_in_their_order(eng):
    import ctypes as C

    import vid_dup_finder_lib_amd as vdf

    vp = vg.case("mirrored")
    p = vp.p
    ah, af, bh, bz, bf = _dev(p.a_hashes, np.int64), _dev(p.a_first, np.int32), _dev(p.b_hashes, np.int64), _dev(vp.b_zero, np.int64), _dev(p.b_first, np.int32)
    out = np.zeros(8, vdf.ALIGN_VARIANT_DTYPE)
    n = C.c_size_t(0)
    call = eng.lib.vdf_align_windows_variants_device

    def dev(ctx=None, ah=ah, az=None, af=af, bh=bh, bz=bz, bf=bf, min_run=1, mask=2, out=out):
        return call(ctx or eng.ctx, _ptr(ah), _ptr(az), _ptr(af), 2, None, _ptr(bh), _ptr(bz), _ptr(bf), 2, None, 350, min_run, mask,
                    out.ctypes.data if out is not None else None, 8, C.byref(n), None), eng.lib.vdf_last_error(ctx or eng.ctx).decode()
    assert dev()[0] == 0 and n.value == 1
    rc, msg = dev(af=None, min_run=0, mask=1, bz=None)
    assert rc == -5 and "null" in msg
    rc, msg = dev(min_run=0, mask=1, bz=None)
    assert rc == -5 and "min_run" in msg
    dec = _dev(np.array([0, 40, 30], np.uint32), np.int32)
    rc, msg = dev(af=dec, mask=1, bz=None)
    assert rc == -5 and "decreases" in msg
    rc, msg = dev(mask=1, bz=None)
    assert rc == -5 and "variant_mask" in msg
    rc, msg = dev(mask=0x100)
    assert rc == -5 and "variant_mask" in msg
    rc, msg = dev(bz=None)
    assert rc == -5 and "zero plane" in msg
    rc, msg = dev(bh=None, bf=None, bz=None)  # self mode without A's planes
    assert rc == -5 and "zero plane" in msg
    multi = vdf.Engine(devices=[0, 0])
    try:
        rc, msg = dev(ctx=multi.ctx, bz=None)
        assert rc == -5 and "zero plane" in msg
        rc, msg = dev(ctx=multi.ctx)
        assert rc == -5 and "single-device" in msg
        with pytest.raises(vdf.VdfError) as ei:
            multi.align_windows_variants(**vg.call_args(vp))
        assert ei.value.code == -5 and "single-device" in str(ei.value)
    finally:
        multi.close()


def test_end_to_end_a_mirrored_reversed_and_trimmed_stretch(eng):
    import vid_dup_finder_lib_amd as vdf
    from vid_dup_finder_lib_amd import Flip

    rng = np.random.default_rng(41)
    a = rng.integers(0, 256, size=(80, 32, 32), dtype=np.uint8)
    noise = lambda n: rng.integers(0, 256, size=(n, 32, 32), dtype=np.uint8)
    # b: 3 frames of its own, frames 10 ... 49 of a mirrored and played backwards, 5 frames of its own - 48 frames
    b = np.ascontiguousarray(np.concatenate([noise(3), a[10:50][::-1, :, ::-1], noise(5)]))
    c = noise(64)
    windows = [vdf.hash_frame_windows(v[None], [name], [len(v)], stride=1, engine=eng, zero_plane=True)[0] for v, name in ((a, "a.mp4"), (b, "b.mp4"), (c, "c.mp4"))]
    assert [len(w) for w in windows] == [65, 33, 49] and all(h.zero is not None for w in windows for h in w)
    # tolerance 0: exactly the windows that lie inside the planted frames match - frames 10 ... 49 of a are frames 3 ... 42 of b, mirrored, b's
    # playing backwards: 25 windows, every one at distance 0
    got = vdf.align_flipped(windows, tolerance=0.0, min_run=4, flips=[Flip.X, Flip.X | Flip.T], engine=eng)
    assert got[Flip.X] == [] and len(got[Flip.X | Flip.T]) == 1
    g = got[Flip.X | Flip.T][0]
    assert (g.a, g.b, g.first_frame_a, g.first_frame_b, g.n_frames, g.n_windows, g.mean_distance, g.offset_frames) == (0, 1, 10, 3, 40, 25, 0.0, -7)
    assert (g.path_a, g.path_b, g.flip) == ("a.mp4", "b.mp4", Flip.X | Flip.T)
    assert np.array_equal(a[g.first_frame_a:g.first_frame_a + g.n_frames], b[g.first_frame_b:g.first_frame_b + g.n_frames][::-1, :, ::-1])
    # the default tolerance: still one record, on the same diagonal; windows that hold a few frames from outside the stretch are within it too,
    # so the run is longer on both sides - and align, which sees only unflipped stretches, reports nothing
    got = vdf.align_flipped(windows, tolerance=vdf.DEFAULT_SEARCH_TOLERANCE, min_run=4, flips=[Flip.X, Flip.X | Flip.T], engine=eng)
    assert got[Flip.X] == [] and len(got[Flip.X | Flip.T]) == 1
    g = got[Flip.X | Flip.T][0]
    assert (g.a, g.b) == (0, 1) and g.first_frame_a <= 10 and g.first_frame_a + g.n_frames >= 50 and g.first_frame_a + g.first_frame_b + g.n_frames == 10 + 3 + 40
    assert vdf.align(windows, tolerance=vdf.DEFAULT_SEARCH_TOLERANCE, min_run=4, engine=eng) == []
    # two sets: the same stretch with b as the flipped side; hashes without planes on that side are refused
    two = vdf.align_flipped([windows[0]], [windows[2], windows[1]], tolerance=0.0, min_run=4, flips=[Flip.X | Flip.T], engine=eng)[Flip.X | Flip.T]
    assert [(t.a, t.b, t.first_frame_a, t.first_frame_b, t.n_frames) for t in two] == [(0, 1, 10, 3, 40)]
    plain = vdf.hash_frame_windows(b[None], ["b.mp4"], [48], stride=1, engine=eng)
    with pytest.raises(vdf.VidProc):
        vdf.align_flipped([windows[0]], plain, flips=[Flip.X], engine=eng)
