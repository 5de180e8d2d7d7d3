"""The zero plane of every hash route (vdf_hash_frames_u8_planes_device; csrc/dct_hash.hip: the PLANES instantiations of dct_hash_block's callers) and
vdf_hash_variants_device, against the CPU oracle.  One row per HashRoute, at the smallest frame size tests/test_gpu_hash_saturating.py's
ROUTE_CASES (checked against the planner by tests/test_hash_route_table.py) gives that route.  Per row, packed and once at an odd base address with padded strides:
  - the hashes equal the plain call's on the same input, and the oracle's;
  - Z equals the oracle's coefs == 0.0;
  - the device-derived hash of the variants equals the oracle's hash of the actually flipped frames (all seven for rows of at most 256 columns, else 1, 2, 7).
Whole words, nothing masked.  The clips: tests/framegen.py's four classes plus static (900 exact zeros), constant (999) and x-symmetric (500) - seven kinds; two
clips for the stream-class rows, whose DCT is the one dct_hash_kernel.  The two persistent kernels also get a batch of 2100 clips (the seven repeated), more than
three times the workgroups of a launch, so that every workgroup packs the planes of several clips of DIFFERENT kinds in turn through the same LDS words."""
import numpy as np
import pytest

import planegen

pytestmark = pytest.mark.gpu

# (route, h, w, env, kinds)
STREAM_KINDS = ("blocks_noise", "static")
ROWS = [
    ("kDirect16", 16, 16, {}, planegen.KINDS),
    ("kPersistentOneTile", 36, 48, {}, planegen.KINDS),
    ("kTiled", 72, 48, {}, planegen.KINDS),
    ("kPerClipFused", 96, 64, {"VDF_HASH_NO_PERSISTENT": "1"}, planegen.KINDS),
    ("kChunkStream", 270, 480, {}, STREAM_KINDS),
    ("kWaveStream", 130, 640, {}, STREAM_KINDS),
    ("kKsplit", 130, 1040, {"VDF_RESIZE_MODE": "6"}, STREAM_KINDS),
    ("kWholeLine", 131, 67, {"VDF_RESIZE_MODE": "4"}, STREAM_KINDS),
    ("kScalar", 97, 150, {"VDF_RESIZE_MODE": "1"}, STREAM_KINDS),
]
_CACHE = {}


def _engine(env, monkeypatch):
    """A fresh context under env (the knobs are read once, when the context is made)."""
    import vid_dup_finder_lib_amd as vdf

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return vdf.Engine(0)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _row(route):
    """(clips [n, 16, h, w], oracle hashes, oracle zero planes, {v: oracle hashes of the flipped clips}) - computed once, left unchanged."""
    if route not in _CACHE:
        _, h, w, _, kinds = next(r for r in ROWS if r[0] == route)
        rng = np.random.default_rng(h * 4099 + w)
        clips = np.stack([planegen.clip(k, rng, h, w) for k in kinds])
        planes = [planegen.oracle_planes(c) for c in clips]
        variants = range(1, 8) if w <= 256 else (1, 2, 7)
        flipped = {v: np.stack([planegen.oracle_variant(c, v) for c in clips]) for v in variants}
        for a in (clips, *flipped.values()):
            a.setflags(write=False)
        _CACHE[route] = (clips, np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes]), flipped, [p[2] for p in planes])
    return _CACHE[route]


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _run(eng, clips, base=0, frame_pad=0, clip_pad=0):
    """Plain call and planes call on the same device-resident clips -> (plain hashes, plain dontcare, hashes, dontcare, zero planes, device tensors of the last two)."""
    import torch

    n, _, h, w = clips.shape
    fs = w * h + frame_pad
    cs = 16 * fs + clip_pad
    host = np.full(base + n * cs, 0xAA, np.uint8)  # (the last clip's padding is part of the buffer: no load of a kernel can leave it)
    for c in range(n):
        for f in range(16):
            o = base + c * cs + f * fs
            host[o:o + w * h] = clips[c, f].reshape(-1)
    d = torch.from_numpy(host).cuda()
    outs = [torch.full((n, 16), -1, dtype=torch.int64, device="cuda") for _ in range(3)]
    dcs = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    eng.hash_frames_device(d.data_ptr() + base, n, 16, w, h, outs[0].data_ptr(), d_dontcare=dcs[0].data_ptr(), frame_stride=fs, clip_stride=cs)
    eng.hash_frames_planes_device(d.data_ptr() + base, n, 16, w, h, outs[1].data_ptr(), outs[2].data_ptr(), d_dontcare=dcs[1].data_ptr(), frame_stride=fs, clip_stride=cs)
    torch.cuda.synchronize()
    return _u64(outs[0]), dcs[0].cpu().numpy(), _u64(outs[1]), dcs[1].cpu().numpy(), _u64(outs[2]), outs[1], outs[2]


def _variants(eng, d_hashes, d_zero, n, v):
    import torch

    out = torch.full((n, 16), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.hash_variants_device(d_hashes.data_ptr(), d_zero.data_ptr(), n, v, out.data_ptr())
    torch.cuda.synchronize()
    return _u64(out)


@pytest.mark.parametrize("layout", ["packed", "odd_base_padded"])
@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_planes_and_variants_match_the_oracle_on_every_route(row, layout, monkeypatch):
    route, h, w, env, kinds = row
    clips, want_h, want_z, flipped, n_zero = _row(route)
    eng = _engine(env, monkeypatch)
    try:
        pads = dict(base=0, frame_pad=0, clip_pad=0) if layout == "packed" else dict(base=1, frame_pad=3, clip_pad=5)
        plain, plain_dc, got, dc, zero, d_h, d_z = _run(eng, clips, **pads)
        print(f"{route} {h} x {w} {layout}: exact zeros per clip {dict(zip(kinds, n_zero))}")
        assert np.array_equal(got, plain) and np.array_equal(dc, plain_dc), "the planes call's hashes / dontcare differ from the plain call's"
        assert np.array_equal(got, want_h), "hashes differ from the oracle's"
        for i, k in enumerate(kinds):
            assert np.array_equal(zero[i], want_z[i]), f"zero plane of clip {i} ({k}): {int(np.unpackbits((zero[i] ^ want_z[i]).view(np.uint8)).sum())} bits differ"
        for v, want in flipped.items():
            assert np.array_equal(_variants(eng, d_h, d_z, len(clips), v), want), f"variant {v}"
    finally:
        eng.close()


@pytest.mark.parametrize("route", ["kPersistentOneTile", "kTiled"])
def test_a_persistent_workgroup_packs_the_planes_of_many_clips_in_turn(route, monkeypatch):
    _, h, w, env, kinds = next(r for r in ROWS if r[0] == route)
    clips, want_h, want_z, _, _ = _row(route)
    reps = 300
    eng = _engine(env, monkeypatch)
    try:
        many = np.ascontiguousarray(np.tile(clips, (reps, 1, 1, 1)))
        plain, _, got, _, zero, _, _ = _run(eng, many)
        assert np.array_equal(got, plain) and np.array_equal(got, np.tile(want_h, (reps, 1)))
        bad = np.nonzero((zero != np.tile(want_z, (reps, 1))).any(axis=1))[0]
        assert len(bad) == 0, f"zero planes of clips {bad[:10]} ... differ"
    finally:
        eng.close()


def test_host_entry_python_mirror_and_refusals(monkeypatch):
    import vid_dup_finder_lib_amd as vdf

    clips, want_h, want_z, flipped, _ = _row("kPersistentOneTile")
    eng = _engine({}, monkeypatch)
    multi = None
    try:
        got, zero, dc = eng.hash_frames_planes(clips, want_dontcare=True)
        plain, plain_dc = eng.hash_frames(clips, want_dontcare=True)
        assert np.array_equal(got, plain) and np.array_equal(dc, plain_dc) and np.array_equal(got, want_h) and np.array_equal(zero, want_z)
        vhs = vdf.hash_frame_stacks(clips, [f"p{i}" for i in range(len(clips))], [10] * len(clips), engine=eng, zero_plane=True)
        assert all(np.array_equal(v.zero, want_z[i]) and np.array_equal(v.flipped(vdf.Flip.X).hash, flipped[1][i]) for i, v in enumerate(vhs))
        assert all(v.zero is None for v in vdf.hash_frame_stacks(clips, ["p"] * len(clips), [10] * len(clips), engine=eng))
        # the plain call's errors, in its order, then the plane's own
        for call, code in ((lambda: eng.hash_frames_planes(clips[:, :15]), -1), (lambda: eng.hash_frames_planes(np.zeros((1, 16, 0, 4), np.uint8)), -2)):
            with pytest.raises(vdf.VdfError) as ei:
                call()
            assert ei.value.code == code
        out = np.zeros((1, 16), np.uint64)
        flat = np.ascontiguousarray(clips[0])
        assert eng.lib.vdf_hash_frames_u8_planes(eng.ctx, flat.ctypes.data, 1, 16, 48, 36, 48 * 36, 16 * 48 * 36, out.ctypes.data, None, None) == -5
        assert eng.lib.vdf_hash_variants_device(eng.ctx, 8, 8, 1, 8, 16, None) == -5  # variant 8 (checked before anything is touched)
        multi = vdf.Engine(devices=[0, 0])
        for call in (lambda: multi.hash_frames_planes(clips), lambda: multi.hash_clips_planes(list(clips)),
                     lambda: multi.search_variants_sorted(want_h, want_z, np.full(len(want_h), 10, np.uint32), 300, 2)):
            with pytest.raises(vdf.VdfError) as ei:
                call()
            assert ei.value.code == -5
    finally:
        eng.close()
        if multi is not None:
            multi.close()
