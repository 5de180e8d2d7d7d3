"""Hash parity on frames that SATURATE the resize, on every kernel route.

The other hash tests fill their frames with iid noise, which from 64 x 64 up all but never reaches the clip8() that ends both resize passes, never
feeds the second pass an operand far from 128 and never moves a thumbnail pixel off mid-grey (tests/framegen.py has the numbers).  Here
every kernel family hashes the content corpus of framegen.py - hard-edged blocks, sparse white on black and its inverse, full-range ramps,
interleaved in one batch - and must give the oracle's 1000 bits and don't-care count.  tests/test_hash_content_corpus.py shows on the CPU
that a resize without either clamp, or without the re-centring of its second pass, changes at least 100 bits of every such clip;
tests/test_hash_route_table.py shows, through the planner, that ROUTE_CASES below reaches every route and instantiation.

Rows x columns throughout.  300 clips for the persistent kernels (more clips than workgroups: the loops wrap), 2 clips per class elsewhere."""
import functools

import numpy as np
import pytest

import framegen
from oracle import vdf_oracle as orc

pytestmark = pytest.mark.gpu
TINY = 1e-6

M3 = {"VDF_RESIZE_MODE": "3"}
M4 = {"VDF_RESIZE_MODE": "4"}
# (name, h, w, n_clips, env, expected_route, expected_detail): a packed, 16-byte-aligned call of that size under that environment takes
# that HashRoute with those HashPlan values (checked on the CPU by test_hash_route_table.py).  The smallest frames that select each form.
# Frame bytes per row: the 300-clip rows 8 MB (36 x 48) ... 157 MB (128 x 256), the 8-clip rows 1 MB (96 x 64) ... 77 MB (300 x 2000) - 300
# clips of the smallest tiled shapes and 8 clips of the narrowest K-split width cannot be had in less; the largest row takes under 3 s.
ROUTE_CASES = [
    ("one_tile_full", 64, 64, 300, {}, "kPersistentOneTile", {"full_tile": 1}),
    ("one_tile_partial", 36, 48, 300, {}, "kPersistentOneTile", {"full_tile": 0}),
    ("tiled_1x2", 72, 48, 300, {}, "kTiled", {"n_kt": 1, "tiled_nrg": 2}),
    ("tiled_1x4", 136, 48, 300, {}, "kTiled", {"n_kt": 1, "tiled_nrg": 4}),
    ("tiled_2x1", 40, 80, 300, {}, "kTiled", {"n_kt": 2, "tiled_nrg": 1}),
    ("tiled_2x2_last_clip_apart", 72, 90, 300, {}, "kTiled", {"n_kt": 2, "tiled_nrg": 2, "last_clip_apart": 1}),
    ("tiled_2x4", 192, 128, 300, {}, "kTiled", {"n_kt": 2, "tiled_nrg": 4}),
    ("tiled_3x1", 40, 144, 300, {}, "kTiled", {"n_kt": 3, "tiled_nrg": 1}),
    ("tiled_3x2", 96, 160, 300, {}, "kTiled", {"n_kt": 3, "tiled_nrg": 2}),
    ("tiled_3x4", 136, 144, 300, {}, "kTiled", {"n_kt": 3, "tiled_nrg": 4}),
    ("tiled_4x1", 40, 208, 300, {}, "kTiled", {"n_kt": 4, "tiled_nrg": 1}),
    ("tiled_4x2", 128, 256, 300, M3, "kTiled", {"n_kt": 4, "tiled_nrg": 2}),
    ("tiled_4x4", 136, 208, 300, M3, "kTiled", {"n_kt": 4, "tiled_nrg": 4}),
    ("per_clip_fused", 96, 64, 8, {"VDF_HASH_NO_PERSISTENT": "1"}, "kPerClipFused", {}),
    ("chunk_stream", 270, 480, 8, {}, "kChunkStream", {"nb": 4, "pitch": 480, "shift": 0}),
    ("chunk_stream_shifted_repitched", 256, 333, 8, {}, "kChunkStream", {"nb": 4, "pitch": 336, "shift": 1}),
    ("wave_stream_8", 130, 640, 8, {}, "kWaveStream", {"waves": 8}),
    ("wave_stream_6", 140, 1024, 8, {}, "kWaveStream", {"waves": 6, "pitch": 1040}),
    ("wave_stream_5", 136, 1440, 8, {}, "kWaveStream", {"waves": 5}),
    ("wave_stream_4", 150, 1920, 8, {}, "kWaveStream", {"waves": 4}),
    ("wave_stream_3", 144, 1950, 8, {}, "kWaveStream", {"waves": 3, "shift": 1}),
    ("ksplit_forced", 130, 1040, 8, {"VDF_RESIZE_MODE": "6"}, "kKsplit", {"nb": 4}),
    ("ksplit_default", 300, 2000, 8, {}, "kKsplit", {"nb": 2}),
    ("whole_line_forced_narrow", 131, 67, 8, M4, "kWholeLine", {}),
    ("whole_line_forced", 200, 136, 8, M4, "kWholeLine", {}),
    ("whole_line_default", 301, 203, 8, {}, "kWholeLine", {}),
    ("scalar", 97, 150, 8, {"VDF_RESIZE_MODE": "1"}, "kScalar", {}),
]
CROP_SIZES = [(360, 640), (576, 720)]
CROP_SMALL = (96, 128)
LETTERBOX_SIZES = [(64, 64, 32), (90, 160, 32), (360, 640, 8)]  # h, w, clips


def corpus_sizes():
    """Every frame size this file hashes (tests/test_hash_content_corpus.py checks the corpus at each)."""
    sizes = [(h, w) for _, h, w, _, _, _, _ in ROUTE_CASES] + CROP_SIZES + [CROP_SMALL] + [(h, w) for h, w, _ in LETTERBOX_SIZES]
    return sorted(set(sizes), key=lambda s: (s[0] * s[1], s))


def _bits(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little").reshape(len(words), 1024)


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


def _expected(clips):
    """The oracle's hash words and don't-care counts of a list of clips ([16, h, w] each; sizes may differ)."""
    hs, dcs = [], []
    for clip in clips:
        rc, hw, coefs = orc.hash_clip(np.ascontiguousarray(clip), want_coefs=True)
        assert rc == 0
        hs.append(hw)
        dcs.append(int((np.abs(coefs) < TINY).sum()))
    return np.stack(hs), np.array(dcs, np.uint32)


def _compare(what, got, dc, want, want_dc, kinds):
    """As test_gpu_hash_parity._check: all 1000 bits unmasked, padding bits zero, the don't-care count the oracle's."""
    gb, wb = _bits(got), _bits(want)
    bad = (gb[:, :1000] != wb[:, :1000]).sum(axis=1)
    assert not bad.any(), f"{what}: hash bits differ in " + ", ".join(f"clip {i} ({kinds[i]}): {bad[i]}" for i in np.nonzero(bad)[0])
    assert (gb[:, 1000:] == 0).all(), f"{what}: padding bits set"
    off = np.nonzero(dc != want_dc)[0]
    assert len(off) == 0, f"{what}: don't-care count differs from the oracle's in " + ", ".join(f"clip {i} ({kinds[i]})" for i in off)


def _device_hash(eng, d_base, n, w, h, frame_stride=None, clip_stride=None, crops=None):
    import torch

    out = torch.zeros((n, 16), dtype=torch.int64, device="cuda")
    dc = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if crops is None:
        eng.hash_frames_device(d_base, n, 16, w, h, out.data_ptr(), d_dontcare=dc.data_ptr(), frame_stride=frame_stride, clip_stride=clip_stride)
    else:
        eng.hash_frames_cropped_device(d_base, n, 16, w, h, crops, out.data_ptr(), d_dontcare=dc.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64), dc.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("case", ROUTE_CASES, ids=[c[0] for c in ROUTE_CASES])
def test_saturating_content_matches_oracle_on_every_route(case, monkeypatch):
    """Packed and aligned (the route the row names), then the same clips at a base 3 bytes off with padded frame and clip strides (the
    careful loaders, the whole-line kernel for everything that does not fuse): the oracle's hashes both times."""
    import torch

    name, h, w, n, env, _, _ = case
    frames, kinds = framegen.interleaved(np.random.default_rng([h, w, 31]), n // 4, h, w)
    want, want_dc = _expected(frames)
    base, fs = 3, w * h + 37
    cs = 16 * fs + 101
    buf = np.full(base + (n - 1) * cs + 15 * fs + w * h, 0xAB, np.uint8)  # ends at the last byte of the last frame
    np.lib.stride_tricks.as_strided(buf[base:], shape=(n, 16, w * h), strides=(cs, fs, 1))[...] = frames.reshape(n, 16, w * h)
    d_packed, d_odd = torch.from_numpy(frames).cuda(), torch.from_numpy(buf).cuda()
    eng = _engine(env, monkeypatch)
    try:
        got, dc = _device_hash(eng, d_packed.data_ptr(), n, w, h)
        _compare(f"{name} {h}x{w} packed", got, dc, want, want_dc, kinds)
        got, dc = _device_hash(eng, d_odd.data_ptr() + base, n, w, h, frame_stride=fs, clip_stride=cs)
        _compare(f"{name} {h}x{w} base + 3, padded strides", got, dc, want, want_dc, kinds)
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _crop_corpus(h, w):
    frames, kinds = framegen.interleaved(np.random.default_rng([h, w, 37]), 2, h, w)
    frames.setflags(write=False)
    return frames, kinds


def _boxes(kind, h, w, n):
    """[n, 4] = left, right, top, bottom."""
    rng = np.random.default_rng([h, w, len(kind)])
    crops = np.zeros((n, 4), np.uint32)
    crops[:, 2] = rng.integers(0, h // 4, size=n)
    crops[:, 3] = rng.integers(0, h // 4, size=n)
    if kind == "rows":        # top / bottom bars only: the ROWCROP launch of the width's stream kernel
        crops[0, 2:] = (h // 8, 0)
    elif kind == "shared":    # one column range for all clips (the box stays wider than 512): the per-wave box launch
        crops[:, 0], crops[:, 1] = w // 16 + 8, w // 16 + 8
    elif kind == "unique":    # every clip its own range, some starting off a dword: the gather kernel
        crops[:, 0] = 1 + 3 * np.arange(n)
        crops[:, 1] = rng.integers(0, w // 5, size=n)
    else:                     # mixed (small frames: one kernel whatever the boxes), one clip whole
        crops[:, 0] = rng.integers(0, w // 5, size=n)
        crops[:, 1] = rng.integers(0, w // 5, size=n)
        crops[1::3, :2] = 0
        crops[0] = 0
    return crops


CROP_CASES = [(h, w, kind, mode) for h, w in CROP_SIZES for kind in ("rows", "shared", "unique") for mode in (0, 4)] + \
             [(*CROP_SMALL, "mixed", 0), (*CROP_SMALL, "mixed", 4)]


@functools.lru_cache(maxsize=None)
def _crop_expected(h, w, kind):
    frames, _ = _crop_corpus(h, w)
    crops = _boxes(kind, h, w, len(frames))
    return crops, _expected([frames[c][:, t:h - b, l:w - r] for c, (l, r, t, b) in enumerate(crops.tolist())])


@pytest.mark.parametrize("h,w,kind,mode", CROP_CASES, ids=[f"{h}x{w}-{k}-mode{m}" for h, w, k, m in CROP_CASES])
def test_saturating_content_through_the_cropped_kernels(h, w, kind, mode, monkeypatch):
    """vdf_hash_frames_u8_cropped_device on corpus frames: boxes with top / bottom bars only, one shared side-bar range, unique ranges -
    by default (ROWCROP launch, per-wave box launch, gather kernel) and under VDF_RESIZE_MODE=4 (the whole-line cropped kernel); 96 x 128:
    resize_dct_hash_cropped_small_kernel.  Expected: the oracle's hash of the cropped copy."""
    import torch

    frames, kinds = _crop_corpus(h, w)
    crops, (want, want_dc) = _crop_expected(h, w, kind)
    d = torch.from_numpy(frames.copy()).cuda()
    eng = _engine({"VDF_RESIZE_MODE": "4"} if mode == 4 else {}, monkeypatch)
    try:
        got, dc = _device_hash(eng, d.data_ptr(), len(frames), w, h, crops=crops)
    finally:
        eng.close()
    _compare(f"cropped {h}x{w} {kind} mode {mode}, boxes {crops.tolist()}", got, dc, want, want_dc, kinds)


@functools.lru_cache(maxsize=None)
def _letterbox_corpus(h, w, n):
    """Corpus clips with painted bars of value 16: top / bottom, left / right, both, none - by clip.  (Dark blocks that touch the border read
    as more bar, and the sparse classes as nothing but bar - an empty box, which is no box: both sides hash the whole frame.)"""
    rng = np.random.default_rng([h, w, 41])
    frames, kinds = framegen.interleaved(rng, n // 4, h, w)
    for c in range(n):
        style = (c // 4) % 4
        t, b = (int(x) for x in rng.integers(1, max(2, h // 6), size=2))
        l, r = (int(x) for x in rng.integers(1, max(2, w // 6), size=2))
        if style in (0, 2):
            frames[c, :, :t] = 16
            frames[c, :, h - b:] = 16
        if style in (1, 2):
            frames[c, :, :, :l] = 16
            frames[c, :, :, w - r:] = 16
    res = [orc.hash_clip_letterbox(clip, want_coefs=True) for clip in frames]
    assert all(r[0] == 0 for r in res)
    want = np.stack([r[1] for r in res])
    want_dc = np.array([(np.abs(r[2]) < TINY).sum() for r in res], np.uint32)
    want_crops = np.array([r[3] for r in res], np.uint32)
    frames.setflags(write=False)
    return frames, kinds, want, want_dc, want_crops


@pytest.mark.parametrize("no_fused", [False, True], ids=["default", "no_lb_fused"])
@pytest.mark.parametrize("h,w,n", LETTERBOX_SIZES, ids=[f"{h}x{w}" for h, w, _ in LETTERBOX_SIZES])
def test_saturating_content_through_the_letterbox_routes(h, w, n, no_fused, monkeypatch):
    """vdf_hash_frames_u8_letterbox: 64 x 64 (detect + crop + hash in one kernel), 90 x 160 (boxes kept on the device), 360 x 640 (boxes
    planned on the host: the cropped kernels), each by default and under VDF_NO_LB_FUSED: boxes and hashes equal to the oracle's."""
    frames, kinds, want, want_dc, want_crops = _letterbox_corpus(h, w, n)
    assert len({tuple(c) for c in want_crops.tolist()}) >= 4  # the painted bars are found, and differ by clip
    eng = _engine({"VDF_NO_LB_FUSED": "1"} if no_fused else {}, monkeypatch)
    try:
        got, crops, dc = eng.hash_frames_letterbox(frames, want_dontcare=True)
    finally:
        eng.close()
    off = np.nonzero((crops != want_crops).any(axis=1))[0]
    assert len(off) == 0, f"letterbox {h}x{w}: boxes differ in " + ", ".join(f"clip {i} ({kinds[i]}): {crops[i].tolist()} for {want_crops[i].tolist()}" for i in off)
    _compare(f"letterbox {h}x{w}", got, dc, want, want_dc, kinds)
