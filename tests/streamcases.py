"""Shared by the stream-order tests (DESIGN.md "Stream contract"): one case per _device entry point of include/vdf.h - for the hash family
one per kernel route - each with THREE valid input sets of the same shapes and sizes and the expected result on every one of them.

include/vdf.h promises that a _device call runs on the stream it is given and nowhere else.  tests/test_gpu_stream_order.py makes the call
while the stream still holds a delay, a fill of the outputs and the copies that bring `real` into buffers that hold `decoy`, and overwrites
the inputs with `decoy2` behind the call.  A result on `decoy` means the call ran ahead of its stream, a result on `decoy2` that it left
work behind.  All three sets are VALID inputs - first arrays monotone and inside their hashes, durations ascending, crop boxes and clip
descriptors inside the buffer - so that a violation shows as wrong words, never as a stray access.

Expected results come from the independent references, never from the library: oracle.vdf_oracle for hashes, planes, boxes and the search,
the numpy twins (aligngen, stretchgen, seedgen, variantgen, seedvariantgen, retimedaligngen) for the align calls, plain numpy for the rest.
tests/test_stream_order_cases.py (CPU) shows that every case can fail: the three expectations differ in every output.

A case: sets = [real, decoy, decoy2], each a dict name -> array; the names in `host` are HOST arrays of the call (descriptors, lists), the
others device buffers.  outputs: name -> (shape, dtype) of the device outputs; a name in `inout` is in the sets too (its value before the
call).  run(eng, p, h, stream) makes the call: p = name -> device address of every device input and output, h = name -> the host arrays
(the caller owns them and may overwrite them as soon as run returns); it returns what the call hands back on the host, or None.
expect(s) -> name -> array for every output, and "host" -> what run returns.  valid(s) asserts the validity rules on one set."""
from __future__ import annotations

import functools
from typing import Callable, NamedTuple

import numpy as np

import aligngen
import hashgen
import planegen
import retimedaligngen
import seedgen
import seedvariantgen
import stretchgen
import variantgen
import windowgen
from oracle import vdf_oracle as orc

# vdf_clip (include/vdf.h), restated: offset, frame_stride, w, h, crop = left, right, top, bottom
CLIP = np.dtype([("offset", np.uint64), ("frame_stride", np.uint64), ("w", np.uint32), ("h", np.uint32), ("crop", np.uint32, (4,))])
PAIR = np.dtype([("a", "<u4"), ("b", "<u4")])
TRIPLE = np.dtype([("a", "<u4"), ("b", "<u4"), ("variant", "<u4")])
U64, U32, U8 = np.uint64, np.uint32, np.uint8
FILL = 0xAB  # what the GPU test fills every output with, on the stream, in front of the call


class Case(NamedTuple):
    name: str
    symbols: tuple
    sets: list
    host: tuple
    outputs: dict
    inout: tuple
    run: Callable
    expect: Callable
    valid: Callable
    cold: bool   # hash family: the first call of a frame size on a fresh context uploads tables - run cold, then warm
    env: dict    # environment of the context's creation (a forced kernel route)


_REG = {}


def _case(name, *symbols, cold=False, env=None):
    def deco(fn):
        assert name not in _REG
        _REG[name] = (symbols, fn, cold, env or {})
        return fn
    return deco


def names() -> list:
    return list(_REG)


def symbols_of(name: str) -> tuple:
    return _REG[name][0]


def is_cold(name: str) -> bool:
    return _REG[name][2]


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    symbols, fn, cold, env = _REG[name]
    d = fn()
    c = Case(name, symbols, d["sets"], tuple(d.get("host", ())), d["outputs"], tuple(d.get("inout", ())), d["run"], d["expect"],
             d.get("valid", lambda s: None), cold, env)
    assert len(c.sets) == 3
    for s in c.sets[1:]:
        assert s.keys() == c.sets[0].keys()
        for k, v in s.items():
            assert v.shape == c.sets[0][k].shape and v.dtype == c.sets[0][k].dtype and v.size, (name, k)
    return c


@functools.lru_cache(maxsize=None)
def expected(name: str, k: int) -> dict:
    """The expected result of case `name` on set k (0 real, 1 decoy, 2 decoy2): output name -> array, "host" -> what run returns."""
    c = case(name)
    e = c.expect(c.sets[k])
    for o, (shape, dtype) in c.outputs.items():
        e[o] = np.ascontiguousarray(e[o], dtype=dtype).reshape(shape)
    assert set(e) - {"host"} == set(c.outputs), (name, sorted(e))
    return e


def filled(shape, dtype) -> np.ndarray:
    """What an output nobody wrote holds after the fill."""
    a = np.empty(shape, dtype)
    a.view(U8).fill(FILL)
    return a


def same(x, y) -> bool:
    if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
        return np.array_equal(x, y)
    return x == y


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
def _clips(seed, k, n, h, w):
    """n clips of 16 noise frames; clips k and k + 3 are static (one frame 16 times: 900 exact zeros), so that the don't-care counts and
    the zero planes of the three sets differ too."""
    rng = np.random.default_rng([61, seed, k])
    f = rng.integers(0, 256, size=(n, 16, h, w), dtype=U8)
    for c in (k, k + 3):
        f[c] = f[c, :1]
    return f


def _boxed(seed, k, n, h, w):
    """letterboxed clips: bars at 16, content 40 ... 219; the bar widths of a clip depend on its index and on the set; clips k and k + 3 static"""
    rng = np.random.default_rng([62, seed, k])
    f = rng.integers(40, 220, size=(n, 16, h, w), dtype=U8)
    for c in (k, k + 3):
        f[c] = f[c, :1]
    for c in range(n):
        t, b = ((c + k) % 4) * max(1, h // 16), ((c + 2 * k + 1) % 3) * max(1, h // 20)
        l, r = ((c + k + 1) % 3) * max(1, w // 16), ((2 * c + k) % 4) * max(1, w // 20)
        f[c, :, :t] = 16
        f[c, :, h - b:] = 16
        f[c, :, :, :l] = 16
        f[c, :, :, w - r:] = 16
    return f


def _crops(seed, k, n, h, w):
    """n crop boxes l, r, t, b that leave at least half of each axis; the first is the whole frame"""
    rng = np.random.default_rng([63, seed, k])
    c = np.stack([rng.integers(0, w // 4 + 1, n), rng.integers(0, w // 4 + 1, n), rng.integers(0, h // 4 + 1, n), rng.integers(0, h // 4 + 1, n)], axis=1)
    c[0] = 0
    return c.astype(U32)


def _cut(frames, crop):
    l, r, t, b = (int(x) for x in crop)
    h, w = frames.shape[-2:]
    return np.ascontiguousarray(frames[..., t:h - b, l:w - r])


def _oracle(stack):
    """(hash [16], don't-care count, zero plane [16]) of one [16, h, w] stack by the oracle"""
    rc, words, coefs = orc.hash_clip(np.ascontiguousarray(stack), want_coefs=True)
    assert rc == 0
    return words, int((np.abs(coefs) < 1e-6).sum()), planegen.pack_bits(coefs == 0.0)


def _oracle_many(stacks):
    r = [_oracle(s) for s in stacks]
    return np.stack([x[0] for x in r]), np.array([x[1] for x in r], U32), np.stack([x[2] for x in r])


def _oracle_windows(video, stride=1, rate=(1, 1)):
    """every (retimed) window of one [F, h, w] video: window k = frames k * stride + (i * num) // den, i < 16 (include/vdf.h)"""
    taps = np.array([(i * rate[0]) // rate[1] for i in range(16)])
    n_win = (len(video) - int(taps[-1]) - 1) // stride + 1
    return _oracle_many([video[k * stride + taps] for k in range(n_win)])


def _valid_box(crop, w, h):
    l, r, t, b = (int(x) for x in crop)
    assert l + r < w and t + b < h, "a crop box that leaves no pixels"


# ---- the uniform hash calls, one per kernel route ------------------------------------------------------------------------------------------------
N_CLIPS = 8


def _hash_frames(seed, h, w):
    def run(eng, p, hst, stream):
        eng.hash_frames_device(p["frames"], N_CLIPS, 16, w, h, p["hashes"], p["dontcare"], stream=stream)

    def expect(s):
        words, dc, _ = _oracle_many(s["frames"])
        return {"hashes": words, "dontcare": dc}
    return dict(sets=[{"frames": _clips(seed, k, N_CLIPS, h, w)} for k in range(3)], outputs={"hashes": ((N_CLIPS, 16), U64), "dontcare": ((N_CLIPS,), U32)},
                run=run, expect=expect)


# (h, w) and the route the planner gives it (tests/test_hash_route_table.py, tests/test_gpu_hash_parity.py)
for _name, _h, _w in (("direct_16x16", 16, 16), ("fused_64x64", 64, 64), ("tiled_96x96", 96, 96), ("chunk_270x480", 270, 480), ("wave_360x640", 360, 640)):
    _case("hash_frames_" + _name, "vdf_hash_frames_u8_device", cold=True)(functools.partial(_hash_frames, 1, _h, _w))
# the scalar fixed-point kernel, by force: the only route through axis_table
_case("hash_frames_scalar_131x67", "vdf_hash_frames_u8_device", cold=True, env={"VDF_RESIZE_MODE": "1"})(functools.partial(_hash_frames, 2, 131, 67))


@_case("hash_frames_planes_96x96", "vdf_hash_frames_u8_planes_device", cold=True)
def _hash_frames_planes(h=96, w=96):
    def run(eng, p, hst, stream):
        eng.hash_frames_planes_device(p["frames"], N_CLIPS, 16, w, h, p["hashes"], p["zero"], p["dontcare"], stream=stream)

    def expect(s):
        words, dc, zero = _oracle_many(s["frames"])
        return {"hashes": words, "dontcare": dc, "zero": zero}
    return dict(sets=[{"frames": _clips(3, k, N_CLIPS, h, w)} for k in range(3)],
                outputs={"hashes": ((N_CLIPS, 16), U64), "dontcare": ((N_CLIPS,), U32), "zero": ((N_CLIPS, 16), U64)}, run=run, expect=expect)


@_case("hash_frames_cropped_96x80", "vdf_hash_frames_u8_cropped_device", cold=True)
def _hash_frames_cropped(h=96, w=80):
    def run(eng, p, hst, stream):  # crops: the caller's own HOST array, straight through the C ABI
        eng._check(eng.lib.vdf_hash_frames_u8_cropped_device(eng.ctx, p["frames"], N_CLIPS, 16, w, h, w * h, 16 * w * h, hst["crops"].ctypes.data, p["hashes"],
                                                             p["dontcare"], stream))

    def expect(s):
        words, dc, _ = _oracle_many([_cut(f, c) for f, c in zip(s["frames"], s["crops"])])
        return {"hashes": words, "dontcare": dc}

    def valid(s):
        for c in s["crops"]:
            _valid_box(c, w, h)
    return dict(sets=[{"frames": _clips(4, k, N_CLIPS, h, w), "crops": _crops(4, k, N_CLIPS, h, w)} for k in range(3)], host=("crops",),
                outputs={"hashes": ((N_CLIPS, 16), U64), "dontcare": ((N_CLIPS,), U32)}, run=run, expect=expect, valid=valid)


def _letterbox_expect(frames):
    r = [orc.hash_clip_letterbox(f, want_coefs=True) for f in frames]
    assert all(x[0] == 0 for x in r)
    return (np.stack([x[1] for x in r]), np.array([int((np.abs(x[2]) < 1e-6).sum()) for x in r], U32), np.array([x[3] for x in r], U32))


def _letterbox(seed, h, w, mode):
    """mode: "host" (boxes to the host: the call ends with a wait), "async" (boxes stay on the device), "detect" (boxes only)"""
    def run(eng, p, hst, stream):
        if mode == "detect":
            return eng.cropdetect_letterbox_device(p["frames"], N_CLIPS, 16, w, h, p["crops"], stream=stream)
        if mode == "async":
            return eng.hash_frames_letterbox_device(p["frames"], N_CLIPS, 16, w, h, p["hashes"], p["dontcare"], stream=stream, d_crops=p["crops"])
        return eng.hash_frames_letterbox_device(p["frames"], N_CLIPS, 16, w, h, p["hashes"], p["dontcare"], stream=stream).tolist()

    def expect(s):
        words, dc, crops = _letterbox_expect(s["frames"])
        return {"detect": {"crops": crops}, "async": {"hashes": words, "dontcare": dc, "crops": crops},
                "host": {"hashes": words, "dontcare": dc, "host": crops.tolist()}}[mode]
    outputs = {"hashes": ((N_CLIPS, 16), U64), "dontcare": ((N_CLIPS,), U32), "crops": ((N_CLIPS, 4), U32)}
    for drop in {"detect": ("hashes", "dontcare"), "async": (), "host": ("crops",)}[mode]:
        del outputs[drop]
    return dict(sets=[{"frames": _boxed(seed, k, N_CLIPS, h, w)} for k in range(3)], outputs=outputs, run=run, expect=expect)


# 64 x 64: detect, crop and hash in one kernel; 160 x 90: detect kernels, then the cropped kernel reads the boxes on the device; 270 x 480: the
# kernel per box shape is chosen on the host, the call waits for its detect (tests/test_gpu_letterbox_no_host_sync.py, include/vdf.h)
_case("cropdetect_letterbox_160x90", "vdf_cropdetect_letterbox_device", cold=True)(functools.partial(_letterbox, 5, 90, 160, "detect"))
_case("cropdetect_letterbox_270x480", "vdf_cropdetect_letterbox_device", cold=True)(functools.partial(_letterbox, 6, 270, 480, "detect"))
_case("hash_frames_letterbox_64x64", "vdf_hash_frames_u8_letterbox_device", cold=True)(functools.partial(_letterbox, 7, 64, 64, "host"))
_case("hash_frames_letterbox_270x480", "vdf_hash_frames_u8_letterbox_device", cold=True)(functools.partial(_letterbox, 8, 270, 480, "host"))
_case("hash_frames_letterbox_async_64x64", "vdf_hash_frames_u8_letterbox_device_async", cold=True)(functools.partial(_letterbox, 9, 64, 64, "async"))
_case("hash_frames_letterbox_async_160x90", "vdf_hash_frames_u8_letterbox_device_async", cold=True)(functools.partial(_letterbox, 10, 90, 160, "async"))
_case("hash_frames_letterbox_async_270x480", "vdf_hash_frames_u8_letterbox_device_async", cold=True)(functools.partial(_letterbox, 11, 270, 480, "async"))


# ---- clips of three frame sizes in one buffer --------------------------------------------------------------------------------------------------
MIXED_SIZES = ((16, 16), (48, 64), (40, 192), (48, 64), (16, 16), (40, 192))  # (h, w) of the buffer's slots


def _slots(sizes, n_frames):
    """slot i holds n_frames frames of sizes[i], on a 64-byte boundary: (offsets, buffer bytes)"""
    at, offs = 0, []
    for h, w in sizes:
        offs.append(at)
        at += (n_frames * h * w + 63) & ~63
    return offs, at


def _slot_buffer(frames, offs, total):
    buf = np.zeros(total, U8)
    for f, o in zip(frames, offs):
        buf[o:o + f.size] = f.reshape(-1)
    return buf


def _descriptors(sizes, offs, order, crops=None):
    """descriptor j names slot order[j] (and carries crops[j])"""
    d = np.zeros(len(order), CLIP)
    for j, s in enumerate(order):
        h, w = sizes[s]
        d[j]["offset"], d[j]["frame_stride"], d[j]["w"], d[j]["h"] = offs[s], h * w, w, h
        if crops is not None:
            d[j]["crop"] = crops[j]
    return d


def _valid_clips(s, n_frames_of=lambda s, j: 16):
    """every descriptor inside the buffer, every box inside its frame (include/vdf.h: offset + (n - 1) frame_stride + w h <= buf_bytes)"""
    for j, d in enumerate(s["clips"]):
        w, h = int(d["w"]), int(d["h"])
        assert w and h and int(d["frame_stride"]) >= w * h
        _valid_box(d["crop"], w, h)
        assert int(d["offset"]) + (n_frames_of(s, j) - 1) * int(d["frame_stride"]) + w * h <= s["buf"].size, "a clip outside the buffer"


def _slot_frames(s, d, n_frames=16):
    w, h, o = int(d["w"]), int(d["h"]), int(d["offset"])
    return s["buf"][o:o + n_frames * h * w].reshape(n_frames, h, w)


def _mixed(seed, mode):
    """mode: "plain", "planes" (descriptors with crop boxes), "letterbox" (boxes to the host), "detect" (boxes on the device)"""
    n = len(MIXED_SIZES)
    offs, total = _slots(MIXED_SIZES, 16)
    boxed = mode in ("letterbox", "detect")
    sets = []
    for k in range(3):
        frames = [(_boxed if boxed else _clips)(seed * 10 + i, k, 6, h, w)[(i + k) % 6] for i, (h, w) in enumerate(MIXED_SIZES)]  # some of them static
        order = np.roll(np.arange(n), k)  # the same slots under another descriptor order: clip j's hash is another clip's
        crops = None if boxed else np.stack([_crops(seed, k, 2, *MIXED_SIZES[s_])[(j + k) % 2] for j, s_ in enumerate(order)])
        sets.append({"buf": _slot_buffer(frames, offs, total), "clips": _descriptors(MIXED_SIZES, offs, order, crops)})

    def run(eng, p, hst, stream):
        args = (eng.ctx, p["buf"], total, hst["clips"].ctypes.data, n, 16)
        if mode == "plain":
            eng._check(eng.lib.vdf_hash_clips_u8_device(*args, p["hashes"], p["dontcare"], stream))
        elif mode == "planes":
            eng._check(eng.lib.vdf_hash_clips_u8_planes_device(*args, p["hashes"], p["dontcare"], p["zero"], stream))
        elif mode == "detect":
            eng._check(eng.lib.vdf_cropdetect_letterbox_clips_device(*args, p["crops"], stream))
        else:
            crops = np.zeros((n, 4), U32)
            eng._check(eng.lib.vdf_hash_clips_u8_letterbox_device(*args, p["hashes"], p["dontcare"], crops.ctypes.data, stream))
            return crops.tolist()

    def expect(s):
        if boxed:
            r = [_letterbox_expect(_slot_frames(s, d)[None]) for d in s["clips"]]
            words, dc, crops = np.concatenate([x[0] for x in r]), np.concatenate([x[1] for x in r]), np.concatenate([x[2] for x in r])
            return {"crops": crops} if mode == "detect" else {"hashes": words, "dontcare": dc, "host": crops.tolist()}
        words, dc, zero = _oracle_many([_cut(_slot_frames(s, d), d["crop"]) for d in s["clips"]])
        return {"hashes": words, "dontcare": dc, **({"zero": zero} if mode == "planes" else {})}
    outputs = {"detect": {"crops": ((n, 4), U32)}}.get(mode, {"hashes": ((n, 16), U64), "dontcare": ((n,), U32)})
    if mode == "planes":
        outputs = dict(outputs, zero=((n, 16), U64))
    return dict(sets=sets, host=("clips",), outputs=outputs, run=run, expect=expect, valid=_valid_clips)


_case("hash_clips_mixed", "vdf_hash_clips_u8_device", cold=True)(functools.partial(_mixed, 1, "plain"))
_case("hash_clips_planes_mixed", "vdf_hash_clips_u8_planes_device", cold=True)(functools.partial(_mixed, 2, "planes"))
_case("hash_clips_letterbox_mixed", "vdf_hash_clips_u8_letterbox_device", cold=True)(functools.partial(_mixed, 3, "letterbox"))
_case("cropdetect_letterbox_clips_mixed", "vdf_cropdetect_letterbox_clips_device", cold=True)(functools.partial(_mixed, 4, "detect"))


# ---- every window of a clip --------------------------------------------------------------------------------------------------------------------
WIN_FRAMES, RATE = 40, (6, 5)


def _videos(seed, k, n, n_frames, h, w):
    """videos with a static and a constant stretch (tests/windowgen.py) that begins at another frame in every set"""
    rng = np.random.default_rng([65, seed, k])
    return np.stack([windowgen.video(rng, n_frames, h, w, lead=2 + 3 * k + c) for c in range(n)])


def _windows(seed, h, w, mode):
    n, rate = 2, RATE if mode == "retimed" else (1, 1)
    n_win = WIN_FRAMES - (15 * rate[0]) // rate[1]

    def run(eng, p, hst, stream):
        a = (p["frames"], n, WIN_FRAMES, w, h, 1)
        if mode == "plain":
            eng.hash_windows_device(*a, p["hashes"], p["dontcare"], stream=stream)
        elif mode == "planes":
            eng.hash_windows_planes_device(*a, p["hashes"], p["zero"], p["dontcare"], stream=stream)
        else:
            eng.hash_windows_retimed_device(*a, rate, p["hashes"], p["dontcare"], stream=stream)

    def expect(s):
        r = [_oracle_windows(v, 1, rate) for v in s["frames"]]
        e = {"hashes": np.stack([x[0] for x in r]), "dontcare": np.stack([x[1] for x in r])}
        return dict(e, zero=np.stack([x[2] for x in r])) if mode == "planes" else e
    outputs = {"hashes": ((n, n_win, 16), U64), "dontcare": ((n, n_win), U32)}
    if mode == "planes":
        outputs["zero"] = ((n, n_win, 16), U64)
    return dict(sets=[{"frames": _videos(seed, k, n, WIN_FRAMES, h, w)} for k in range(3)], outputs=outputs, run=run, expect=expect)


_case("hash_windows_64x64", "vdf_hash_windows_u8_device", cold=True)(functools.partial(_windows, 1, 64, 64, "plain"))
_case("hash_windows_direct_16x16", "vdf_hash_windows_u8_device", cold=True)(functools.partial(_windows, 2, 16, 16, "plain"))  # the kernel reads the caller's frames
_case("hash_windows_planes_64x64", "vdf_hash_windows_u8_planes_device", cold=True)(functools.partial(_windows, 3, 64, 64, "planes"))
_case("hash_windows_planes_direct_16x16", "vdf_hash_windows_u8_planes_device", cold=True)(functools.partial(_windows, 4, 16, 16, "planes"))
_case("hash_windows_retimed_64x64", "vdf_hash_windows_u8_retimed_device", cold=True)(functools.partial(_windows, 5, 64, 64, "retimed"))
_case("hash_windows_retimed_direct_16x16", "vdf_hash_windows_u8_retimed_device", cold=True)(functools.partial(_windows, 6, 16, 16, "retimed"))

# three videos of two sizes and three lengths; every slot holds 40 frames, so that every length fits every slot
LIB_SIZES, LIB_FRAMES = ((16, 16), (48, 64), (16, 16)), (40, 33, 24)


def _windows_clips(seed, mode):
    n, rate = len(LIB_SIZES), RATE if mode == "retimed" else (1, 1)
    span = (15 * rate[0]) // rate[1] + 1
    offs, total = _slots(LIB_SIZES, WIN_FRAMES)
    rows = sum(f - span + 1 for f in LIB_FRAMES)
    sets = []
    for k in range(3):
        frames = [_videos(seed * 10 + i, k, 1, WIN_FRAMES, h, w)[0] for i, (h, w) in enumerate(LIB_SIZES)]
        order = np.roll(np.arange(n), k)
        crops = np.stack([_crops(seed, k, 2, *LIB_SIZES[s_])[(j + k) % 2] for j, s_ in enumerate(order)])
        # the lengths go round the other way: another first[] - every window lands elsewhere - over the same number of rows
        sets.append({"buf": _slot_buffer(frames, offs, total), "clips": _descriptors(LIB_SIZES, offs, order, crops),
                     "n_frames": np.roll(np.array(LIB_FRAMES, U32), -k)})

    def run(eng, p, hst, stream):
        a = (eng.ctx, p["buf"], total, hst["clips"].ctypes.data, hst["n_frames"].ctypes.data, n, 1)
        if mode == "plain":
            eng._check(eng.lib.vdf_hash_windows_clips_u8_device(*a, p["hashes"], p["dontcare"], stream))
        elif mode == "planes":
            eng._check(eng.lib.vdf_hash_windows_clips_u8_planes_device(*a, p["hashes"], p["dontcare"], p["zero"], stream))
        else:
            eng._check(eng.lib.vdf_hash_windows_clips_u8_retimed_device(*a, rate[0], rate[1], p["hashes"], p["dontcare"], stream))

    def expect(s):
        r = [_oracle_windows(_cut(_slot_frames(s, d, int(f)), d["crop"]), 1, rate) for d, f in zip(s["clips"], s["n_frames"])]
        e = {"hashes": np.concatenate([x[0] for x in r]), "dontcare": np.concatenate([x[1] for x in r])}
        return dict(e, zero=np.concatenate([x[2] for x in r])) if mode == "planes" else e

    def valid(s):
        _valid_clips(s, lambda s_, j: int(s_["n_frames"][j]))
        assert all(int(f) >= span for f in s["n_frames"]) and sum(int(f) - span + 1 for f in s["n_frames"]) == rows
    outputs = {"hashes": ((rows, 16), U64), "dontcare": ((rows,), U32)}
    if mode == "planes":
        outputs["zero"] = ((rows, 16), U64)
    return dict(sets=sets, host=("clips", "n_frames"), outputs=outputs, run=run, expect=expect, valid=valid)


_case("hash_windows_clips_mixed", "vdf_hash_windows_clips_u8_device", cold=True)(functools.partial(_windows_clips, 1, "plain"))
_case("hash_windows_clips_planes_mixed", "vdf_hash_windows_clips_u8_planes_device", cold=True)(functools.partial(_windows_clips, 2, "planes"))
_case("hash_windows_clips_retimed_mixed", "vdf_hash_windows_clips_u8_retimed_device", cold=True)(functools.partial(_windows_clips, 3, "retimed"))


# ---- variants ----------------------------------------------------------------------------------------------------------------------------------
def _hash_set(seed, k, n, density=0.05):
    rng = np.random.default_rng([66, seed, k])
    h = hashgen.random_hashes(rng, n)
    return rng, h, variantgen.random_planes(rng, h, density)


def _firsts(k, total):
    """four videos over `total` rows, cut elsewhere in every set (first[0] = 0, first[4] = total: every row belongs to a video)"""
    cuts = ((0.25, 0.5, 0.8), (0.1, 0.45, 0.6), (0.35, 0.7, 0.9))[k]
    return np.array([0] + [int(total * c) for c in cuts] + [total], U32)


def _valid_first(first, rows):
    f = first.astype(np.int64)
    assert np.all(np.diff(f) >= 0) and f[0] >= 0 and f[-1] <= rows, "a first array must be monotone and inside its hashes"


@_case("hash_variants", "vdf_hash_variants_device")
def _hash_variants(n=40, v=3):
    def run(eng, p, hst, stream):
        eng.hash_variants_device(p["hashes"], p["zero"], n, v, p["out"], stream=stream)
    sets = [dict(zip(("hashes", "zero"), _hash_set(1, k, n)[1:])) for k in range(3)]
    return dict(sets=sets, outputs={"out": ((n, 16), U64)}, run=run,
                expect=lambda s: {"out": variantgen.variant_twin(s["hashes"], s["zero"], np.array([0, n]), v)})


@_case("window_variants", "vdf_window_variants_device")
def _window_variants(n=60, v=5):
    def run(eng, p, hst, stream):
        eng.window_variants(p["hashes"], p["zero"], p["first"], 4, v, p["out"], p["skip"], p["out_skip"], stream=stream)
    sets = []
    for k in range(3):
        rng, h, z = _hash_set(2, k, n)
        sets.append({"hashes": h, "zero": z, "first": _firsts(k, n), "skip": (rng.random(n) < 0.3).astype(U8) * U8(1 + k)})

    def expect(s):
        out, out_skip = variantgen.variant_twin(s["hashes"], s["zero"], s["first"], v, s["skip"])
        return {"out": out, "out_skip": out_skip}
    return dict(sets=sets, outputs={"out": ((n, 16), U64), "out_skip": ((n,), U8)}, run=run, expect=expect, valid=lambda s: _valid_first(s["first"], n))


def _class_layout(rows_form):
    n, min_run, width = 60, 2, 72 if rows_form else 36

    def run(eng, p, hst, stream):
        return eng.window_class_layout_device(p["hashes"], p["first"], 4, p["out"], n, d_zero=p["zero"] if rows_form else 0, d_skip=p["skip"],
                                              min_run=min_run, stream=stream)
    sets = []
    for k in range(3):
        rng, h, z = _hash_set(3, k, n)
        # a set that begins and ends at another row in every set: another number of rows and of seeds
        first = np.array(((0, 15, 30, 48, 60), (3, 9, 27, 36, 58), (1, 22, 42, 50, 54))[k], U32)
        sets.append({"hashes": h, "zero": z, "first": first, "skip": (rng.random(n) < 0.3).astype(U8) * U8(1 + k)})

    def expect(s):
        got = seedvariantgen.class_layout_twin(s["hashes"], s["first"], s["zero"] if rows_form else None, s["skip"], min_run)
        out = filled((n, width), U32)  # room for n rows; the seeds are fewer, and the rows behind them stay as they were
        out[:len(got)] = got
        return {"out": out, "host": len(got)}
    return dict(sets=sets, outputs={"out": ((n, width), U32)}, run=run, expect=expect, valid=lambda s: _valid_first(s["first"], n))


_case("window_class_layout_rows", "vdf_window_class_layout_device")(functools.partial(_class_layout, True))
_case("window_class_layout_seeds", "vdf_window_class_layout_device")(functools.partial(_class_layout, False))


# ---- align: three videos of at most 70 windows against three others ------------------------------------------------------------------------------
ALIGN_A = ((40, 30, 70), (30, 70, 40), (70, 40, 30))  # window counts of A's videos, per set: other first arrays over the same 140 rows
ALIGN_B = ((35, 50, 20), (50, 20, 35), (20, 35, 50))
# (a, ka, b, kb, n, flips): windows kb ... of video b of B := windows ka ... of video a of A.  The second plant of every set is a second, shorter
# stretch of the first one's pair at another offset
ALIGN_PLANTS = (((2, 10, 0, 3, 25, (0, 30)), (2, 50, 0, 29, 6, 2), (0, 5, 1, 10, 20, (0, 30))),
                ((1, 20, 0, 5, 30, (0, 30)), (1, 60, 0, 40, 8, 1), (2, 0, 2, 10, 20, (0, 30))),
                ((0, 30, 2, 0, 30, (0, 30)), (0, 5, 2, 35, 10, 3), (1, 10, 1, 5, 25, (0, 30))))
ALIGN_TOL, ALIGN_MIN_RUN = 350, 2
PAIR_LISTS = (((0, 1), (1, 2), (2, 0), (2, 2)), ((0, 0), (1, 0), (1, 1), (2, 2)), ((0, 2), (1, 0), (1, 1), (2, 1)))


def _align_problem(k) -> aligngen.Problem:
    rng = np.random.default_rng([67, k])
    ah, af = aligngen.videos(rng, ALIGN_A[k])
    bh, bf = aligngen.videos(rng, ALIGN_B[k])
    for a, ka, b, kb, n, flips in ALIGN_PLANTS[k]:
        assert ka + n <= ALIGN_A[k][a] and kb + n <= ALIGN_B[k][b]
        aligngen.plant(rng, ah, af, a, ka, bh, bf, b, kb, n, flips)
    a_skip, b_skip = np.zeros(len(ah), U8), np.zeros(len(bh), U8)
    a, ka, b, kb, n, _ = ALIGN_PLANTS[k][2]
    a_skip[int(af[a]) + ka + n // 2] = 1 + k            # cuts the third plant's run in two
    b_skip[int(bf[b]) + kb + n // 4] = 200 + k          # ... and once more on B's side
    return aligngen.Problem(ah, af, bh, bf, ALIGN_TOL, ALIGN_MIN_RUN, a_skip, b_skip)


def _align_set(p):
    return {"a_hashes": p.a_hashes, "a_first": p.a_first, "a_skip": p.a_skip, "b_hashes": p.b_hashes, "b_first": p.b_first, "b_skip": p.b_skip}


def _problem_of(s) -> aligngen.Problem:
    return aligngen.Problem(s["a_hashes"], s["a_first"], s["b_hashes"], s["b_first"], ALIGN_TOL, ALIGN_MIN_RUN, s["a_skip"], s["b_skip"])


def _pair_list(k):
    out = np.zeros(len(PAIR_LISTS[k]), PAIR)
    out["a"], out["b"] = zip(*PAIR_LISTS[k])
    return out


def _valid_align(s, n_a=3, n_b=3):
    _valid_first(s["a_first"], len(s["a_hashes"]))
    _valid_first(s["b_first"], len(s["b_hashes"]))
    assert len(s["a_first"]) == n_a + 1 and len(s["b_first"]) == n_b + 1
    for key in ("pairs", "triples"):
        if key in s:
            keys = [((int(t["variant"]),) if key == "triples" else ()) + (int(t["a"]), int(t["b"])) for t in s[key]]
            assert keys == sorted(set(keys)) and all(int(t["a"]) < n_a and int(t["b"]) < n_b for t in s[key]), "a list must be strictly increasing and name videos that exist"
            assert key == "pairs" or all(1 <= int(t["variant"]) <= 7 for t in s[key])


def _sides(p):
    return dict(d_a_hashes=p["a_hashes"], d_a_first=p["a_first"], n_a=3, d_b_hashes=p["b_hashes"], d_b_first=p["b_first"], n_b=3, d_a_skip=p["a_skip"],
                d_b_skip=p["b_skip"], tol_int=ALIGN_TOL, min_run=ALIGN_MIN_RUN)


def _pairs_of(s):
    return [(int(t["a"]), int(t["b"])) for t in s["pairs"]]


def _align(call, records, twin, pairs=False, **kw):
    def run(eng, p, hst, stream):
        a = _sides(p)
        if pairs:
            a["pairs"] = hst["pairs"]
        rec, n = getattr(eng, call)(**a, **kw, stream=stream)
        assert n == len(rec)
        return records(rec)
    sets = [_align_set(_align_problem(k)) for k in range(3)]
    if pairs:
        for k, s in enumerate(sets):
            s["pairs"] = _pair_list(k)
    return dict(sets=sets, host=("pairs",) if pairs else (), outputs={}, run=run, expect=lambda s: {"host": twin(s)}, valid=_valid_align)


_case("align_windows", "vdf_align_windows_device")(functools.partial(_align, "align_windows_device", aligngen.records, lambda s: aligngen.align_twin(_problem_of(s))))
_case("align_windows_stretches", "vdf_align_windows_stretches_device")(functools.partial(
    _align, "align_windows_stretches_device", stretchgen.records, lambda s: stretchgen.stretches_twin(_problem_of(s), 4, 1), max_stretches=4, guard=1))
_case("align_seed_pairs", "vdf_align_seed_pairs_device")(functools.partial(_align, "align_seed_pairs_device", seedgen.pairs_of, lambda s: seedgen.seed_twin(_problem_of(s))))
_case("align_windows_pairs", "vdf_align_windows_pairs_device")(functools.partial(
    _align, "align_windows_pairs_device", aligngen.records, lambda s: seedgen.pairs_twin(_problem_of(s), _pairs_of(s)), pairs=True))
_case("align_windows_stretches_pairs", "vdf_align_windows_stretches_pairs_device")(functools.partial(
    _align, "align_windows_stretches_pairs_device", stretchgen.records, lambda s: seedgen.stretches_pairs_twin(_problem_of(s), _pairs_of(s), 4, 1), pairs=True,
    max_stretches=4, guard=1))


# ---- align against the variants of B --------------------------------------------------------------------------------------------------------------
VARIANT_MASK = (1 << 1) | (1 << 5)
# (a, ka, b, kb, n, variant): windows ka ... of video a of A := DERIVED rows kb ... of video b of B under the variant
VARIANT_PLANTS = (((2, 10, 0, 3, 25, 1), (0, 5, 1, 10, 20, 5)), ((1, 20, 0, 5, 30, 5), (2, 0, 2, 10, 20, 1)), ((0, 30, 2, 0, 30, 1), (1, 10, 1, 5, 25, 5)))
TRIPLE_LISTS = (((1, 0, 1), (1, 2, 0), (5, 0, 1), (5, 2, 2)), ((1, 2, 2), (5, 0, 0), (5, 1, 0), (5, 2, 1)), ((1, 0, 2), (1, 1, 1), (5, 1, 1), (5, 2, 0)))


def _variant_set(k):
    rng = np.random.default_rng([68, k])
    ah, af = aligngen.videos(rng, ALIGN_A[k])
    bh, bf = aligngen.videos(rng, ALIGN_B[k])
    bz = variantgen.random_planes(rng, bh)
    for a, ka, b, kb, n, v in VARIANT_PLANTS[k]:
        assert ka + n <= ALIGN_A[k][a] and kb + n <= ALIGN_B[k][b]
        variantgen.plant_variant(rng, ah, af, a, ka, bh, bz, bf, b, kb, n, v, 3)
    b_skip = np.zeros(len(bh), U8)
    b_skip[int(bf[VARIANT_PLANTS[k][0][2]]) + 12] = 1 + k  # a skipped row inside the first plant
    return {"a_hashes": ah, "a_first": af, "b_hashes": bh, "b_zero": bz, "b_first": bf, "b_skip": b_skip}


def _variant_problem_of(s) -> variantgen.VariantProblem:
    return variantgen.VariantProblem(aligngen.Problem(s["a_hashes"], s["a_first"], s["b_hashes"], s["b_first"], ALIGN_TOL, ALIGN_MIN_RUN, None, s["b_skip"]),
                                     None, s["b_zero"], VARIANT_MASK)


def _align_variants(call, records, twin, triples=False, **kw):
    def run(eng, p, hst, stream):
        a = dict(d_a_hashes=p["a_hashes"], d_a_first=p["a_first"], n_a=3, d_b_hashes=p["b_hashes"], d_b_first=p["b_first"], n_b=3, d_b_zero=p["b_zero"],
                 d_b_skip=p["b_skip"], tol_int=ALIGN_TOL, min_run=ALIGN_MIN_RUN)
        if triples:
            a["triples"] = hst["triples"]
        rec, n = getattr(eng, call)(**a, **kw, stream=stream)
        assert n == len(rec)
        return records(rec)
    sets = [_variant_set(k) for k in range(3)]
    if triples:
        for k, s in enumerate(sets):
            s["triples"] = np.zeros(len(TRIPLE_LISTS[k]), TRIPLE)
            s["triples"]["variant"], s["triples"]["a"], s["triples"]["b"] = zip(*TRIPLE_LISTS[k])
    return dict(sets=sets, host=("triples",) if triples else (), outputs={}, run=run, expect=lambda s: {"host": twin(s)}, valid=_valid_align)


_case("align_windows_variants", "vdf_align_windows_variants_device")(functools.partial(
    _align_variants, "align_windows_variants_device", variantgen.records, lambda s: variantgen.twin(_variant_problem_of(s)), variant_mask=VARIANT_MASK))
_case("align_seed_pairs_variants", "vdf_align_seed_pairs_variants_device")(functools.partial(
    _align_variants, "align_seed_pairs_variants_device", seedvariantgen.triples_of, lambda s: seedvariantgen.seed_twin(_variant_problem_of(s)),
    variant_mask=VARIANT_MASK))
_case("align_windows_variants_pairs", "vdf_align_windows_variants_pairs_device")(functools.partial(
    _align_variants, "align_windows_variants_pairs_device", variantgen.records,
    lambda s: seedvariantgen.records_twin(_variant_problem_of(s), [(int(t["variant"]), int(t["a"]), int(t["b"])) for t in s["triples"]]), triples=True))


# ---- align retimed windows -------------------------------------------------------------------------------------------------------------------------
ALIGN_RATE = (3, 2)
# (a, b, phase, i0, j0, n, flips): row 2 (j0 + m) of video b := row phase + 3 (i0 + m) of video a
RETIMED_PLANTS = (((0, 1, 1, 2, 3, 11, (0, 30)), (2, 0, 0, 1, 0, 8, 4)), ((1, 0, 2, 5, 2, 14, (0, 30)), (2, 2, 0, 0, 1, 9, 4)),
                  ((0, 2, 1, 3, 0, 15, (0, 30)), (1, 1, 0, 0, 2, 8, 4)))


def _retimed_set(k):
    rng = np.random.default_rng([69, k])
    ah, af = aligngen.videos(rng, ALIGN_A[k])
    bh, bf = aligngen.videos(rng, ALIGN_B[k])
    p = retimedaligngen.Problem(ah, af, bh, bf, ALIGN_RATE, ALIGN_TOL, ALIGN_MIN_RUN)
    for plant in RETIMED_PLANTS[k]:
        retimedaligngen.plant(rng, p, *plant)
    a_skip = np.zeros(len(ah), U8)
    a, _, phase, i0, _, n, _ = RETIMED_PLANTS[k][0]
    a_skip[int(af[a]) + phase + 3 * (i0 + n // 2)] = 1 + k  # cuts the first plant's run in two
    return {"a_hashes": ah, "a_first": af, "a_skip": a_skip, "b_hashes": bh, "b_first": bf}


def _retimed(pairs):
    def run(eng, p, hst, stream):
        a = dict(d_a_hashes=p["a_hashes"], d_a_first=p["a_first"], n_a=3, d_b_hashes=p["b_hashes"], d_b_first=p["b_first"], n_b=3, rate=ALIGN_RATE,
                 d_a_skip=p["a_skip"], tol_int=ALIGN_TOL, min_run=ALIGN_MIN_RUN, stream=stream)
        rec, n = eng.align_windows_retimed_pairs_device(pairs=hst["pairs"], **a) if pairs else eng.align_windows_retimed_device(**a)
        assert n == len(rec)
        return retimedaligngen.records(rec)

    def expect(s):
        p = retimedaligngen.Problem(s["a_hashes"], s["a_first"], s["b_hashes"], s["b_first"], ALIGN_RATE, ALIGN_TOL, ALIGN_MIN_RUN, s["a_skip"])
        return {"host": retimedaligngen.align_retimed_twin(p, _pairs_of(s) if pairs else None)}
    sets = [_retimed_set(k) for k in range(3)]
    if pairs:
        for k, s in enumerate(sets):
            s["pairs"] = _pair_list(k)
    return dict(sets=sets, host=("pairs",) if pairs else (), outputs={}, run=run, expect=expect, valid=_valid_align)


_case("align_windows_retimed", "vdf_align_windows_retimed_device")(functools.partial(_retimed, False))
_case("align_windows_retimed_pairs", "vdf_align_windows_retimed_pairs_device")(functools.partial(_retimed, True))


# ---- search ----------------------------------------------------------------------------------------------------------------------------------------
SEARCH_N, SEARCH_TOL = 600, 350


def _database(seed, k, n=SEARCH_N):
    rng = np.random.default_rng([70, seed, k])
    words, dur = hashgen.planted_set(rng, n, n_clusters=25, max_copies=8, durations="windowed")
    w, d, _ = hashgen.sort_by_duration(words, dur)
    return rng, np.ascontiguousarray(w), np.ascontiguousarray(d)


def _valid_durations(s):
    for key in ("durations", "cand_durations"):
        if key in s:
            assert np.all(np.diff(s[key].astype(np.int64)) >= 0), "durations must be ascending"


def _dense_database(seed, k, n=SEARCH_N, members=560):
    """560 of the 600 entries within 240 bits of each other, all inside each other's duration window: 156 520 hits - long enough for the device-side
    hit sort (2^17) and for the replay filter (2^16), whose kernels and counters then sit on the caller's stream too"""
    rng = np.random.default_rng([70, seed, k])
    words, base = hashgen.random_hashes(rng, n), hashgen.random_hashes(rng, 1)[0]
    for i in rng.choice(n, size=members, replace=False):
        words[i] = aligngen.flipped(base, int(rng.integers(0, 121)), rng)
    return rng, words, np.sort(rng.integers(1000, 1041, size=n)).astype(U32)


def _search_self(replay, dense=False):
    def run(eng, p, hst, stream):
        from vid_dup_finder_lib_amd import engine as ve   # the host replay of the hit list (CPU-tested: tests/test_capi_symbols.py)

        call = eng.search_self_device_replay if replay else eng.search_self_device
        hits, n_hits, overflow = call(p["hashes"], p["durations"], SEARCH_N, SEARCH_TOL, capacity=1 << 18, stream=stream)
        assert n_hits == len(hits) and overflow == 0xFFFFFFFF
        groups = ve.finish_self(ve.replay_self(SEARCH_N, hits))
        return groups if replay else (hits.tolist(), groups)

    def expect(s):
        groups = orc.search_self_sorted(s["hashes"], s["durations"], SEARCH_TOL)
        if replay:  # the replay form may drop hits the greedy loop never uses: the groups are the contract
            return {"host": groups}
        d = s["durations"]
        dist = hashgen.all_distances(s["hashes"], s["hashes"])
        hits = []
        for i in range(SEARCH_N):  # search_algorithm.rs:99: j in (i, first index with duration > (f64(duration[i]) * 1.1) as u32)
            rhs = int(np.searchsorted(d, np.uint32(min(int(float(d[i]) * 1.1), 2**32 - 1)), side="right"))
            hits += [[i, int(j)] for j in range(i + 1, rhs) if dist[i, j] <= SEARCH_TOL]
        return {"host": (hits, groups)}
    sets = [dict(zip(("hashes", "durations"), (_dense_database if dense else _database)(1 + replay, k)[1:])) for k in range(3)]
    return dict(sets=sets, outputs={}, run=run, expect=expect, valid=_valid_durations)


_case("search_self", "vdf_search_self_device")(functools.partial(_search_self, False))
_case("search_self_dense", "vdf_search_self_device")(functools.partial(_search_self, False, True))
_case("search_self_replay", "vdf_search_self_device_replay")(functools.partial(_search_self, True))
_case("search_self_replay_dense", "vdf_search_self_device_replay")(functools.partial(_search_self, True, True))


@_case("search_refs", "vdf_search_refs_device")
def _search_refs(n_ref=50):
    def run(eng, p, hst, stream):
        from vid_dup_finder_lib_amd import engine as ve

        hits, n_hits = eng.search_refs_device(p["cand_hashes"], p["cand_durations"], SEARCH_N, p["ref_hashes"], p["ref_durations"], n_ref, SEARCH_TOL,
                                              capacity=1 << 16, stream=stream)
        assert n_hits == len(hits)
        return ve.groups_from_ref_hits(hits)
    sets = []
    for k in range(3):
        rng, w, d = _database(3, k)
        pick = rng.choice(SEARCH_N, size=n_ref, replace=False)  # the references: entries of the database, a few bits off, in any order
        refs = np.stack([aligngen.flipped(w[i], int(rng.integers(0, 60)), rng) for i in pick])
        sets.append({"cand_hashes": w, "cand_durations": d, "ref_hashes": refs, "ref_durations": np.ascontiguousarray(d[pick])})
    return dict(sets=sets, outputs={}, run=run, valid=_valid_durations,
                expect=lambda s: {"host": orc.search_refs_sorted(s["cand_hashes"], s["cand_durations"], s["ref_hashes"], s["ref_durations"], SEARCH_TOL)})


@_case("search_variants", "vdf_search_variants_device")
def _search_variants(n=SEARCH_N, mask=(1 << 1) | (1 << 5)):
    def run(eng, p, hst, stream):
        return eng.search_variants_device(p["hashes"], p["zero"], p["durations"], n, SEARCH_TOL, mask, stream=stream)
    sets = []
    for k in range(3):
        rng = np.random.default_rng([70, 4, k])
        words, dur = hashgen.planted_set(rng, n, n_clusters=25, max_copies=8, durations="windowed")
        zero = variantgen.random_planes(rng, words)
        for i, (s_, t) in enumerate(rng.choice(n, size=(20, 2), replace=False)):  # t looks like the mirror (or the reversed mirror) of s_
            v = (1, 5)[i % 2]
            words[t] = aligngen.flipped((words[s_] ^ planegen.variant_mask(v)) & ~zero[s_], int(rng.integers(0, 40)), rng)
            words[t, 15] &= U64((1 << 40) - 1)
            zero[t] &= ~words[t]
            dur[t] = dur[s_]
        order = np.argsort(dur, kind="stable")
        sets.append({"hashes": np.ascontiguousarray(words[order]), "zero": np.ascontiguousarray(zero[order]), "durations": np.ascontiguousarray(dur[order])})

    def expect(s):
        out = {}
        for v in range(1, 8):
            if mask >> v & 1:  # the reference search with the variant-v hashes as references; (r, r) and emptied groups dropped
                res = orc.search_refs_sorted(s["hashes"], s["durations"], (s["hashes"] ^ planegen.variant_mask(v)) & ~s["zero"], s["durations"], SEARCH_TOL)
                out[v] = [(r, [m for m in ms if m != r]) for r, ms in res if [m for m in ms if m != r]]
        return {"host": out}
    return dict(sets=sets, outputs={}, run=run, expect=expect, valid=_valid_durations)


@_case("sort_order", "vdf_sort_order_device")
def _sort_order(n=SEARCH_N):
    def run(eng, p, hst, stream):
        eng.sort_order_device(p["durations"], n, p["perm"], p["rank"], stream=stream)
    sets = []
    for k in range(3):
        rng = np.random.default_rng([71, k])
        sets.append({"durations": rng.integers(5, 60, size=n).astype(U32), "rank": rng.integers(0, 40, size=n).astype(U32)})
    # Search::sort: stable by (duration, path rank) - numpy's lexsort is stable, the last key is the primary one
    return dict(sets=sets, outputs={"perm": ((n,), U32)}, run=run, expect=lambda s: {"perm": np.lexsort((s["rank"], s["durations"]))})


@_case("apply_order", "vdf_apply_order_device")
def _apply_order(n=SEARCH_N):
    def run(eng, p, hst, stream):
        eng.apply_order_device(p["hashes"], p["durations"], p["perm"], n, p["hashes_out"], p["durations_out"], stream=stream)
    sets = []
    for k in range(3):
        rng = np.random.default_rng([72, k])
        sets.append({"hashes": hashgen.random_hashes(rng, n), "durations": rng.integers(5, 7200, size=n).astype(U32), "perm": rng.permutation(n).astype(U32)})

    def valid(s):
        assert sorted(s["perm"].tolist()) == list(range(n)), "perm must be a permutation"
    return dict(sets=sets, outputs={"hashes_out": ((n, 16), U64), "durations_out": ((n,), U32)}, run=run, valid=valid,
                expect=lambda s: {"hashes_out": s["hashes"][s["perm"]], "durations_out": s["durations"][s["perm"]]})


@_case("bitmap_or", "vdf_bitmap_or_device")
def _bitmap_or(n_words=301, n_srcs=3):
    def run(eng, p, hst, stream):
        eng.bitmap_or_device(p["dst"], p["srcs"], n_words, n_srcs, stream=stream)
    sets = []
    for k in range(3):
        rng = np.random.default_rng([73, k])
        sparse = lambda shape: (rng.integers(0, 2**32, size=shape, dtype=U32) & rng.integers(0, 2**32, size=shape, dtype=U32) & rng.integers(0, 2**32, size=shape, dtype=U32))
        sets.append({"dst": sparse(n_words), "srcs": sparse((n_srcs, n_words))})
    return dict(sets=sets, outputs={"dst": ((n_words,), U32)}, inout=("dst",), run=run,
                expect=lambda s: {"dst": s["dst"] | np.bitwise_or.reduce(s["srcs"], axis=0)})
