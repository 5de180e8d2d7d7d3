"""Engine: one vdf_ctx (one GPU) behind numpy-friendly methods.

Thin host plumbing over the C ABI (include/vdf.h).  All arithmetic of the hot path runs in
libvdf_hip.so on the GPU; nothing here computes a hash bit or a Hamming distance on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _capi
from ._capi import HASH_WORDS, VdfError, VdfGroups, VdfHit, VdfSearchStats, VdfSearchTiming

UINT32_MAX = 0xFFFFFFFF
# vdf_clip as a numpy record (include/vdf.h): offset, frame_stride, w, h, crop = left, right, top, bottom
CLIP_DTYPE = np.dtype([("offset", np.uint64), ("frame_stride", np.uint64), ("w", np.uint32), ("h", np.uint32), ("crop", np.uint32, (4,))])
assert CLIP_DTYPE.itemsize == C.sizeof(_capi.VdfClip) == 40


def _groups_to_lists(g: VdfGroups) -> List[Tuple[int, List[int]]]:
    offsets, members, refs = groups_to_arrays(g)
    offs = offsets.tolist()
    mem = members.tolist()
    return [(int(refs[i]), mem[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)]


def groups_to_arrays(g: VdfGroups):
    """(offsets u64[n+1], members u64[m], ref_index i64[n]) copies of a vdf_groups."""
    n = int(g.n_groups)
    offsets = np.ctypeslib.as_array(g.offsets, shape=(n + 1,)).copy() if g.offsets else np.zeros(1, np.uint64)
    m = int(offsets[-1])
    members = np.ctypeslib.as_array(g.members, shape=(m,)).copy() if m else np.zeros(0, np.uint64)
    refs = np.ctypeslib.as_array(g.ref_index, shape=(n,)).copy() if n else np.zeros(0, np.int64)
    return offsets, members, refs


def _ptr_array(ptrs: Sequence[int]):
    return (C.c_void_p * len(ptrs))(*[C.c_void_p(int(p) or None) for p in ptrs])


def _size_array(sizes: Sequence[int]):
    return (C.c_size_t * len(sizes))(*[int(x) for x in sizes])


def _atoi(text: str) -> int:
    """C's atoi: optional blanks, optional sign, leading digits; anything else counts as 0 (how csrc/api.cpp reads its switches)."""
    import re

    m = re.match(r"\s*([+-]?\d+)", text or "")
    return int(m.group(1)) if m else 0


def _window_stride(stride) -> int:
    """The window stride as the C ABI's uint32_t takes it.  ctypes would wrap a value outside the type without a word (-1 -> 2^32 - 1,
    2^32 + 1 -> 1) and the library would then write a different number of windows than the caller sized its output for."""
    s = int(stride)
    if s != stride or not 1 <= s < 2**32:
        raise ValueError(f"window stride must be an integer in 1 .. 2^32 - 1, not {stride!r}")
    return s


def _window_rate(rate):
    """A rate (num, den) as the C ABI's two uint32_t take it.  Whether it is a rate the calls offer (1 <= den <= num <= 2 den, num <= 65535)
    is the library's to say (VDF_E_INVAL); only what ctypes would wrap without a word is refused here."""
    try:
        num, den = rate
        n, d = int(num), int(den)
    except (TypeError, ValueError):
        raise ValueError(f"rate must be a pair of integers (num, den), not {rate!r}") from None
    if n != num or d != den or not (0 <= n < 2**32 and 0 <= d < 2**32):
        raise ValueError(f"rate must be a pair of integers (num, den) in 0 .. 2^32 - 1, not {rate!r}")
    return n, d


def hash_window_count_retimed(n_frames: int, stride: int, rate) -> int:
    """Retimed windows of a clip of n_frames frames (vdf_hash_window_count_retimed; host-only): 0 if the clip is shorter than a window's span
    or the rate is not one the calls take."""
    num, den = _window_rate(rate)
    return int(_capi.load().vdf_hash_window_count_retimed(int(n_frames), _window_stride(stride), num, den))


def _window_rates(rates):
    """A list of rates as the C ABI's two uint32_t arrays take it: (num [n] u32, den [n] u32).  How many there may be and which rates are
    offered is the library's to say."""
    pairs = [_window_rate(r) for r in rates]
    return np.array([p[0] for p in pairs], np.uint32), np.array([p[1] for p in pairs], np.uint32)


def hash_window_count_rates(n_clips: int, n_frames: int, stride: int, rates):
    """vdf_hash_window_count_rates (host only, no context): (rows, first [n_rates + 1]) of Engine.hash_windows_rates' rate-major outputs - rate
    r's windows of clip c are the rows first[r] + c * n_win_r ... .  (0, zeros) if there are no or more than 8 rates, or a rate has no window."""
    num, den = _window_rates(rates)
    first = np.zeros(len(num) + 1, np.uintp)
    total = _capi.load().vdf_hash_window_count_rates(int(n_clips), int(n_frames), _window_stride(stride), len(num), num.ctypes.data if len(num) else None,
                                                     den.ctypes.data if len(num) else None, first.ctypes.data)
    return int(total), first.astype(np.int64)


# one record of the align calls (include/vdf.h: vdf_alignment, 24 bytes)
ALIGN_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("offset", "<i4"), ("start_a", "<u4"), ("n_windows", "<u4"), ("dist_sum", "<u4")])


def hash_windows_first(n_frames, stride: int = 1) -> np.ndarray:
    """vdf_hash_windows_clips_first (host only, no context): first [n_videos + 1] u32 = the prefix sums of the videos' window counts - where
    Engine.hash_windows_clips puts video i's windows (rows first[i] ... first[i + 1]) and what the align calls read beside the hashes.
    VdfError: a video of fewer than 16 frames (VDF_E_NOT_ENOUGH_FRAMES), 2^32 windows or more (VDF_E_INVAL)."""
    nf = np.asarray(n_frames).reshape(-1)
    if nf.size and (np.any(nf != nf.astype(np.int64)) or int(nf.min()) < 0 or int(nf.max()) >= 2**32):
        raise ValueError("frame counts must be integers in 0 .. 2^32 - 1")
    nf = np.ascontiguousarray(nf, dtype=np.uint32)
    first = np.zeros(nf.size + 1, np.uint32)
    rc = _capi.load().vdf_hash_windows_clips_first(nf.ctypes.data if nf.size else None, nf.size, _window_stride(stride), first.ctypes.data)
    if rc != _capi.VDF_OK:
        raise VdfError(rc, "vdf_hash_windows_clips_first: " + ("a video of fewer than 16 frames" if rc == _capi.VDF_E_NOT_ENOUGH_FRAMES else "2^32 windows or more"))
    return first


def _library_rate(rate):
    """_window_rate, and a ValueError for a rate outside 1 <= den <= num <= 2 den, num <= 65535: the library calls size their output by it."""
    num, den = _window_rate(rate)
    if not (1 <= den <= num <= 2 * den and num <= 65535):
        raise ValueError(f"rate must satisfy 1 <= den <= num <= 2 den and num <= 65535, not {rate!r}")
    return num, den


def hash_windows_first_retimed(n_frames, rate, stride: int = 1) -> np.ndarray:
    """vdf_hash_windows_clips_first_retimed (host only, no context): first [n_videos + 1] u32 = the prefix sums of the videos' RETIMED window
    counts at rate = (num, den) - where Engine.hash_windows_clips_retimed puts video i's windows and what align_windows_retimed* reads beside
    the A side's hashes.  VdfError: a video of fewer frames than a retimed window spans (VDF_E_NOT_ENOUGH_FRAMES), a rate outside the range or
    2^32 windows or more (VDF_E_INVAL)."""
    nf = np.asarray(n_frames).reshape(-1)
    if nf.size and (np.any(nf != nf.astype(np.int64)) or int(nf.min()) < 0 or int(nf.max()) >= 2**32):
        raise ValueError("frame counts must be integers in 0 .. 2^32 - 1")
    nf = np.ascontiguousarray(nf, dtype=np.uint32)
    num, den = _window_rate(rate)
    first = np.zeros(nf.size + 1, np.uint32)
    rc = _capi.load().vdf_hash_windows_clips_first_retimed(nf.ctypes.data if nf.size else None, nf.size, _window_stride(stride), num, den, first.ctypes.data)
    if rc != _capi.VDF_OK:
        raise VdfError(rc, "vdf_hash_windows_clips_first_retimed: " + ("a video of fewer frames than a retimed window spans" if rc == _capi.VDF_E_NOT_ENOUGH_FRAMES
                                                                       else "a rate outside the range, or 2^32 windows or more"))
    return first


def hash_windows_first_rates(n_frames, rates, stride: int = 1):
    """vdf_hash_windows_clips_first_rates (host only, no context): (first [n_rates, n_videos + 1] u32, rate_first [n_rates + 1] int64) of
    Engine.hash_windows_clips_rates' rate-major outputs.  Row r of first is hash_windows_first_retimed(n_frames, rates[r], stride); window k of
    video i at rate r is row rate_first[r] + first[r, i] + k, and rate_first[-1] is the number of rows.  VdfError: a video of fewer frames than a
    window of one of the rates spans (VDF_E_NOT_ENOUGH_FRAMES); no or more than 8 rates, a rate outside the range or 2^32 rows or more
    (VDF_E_INVAL)."""
    nf = np.asarray(n_frames).reshape(-1)
    if nf.size and (np.any(nf != nf.astype(np.int64)) or int(nf.min()) < 0 or int(nf.max()) >= 2**32):
        raise ValueError("frame counts must be integers in 0 .. 2^32 - 1")
    nf = np.ascontiguousarray(nf, dtype=np.uint32)
    num, den = _window_rates(rates)
    first = np.zeros((max(len(num), 1), nf.size + 1), np.uint32)
    rate_first = np.zeros(len(num) + 1, np.uintp)
    rc = _capi.load().vdf_hash_windows_clips_first_rates(nf.ctypes.data if nf.size else None, nf.size, _window_stride(stride), len(num),
                                                         num.ctypes.data if len(num) else None, den.ctypes.data if len(num) else None, first.ctypes.data,
                                                         rate_first.ctypes.data)
    if rc != _capi.VDF_OK:
        raise VdfError(rc, "vdf_hash_windows_clips_first_rates: " + ("a video of fewer frames than a retimed window spans" if rc == _capi.VDF_E_NOT_ENOUGH_FRAMES
                                                                     else "no or more than 8 rates, a rate outside the range, or 2^32 rows or more"))
    return first[:len(num)], rate_first.astype(np.int64)


def _align_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip):
    """The host arrays of an align call as the C ABI takes them; b_hashes None = self mode.  Returns the arrays (to keep alive) and
    (a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip) as ctypes arguments."""
    def side(hashes, first, skip):
        h = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1, HASH_WORDS)
        f = np.ascontiguousarray(first, dtype=np.uint32).reshape(-1)
        if f.size == 0:
            raise ValueError("a first array has n_videos + 1 entries")
        if int(f.max()) > h.shape[0]:
            raise ValueError("a first array points behind its hashes")
        k = None
        if skip is not None:
            k = np.ascontiguousarray(skip, dtype=np.uint8).reshape(-1)
            if k.size != h.shape[0]:
                raise ValueError("one skip byte per window")
        return h, f, k
    ah, af, ak = side(a_hashes, a_first, a_skip)
    keep = [ah, af, ak]
    args = [ah.ctypes.data, af.ctypes.data, af.size - 1, ak.ctypes.data if ak is not None else None]
    if b_hashes is None:
        args += [None, None, 0, None]
    else:
        bh, bf, bk = side(b_hashes, b_first, b_skip)
        keep += [bh, bf, bk]
        # an empty B must not read as self mode (a NULL b_hashes): numpy gives an empty array a non-null address
        args += [bh.ctypes.data or af.ctypes.data, bf.ctypes.data, bf.size - 1, bk.ctypes.data if bk is not None else None]
    return keep, args


def _align_uint32(name: str, v) -> int:
    i = int(v)
    if i != v or not 0 <= i < 2**32:
        raise ValueError(f"{name} must be an integer in 0 .. 2^32 - 1, not {v!r}")
    return i


def align_windows_host(a_hashes, a_first, b_hashes=None, b_first=None, tol_int: int = 350, min_run: int = 1, a_skip=None, b_skip=None,
                       capacity: int = 1024):
    """vdf_align_windows_host: the definition of the align calls in plain C++ on the CPU (no context, no GPU) - for tiny inputs and tests.
    -> (records [min(found, capacity)] of ALIGN_DTYPE in (a, b) order, found); found > capacity: call again with a larger capacity."""
    lib = _capi.load()
    keep, args = _align_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)
    out = np.zeros(max(int(capacity), 0), ALIGN_DTYPE)
    n = C.c_size_t(0)
    rc = lib.vdf_align_windows_host(*args, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run), out.ctypes.data if out.size else None,
                                    out.size, C.byref(n))
    if rc != _capi.VDF_OK:
        raise VdfError(rc, "vdf_align_windows_host: bad argument")
    return out[:min(n.value, out.size)], int(n.value)


# one record of the align-variants calls (include/vdf.h: vdf_alignment_variant, 28 bytes)
ALIGN_VARIANT_DTYPE = np.dtype(ALIGN_DTYPE.descr + [("variant", "<u4")])


def _zero_arg(zero, hashes_arg_rows: int):
    """A zero plane beside its hashes, as the C ABI takes it (None stays NULL: the library says what is missing)."""
    if zero is None:
        return None
    z = np.ascontiguousarray(zero, dtype=np.uint64).reshape(-1, HASH_WORDS)
    if z.shape[0] != hashes_arg_rows:
        raise ValueError("one zero plane per window hash")
    return z


def _align_variants_host_args(a_hashes, a_zero, a_first, b_hashes, b_zero, b_first, a_skip, b_skip):
    """_align_host_args with the zero planes in their places: (a_hashes, a_zero, a_first, n_a, a_skip, b_hashes, b_zero, b_first, n_b, b_skip)."""
    keep, args = _align_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)
    az = _zero_arg(a_zero, keep[0].shape[0])
    bz = None if b_hashes is None else _zero_arg(b_zero, keep[3].shape[0])
    keep += [az, bz]
    # an empty plane must not read as a missing one: numpy gives an empty array a non-null address, ctypes turns 0 into NULL
    ptr = lambda z: None if z is None else (z.ctypes.data or keep[1].ctypes.data)
    return keep, [args[0], ptr(az), args[1], args[2], args[3], args[4], ptr(bz), args[5], args[6], args[7]]


def _variant_mask(variant_mask) -> int:
    return _align_uint32("variant_mask", variant_mask)


def align_windows_variants_host(a_hashes, a_first, a_zero=None, b_hashes=None, b_first=None, b_zero=None, tol_int: int = 350, min_run: int = 1,
                                variant_mask: int = 2, a_skip=None, b_skip=None, capacity: int = 1024):
    """vdf_align_windows_variants_host: align_windows_host against the variants of B named by variant_mask (bits 1 ... 7), in plain C++ on the
    CPU.  b_hashes None: self mode, B = A with a_zero.  -> (records [min(found, capacity)] of ALIGN_VARIANT_DTYPE in (variant, a, b) order, found)."""
    lib = _capi.load()
    keep, args = _align_variants_host_args(a_hashes, a_zero, a_first, b_hashes, b_zero, b_first, a_skip, b_skip)
    out = np.zeros(max(int(capacity), 0), ALIGN_VARIANT_DTYPE)
    n = C.c_size_t(0)
    rc = lib.vdf_align_windows_variants_host(*args, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run), _variant_mask(variant_mask),
                                             out.ctypes.data if out.size else None, out.size, C.byref(n))
    if rc != _capi.VDF_OK:
        raise VdfError(rc, "vdf_align_windows_variants_host: bad argument")
    return out[:min(n.value, out.size)], int(n.value)


# one record of the align-stretches calls (include/vdf.h: vdf_alignment_stretch, 28 bytes)
ALIGN_STRETCH_DTYPE = np.dtype(ALIGN_DTYPE.descr + [("rank", "<u4")])


def align_windows_stretches_host(a_hashes, a_first, b_hashes=None, b_first=None, tol_int: int = 350, min_run: int = 1, max_stretches: int = 4,
                                 guard: int = 0, a_skip=None, b_skip=None, capacity: int = 1024):
    """vdf_align_windows_stretches_host: every shared stretch of every pair - align_windows_host's record as rank 0, then the best run of the
    matrix with the rectangles of the earlier ranks (widened by guard) masked, up to max_stretches per pair - in plain C++ on the CPU.
    -> (records [min(found, capacity)] of ALIGN_STRETCH_DTYPE in (a, b, rank) order, found)."""
    lib = _capi.load()
    keep, args = _align_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)
    out = np.zeros(max(int(capacity), 0), ALIGN_STRETCH_DTYPE)
    n = C.c_size_t(0)
    rc = lib.vdf_align_windows_stretches_host(*args, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run),
                                              _align_uint32("max_stretches", max_stretches), _align_uint32("guard", guard),
                                              out.ctypes.data if out.size else None, out.size, C.byref(n))
    if rc != _capi.VDF_OK:
        raise VdfError(rc, "vdf_align_windows_stretches_host: bad argument")
    return out[:min(n.value, out.size)], int(n.value)


# one pair of videos (include/vdf.h: vdf_video_pair, 8 bytes): what the seed calls return and the *_pairs calls take
VIDEO_PAIR_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4")])


def video_pairs(pairs) -> np.ndarray:
    """A list of (a, b) - VIDEO_PAIR_DTYPE records, or anything numpy reads as [n, 2] integers - as the C ABI takes it."""
    p = np.asarray(pairs)
    if p.dtype == VIDEO_PAIR_DTYPE:
        return np.ascontiguousarray(p).reshape(-1)
    if p.size == 0:
        return np.zeros(0, VIDEO_PAIR_DTYPE)
    if p.dtype.kind not in "iu" or p.ndim != 2 or p.shape[1] != 2:
        raise ValueError("pairs: [n, 2] integers or VIDEO_PAIR_DTYPE records")
    if int(p.min()) < 0 or int(p.max()) >= 2**32:
        raise ValueError("pairs: video indices are 0 .. 2^32 - 1")
    out = np.zeros(len(p), VIDEO_PAIR_DTYPE)
    out["a"], out["b"] = p[:, 0], p[:, 1]
    return out


def pair_list_problem(pairs: np.ndarray, n_a: int, n_b: int, self_mode: bool):
    """What the *_pairs calls refuse in a list, in the library's order and words (include/vdf.h) - the first entry that breaks a rule, and of
    its rules the first; None: the list is fine.  The host forms have no context to keep the library's message in, and api.align checks the
    caller's whole list before it cuts it into blocks: both name the problem through this."""
    a, b = pairs["a"].astype(np.int64), pairs["b"].astype(np.int64)
    code = np.zeros(len(pairs), np.uint8)
    code[self_mode & (a >= b)] = 3
    code[(a >= n_a) | (b >= (n_a if self_mode else n_b))] = 2
    code[1:][(a[1:] < a[:-1]) | ((a[1:] == a[:-1]) & (b[1:] <= b[:-1]))] = 1
    bad = np.flatnonzero(code)
    if not bad.size:
        return None
    i = int(bad[0])
    return {1: f"the pair list is not strictly increasing in (a, b) at entry {i}", 2: f"pair {i} of the list names a video that does not exist",
            3: f"pair {i} of the list has a >= b in self mode"}[int(code[i])]


def _pairs_host_error(name: str, rc: int, pairs: np.ndarray, args, self_mode: bool):
    # the host forms have no context to keep a message in: the list's problem, if it has one, is named here
    return VdfError(rc, f"{name}: {pair_list_problem(pairs, args[2], args[6], self_mode) or 'bad argument'}")


def align_seed_pairs_host(a_hashes, a_first, b_hashes=None, b_first=None, tol_int: int = 350, min_run: int = 1, a_skip=None, b_skip=None,
                          capacity: int = 1024):
    """vdf_align_seed_pairs_host: the candidate pairs of the align calls - the pairs (a, b) with a matching cell (ka, kb), ka % min_run == 0 -
    in plain C++ on the CPU.  Every pair align_windows_host has a record for is among them.
    -> (pairs [min(found, capacity)] of VIDEO_PAIR_DTYPE in (a, b) order, found)."""
    lib = _capi.load()
    keep, args = _align_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)
    out = np.zeros(max(int(capacity), 0), VIDEO_PAIR_DTYPE)
    n = C.c_size_t(0)
    rc = lib.vdf_align_seed_pairs_host(*args, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run), out.ctypes.data if out.size else None,
                                       out.size, C.byref(n))
    if rc != _capi.VDF_OK:
        raise VdfError(rc, "vdf_align_seed_pairs_host: bad argument")
    return out[:min(n.value, out.size)], int(n.value)


def align_windows_pairs_host(a_hashes, a_first, pairs, b_hashes=None, b_first=None, tol_int: int = 350, min_run: int = 1, a_skip=None, b_skip=None,
                             capacity: int = 1024):
    """vdf_align_windows_pairs_host: align_windows_host on the listed pairs only (strictly increasing in (a, b); a < b in self mode).
    -> (records [min(found, capacity)] of ALIGN_DTYPE in (a, b) order, found)."""
    lib = _capi.load()
    keep, args = _align_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)
    p = video_pairs(pairs)
    out = np.zeros(max(int(capacity), 0), ALIGN_DTYPE)
    n = C.c_size_t(0)
    rc = lib.vdf_align_windows_pairs_host(*args, p.ctypes.data if p.size else None, p.size, _align_uint32("tol_int", tol_int),
                                          _align_uint32("min_run", min_run), out.ctypes.data if out.size else None, out.size, C.byref(n))
    if rc != _capi.VDF_OK:
        raise _pairs_host_error("vdf_align_windows_pairs_host", rc, p, args, b_hashes is None)
    return out[:min(n.value, out.size)], int(n.value)


def align_windows_stretches_pairs_host(a_hashes, a_first, pairs, b_hashes=None, b_first=None, tol_int: int = 350, min_run: int = 1,
                                       max_stretches: int = 4, guard: int = 0, a_skip=None, b_skip=None, capacity: int = 1024):
    """vdf_align_windows_stretches_pairs_host: align_windows_stretches_host on the listed pairs only.
    -> (records [min(found, capacity)] of ALIGN_STRETCH_DTYPE in (a, b, rank) order, found)."""
    lib = _capi.load()
    keep, args = _align_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)
    p = video_pairs(pairs)
    out = np.zeros(max(int(capacity), 0), ALIGN_STRETCH_DTYPE)
    n = C.c_size_t(0)
    rc = lib.vdf_align_windows_stretches_pairs_host(*args, p.ctypes.data if p.size else None, p.size, _align_uint32("tol_int", tol_int),
                                                    _align_uint32("min_run", min_run), _align_uint32("max_stretches", max_stretches),
                                                    _align_uint32("guard", guard), out.ctypes.data if out.size else None, out.size, C.byref(n))
    if rc != _capi.VDF_OK:
        raise _pairs_host_error("vdf_align_windows_stretches_pairs_host", rc, p, args, b_hashes is None)
    return out[:min(n.value, out.size)], int(n.value)


# one record of the retimed align calls (include/vdf.h: vdf_alignment_retimed, 24 bytes)
ALIGN_RETIMED_DTYPE = _capi.ALIGN_RETIMED_DTYPE


def _align_rate(rate):
    """(rate_num, rate_den) of a retimed align call as two uint32; the library says which rates it takes."""
    try:
        num, den = rate
    except (TypeError, ValueError):
        raise ValueError(f"rate must be a pair of integers (num, den), not {rate!r}") from None
    return _align_uint32("rate num", num), _align_uint32("rate den", den)


def _align_retimed_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip):
    if b_hashes is None or b_first is None:
        raise ValueError("the retimed align calls have no self mode: give b_hashes and b_first")
    return _align_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)


def align_windows_retimed_host(a_hashes, a_first, b_hashes, b_first, rate, tol_int: int = 350, min_run: int = 1, a_skip=None, b_skip=None,
                               capacity: int = 1024):
    """vdf_align_windows_retimed_host: the definition of the retimed align calls in plain C++ on the CPU (no context, no GPU).  a_hashes: RETIMED
    windows at stride 1 (hash_windows(..., rate=rate)), b_hashes: plain windows at stride 1; rate = (num, den), 1 <= den <= num <= 2 den, at most
    ALIGN_RETIMED_MAX_NUM in lowest terms.  -> (records [min(found, capacity)] of ALIGN_RETIMED_DTYPE in (a, b) order, found)."""
    lib = _capi.load()
    keep, args = _align_retimed_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)
    out = np.zeros(max(int(capacity), 0), ALIGN_RETIMED_DTYPE)
    n = C.c_size_t(0)
    rc = lib.vdf_align_windows_retimed_host(*args, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run), *_align_rate(rate),
                                            out.ctypes.data if out.size else None, out.size, C.byref(n))
    if rc != _capi.VDF_OK:
        raise VdfError(rc, "vdf_align_windows_retimed_host: bad argument")
    return out[:min(n.value, out.size)], int(n.value)


def align_windows_retimed_pairs_host(a_hashes, a_first, pairs, b_hashes, b_first, rate, tol_int: int = 350, min_run: int = 1, a_skip=None, b_skip=None,
                                     capacity: int = 1024):
    """vdf_align_windows_retimed_pairs_host: align_windows_retimed_host on the listed pairs only (strictly increasing in (a, b)).
    -> (records [min(found, capacity)] of ALIGN_RETIMED_DTYPE in (a, b) order, found)."""
    lib = _capi.load()
    keep, args = _align_retimed_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)
    p = video_pairs(pairs)
    out = np.zeros(max(int(capacity), 0), ALIGN_RETIMED_DTYPE)
    n = C.c_size_t(0)
    rc = lib.vdf_align_windows_retimed_pairs_host(*args, p.ctypes.data if p.size else None, p.size, _align_uint32("tol_int", tol_int),
                                                  _align_uint32("min_run", min_run), *_align_rate(rate), out.ctypes.data if out.size else None, out.size,
                                                  C.byref(n))
    if rc != _capi.VDF_OK:
        raise _pairs_host_error("vdf_align_windows_retimed_pairs_host", rc, p, args, False)
    return out[:min(n.value, out.size)], int(n.value)


# one (a, b, rate) triple of the seeded retimed call (include/vdf.h: vdf_video_pair_rate, 12 bytes); rate = the index into the call's list of rates
VIDEO_PAIR_RATE_DTYPE = _capi.VIDEO_PAIR_RATE_DTYPE


def _seed_rates_job(a_hashes, a_first, n_a, a_rate_first, a_skip, b_hashes, b_first, n_b, b_skip, rates, tol_int, min_run, exclude_same, capacity, stream=0):
    """(job, out, n, what the job points into): the job of vdf_align_seed_pairs_rates[_host|_device].  The array arguments are addresses (0 =
    NULL) - of host or of device memory, as the form takes them; rates and a_rate_first are host lists."""
    num, den = _align_rates(rates)
    rf = None if a_rate_first is None else np.ascontiguousarray(a_rate_first, dtype=np.uintp).reshape(-1)
    if rf is not None and rf.size < min(len(num), _capi.WINDOWS_MAX_RATES):
        raise ValueError("a_rate_first has an entry per rate")
    out = np.zeros(max(int(capacity), 0), VIDEO_PAIR_RATE_DTYPE)
    n = C.c_size_t(0)
    job = _capi.VdfAlignSeedRatesJob(a_hashes or None, a_first or None, rf.ctypes.data if rf is not None else None, a_skip or None, int(n_a), b_hashes or None,
                                     b_first or None, b_skip or None, int(n_b), len(num), num.ctypes.data if len(num) else None,
                                     den.ctypes.data if len(num) else None, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run),
                                     1 if exclude_same else 0, out.ctypes.data if out.size else None, out.size, C.pointer(n), stream or None)
    return job, out, n, (num, den, rf)


def _align_rates(rates):
    """A list of rates of an align call as two uint32 arrays; the library says how many there may be and which it takes."""
    pairs = [_align_rate(r) for r in rates]
    return np.array([p[0] for p in pairs], np.uint32), np.array([p[1] for p in pairs], np.uint32)


def _seed_rates_host_args(a_hashes, a_first, a_rate_first, a_skip, b_hashes, b_first, b_skip, n_rates):
    """The host arrays of a seeded retimed call: A rate-major - hashes [rows, 16], first [n_rates, n_a + 1], rate_first [n_rates (+ 1)] or None
    (zeros), skip [rows] or None - and B as the align calls take it.  Returns the arrays (to keep alive) and their addresses and counts."""
    ah = np.ascontiguousarray(a_hashes, dtype=np.uint64).reshape(-1, HASH_WORDS)
    af = np.ascontiguousarray(a_first, dtype=np.uint32)
    if af.ndim != 2 or af.shape[1] == 0 or af.shape[0] < min(int(n_rates), _capi.WINDOWS_MAX_RATES):
        raise ValueError("a_first has one row of n_a + 1 entries per rate")
    rf = np.zeros(af.shape[0], np.int64) if a_rate_first is None else np.asarray(a_rate_first, dtype=np.int64).reshape(-1)[:af.shape[0]]
    if rf.size < af.shape[0] or (af.size and int((rf[:, None] + af).max()) > ah.shape[0]):
        raise ValueError("a first array points behind its hashes")
    ak = None
    if a_skip is not None:
        ak = np.ascontiguousarray(a_skip, dtype=np.uint8).reshape(-1)
        if ak.size != ah.shape[0]:
            raise ValueError("one skip byte per window")
    if b_hashes is None or b_first is None:
        raise ValueError("the seeded retimed call has no self mode: give b_hashes and b_first")
    bh = np.ascontiguousarray(b_hashes, dtype=np.uint64).reshape(-1, HASH_WORDS)
    bf = np.ascontiguousarray(b_first, dtype=np.uint32).reshape(-1)
    if bf.size == 0:
        raise ValueError("a first array has n_videos + 1 entries")
    if int(bf.max()) > bh.shape[0]:
        raise ValueError("a first array points behind its hashes")
    bk = None
    if b_skip is not None:
        bk = np.ascontiguousarray(b_skip, dtype=np.uint8).reshape(-1)
        if bk.size != bh.shape[0]:
            raise ValueError("one skip byte per window")
    # an empty side must not read as a null pointer: numpy gives an empty array a non-null address
    args = dict(a_hashes=ah.ctypes.data or af.ctypes.data, a_first=af.ctypes.data, n_a=af.shape[1] - 1, a_skip=ak.ctypes.data if ak is not None else 0,
                b_hashes=bh.ctypes.data or bf.ctypes.data, b_first=bf.ctypes.data, n_b=bf.size - 1, b_skip=bk.ctypes.data if bk is not None else 0)
    return (ah, af, ak, bh, bf, bk), args


def align_seed_pairs_rates_host(a_hashes, a_first, b_hashes, b_first, rates, tol_int: int = 350, min_run: int = 1, a_rate_first=None, a_skip=None,
                                b_skip=None, exclude_same: bool = False, capacity: int = 1024):
    """vdf_align_seed_pairs_rates_host: which pairs (a, b) can have a record of align_windows_retimed at which rate of `rates` - the definition in
    plain C++ on the CPU.  A is RATE-MAJOR, as Engine.hash_windows_clips_rates writes it: a_hashes [rows, 16], a_first [n_rates, n_a + 1],
    a_rate_first [n_rates (+ 1)] (None: zeros); window k of video i at rate r is row a_rate_first[r] + a_first[r, i] + k.  B: plain windows.
    -> (triples [min(found, capacity)] of VIDEO_PAIR_RATE_DTYPE in (rate, a, b) order - rate is the index into `rates` - and found)."""
    keep, args = _seed_rates_host_args(a_hashes, a_first, a_rate_first, a_skip, b_hashes, b_first, b_skip, len(rates))
    job, out, n, keep2 = _seed_rates_job(rates=rates, a_rate_first=a_rate_first, tol_int=tol_int, min_run=min_run, exclude_same=exclude_same, capacity=capacity,
                                         **args)
    rc = _capi.load().vdf_align_seed_pairs_rates_host(C.byref(job))
    if rc != _capi.VDF_OK:
        raise VdfError(rc, "vdf_align_seed_pairs_rates_host: bad argument")
    return out[:min(n.value, out.size)], int(n.value)


# one record of the align call over (rate, a, b) triples (include/vdf.h: vdf_alignment_rate, 32 bytes)
ALIGN_RATE_DTYPE = _capi.ALIGN_RATE_DTYPE


def video_pair_rates(triples) -> np.ndarray:
    """A list of (rate, a, b) - VIDEO_PAIR_RATE_DTYPE records (what the seeded retimed call returns), or anything numpy reads as [n, 3] integers in
    that order - as the C ABI takes it."""
    if isinstance(triples, np.ndarray) and triples.dtype == VIDEO_PAIR_RATE_DTYPE:
        return np.ascontiguousarray(triples).reshape(-1)
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    if t.size and (t.min() < 0 or t.max() > 0xFFFFFFFF):
        raise ValueError("rate and video indices are unsigned 32-bit")
    out = np.zeros(len(t), VIDEO_PAIR_RATE_DTYPE)
    out["rate"], out["a"], out["b"] = t[:, 0], t[:, 1], t[:, 2]
    return out


def _align_rates_job(a_hashes, a_first, n_a, a_rate_first, a_skip, b_hashes, b_first, n_b, b_skip, rates, tol_int, min_run, triples, seed, exclude_same,
                     capacity, stream=0):
    """(job, out, n, what the job points into): the job of vdf_align_windows_rates[_host|_device].  The array arguments are addresses (0 = NULL) -
    of host or of device memory, as the form takes them; rates, a_rate_first and triples (None: no list) are host data."""
    num, den = _align_rates(rates)
    rf = None if a_rate_first is None else np.ascontiguousarray(a_rate_first, dtype=np.uintp).reshape(-1)
    if rf is not None and rf.size < min(len(num), _capi.WINDOWS_MAX_RATES):
        raise ValueError("a_rate_first has an entry per rate")
    t = None if triples is None else video_pair_rates(triples)
    out = np.zeros(max(int(capacity), 0), ALIGN_RATE_DTYPE)
    n = C.c_size_t(0)
    # an empty list must not read as "no list": numpy gives an empty array a non-null address
    job = _capi.VdfAlignRatesJob(a_hashes or None, a_first or None, rf.ctypes.data if rf is not None else None, a_skip or None, int(n_a), b_hashes or None,
                                 b_first or None, b_skip or None, int(n_b), len(num), num.ctypes.data if len(num) else None,
                                 den.ctypes.data if len(num) else None, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run),
                                 None if t is None else (t.ctypes.data or out.ctypes.data or num.ctypes.data), 0 if t is None else t.size, 1 if seed else 0,
                                 1 if exclude_same else 0, out.ctypes.data if out.size else None, out.size, C.pointer(n), stream or None)
    return job, out, n, (num, den, rf, t)


def align_windows_rates_host(a_hashes, a_first, b_hashes, b_first, rates, tol_int: int = 350, min_run: int = 1, a_rate_first=None, a_skip=None, b_skip=None,
                             triples=None, seed: bool = False, exclude_same: bool = False, capacity: int = 1024):
    """vdf_align_windows_rates_host: the retimed alignment at every rate of `rates` in one call - the definition in plain C++ on the CPU.  A is
    RATE-MAJOR as align_seed_pairs_rates_host takes it, B plain windows.  triples: only these (rate, a, b) are walked (strictly increasing;
    what align_seed_pairs_rates returns goes in unchanged); None: all of them - without a == b under exclude_same - or, with seed=True, the
    candidates of the seed call, found inside the call: the same records.
    -> (records [min(found, capacity)] of ALIGN_RATE_DTYPE in (rate, a, b) order - rate is the index into `rates` - and found)."""
    keep, args = _seed_rates_host_args(a_hashes, a_first, a_rate_first, a_skip, b_hashes, b_first, b_skip, len(rates))
    job, out, n, keep2 = _align_rates_job(rates=rates, a_rate_first=a_rate_first, tol_int=tol_int, min_run=min_run, triples=triples, seed=seed,
                                          exclude_same=exclude_same, capacity=capacity, **args)
    rc = _capi.load().vdf_align_windows_rates_host(C.byref(job))
    if rc != _capi.VDF_OK:
        raise VdfError(rc, "vdf_align_windows_rates_host: bad argument")
    return out[:min(n.value, out.size)], int(n.value)


# one record of the stretches call over (rate, a, b) triples (include/vdf.h: vdf_alignment_rate_stretch, 36 bytes)
ALIGN_RATE_STRETCH_DTYPE = _capi.ALIGN_RATE_STRETCH_DTYPE


def _align_rates_stretches_job(a_hashes, a_first, n_a, a_rate_first, a_skip, b_hashes, b_first, n_b, b_skip, rates, tol_int, min_run, triples, seed, exclude_same,
                               max_stretches, guard, capacity, stream=0):
    """(job, out, n, what the job points into): the job of vdf_align_windows_rates_stretches[_host|_device] - _align_rates_job with max_stretches, guard
    and the 36-byte records."""
    num, den = _align_rates(rates)
    rf = None if a_rate_first is None else np.ascontiguousarray(a_rate_first, dtype=np.uintp).reshape(-1)
    if rf is not None and rf.size < min(len(num), _capi.WINDOWS_MAX_RATES):
        raise ValueError("a_rate_first has an entry per rate")
    t = None if triples is None else video_pair_rates(triples)
    out = np.zeros(max(int(capacity), 0), ALIGN_RATE_STRETCH_DTYPE)
    n = C.c_size_t(0)
    # an empty list must not read as "no list": numpy gives an empty array a non-null address
    job = _capi.VdfAlignRatesStretchesJob(a_hashes or None, a_first or None, rf.ctypes.data if rf is not None else None, a_skip or None, int(n_a), b_hashes or None,
                                          b_first or None, b_skip or None, int(n_b), len(num), num.ctypes.data if len(num) else None,
                                          den.ctypes.data if len(num) else None, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run),
                                          None if t is None else (t.ctypes.data or out.ctypes.data or num.ctypes.data), 0 if t is None else t.size,
                                          1 if seed else 0, 1 if exclude_same else 0, _align_uint32("max_stretches", max_stretches), _align_uint32("guard", guard),
                                          out.ctypes.data if out.size else None, out.size, C.pointer(n), stream or None)
    return job, out, n, (num, den, rf, t)


def align_windows_rates_stretches_host(a_hashes, a_first, b_hashes, b_first, rates, tol_int: int = 350, min_run: int = 1, max_stretches: int = 4, guard: int = 15,
                                       a_rate_first=None, a_skip=None, b_skip=None, triples=None, seed: bool = False, exclude_same: bool = False,
                                       capacity: int = 1024):
    """vdf_align_windows_rates_stretches_host: EVERY stretch of every (rate, a, b) triple, ranked - align_windows_rates_host's record as rank 0, then per
    rank the best record of the triple's matrix with the rectangles of the ranks before it masked, in the rows of the two videos and so in every
    phase; guard counts rows of B.  The definition in plain C++ on the CPU; arguments as align_windows_rates_host.
    -> (records [min(found, capacity)] of ALIGN_RATE_STRETCH_DTYPE in (rate, a, b, rank) order, and found)."""
    keep, args = _seed_rates_host_args(a_hashes, a_first, a_rate_first, a_skip, b_hashes, b_first, b_skip, len(rates))
    job, out, n, keep2 = _align_rates_stretches_job(rates=rates, a_rate_first=a_rate_first, tol_int=tol_int, min_run=min_run, triples=triples, seed=seed,
                                                    exclude_same=exclude_same, max_stretches=max_stretches, guard=guard, capacity=capacity, **args)
    rc = _capi.load().vdf_align_windows_rates_stretches_host(C.byref(job))
    if rc != _capi.VDF_OK:
        raise VdfError(rc, "vdf_align_windows_rates_stretches_host: bad argument")
    return out[:min(n.value, out.size)], int(n.value)


# one (variant, a, b) triple (include/vdf.h: vdf_video_pair_variant, 12 bytes): what the seeded variants call returns and the variants-pairs calls take
VIDEO_PAIR_VARIANT_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("variant", "<u4")])


def video_pair_variants(triples) -> np.ndarray:
    """A list of (variant, a, b) - VIDEO_PAIR_VARIANT_DTYPE records, or anything numpy reads as [n, 3] integers in that order - as the C ABI
    takes it."""
    t = np.asarray(triples)
    if t.dtype == VIDEO_PAIR_VARIANT_DTYPE:
        return np.ascontiguousarray(t).reshape(-1)
    if t.size == 0:
        return np.zeros(0, VIDEO_PAIR_VARIANT_DTYPE)
    if t.dtype.kind not in "iu" or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("triples: [n, 3] integers (variant, a, b) or VIDEO_PAIR_VARIANT_DTYPE records")
    if int(t.min()) < 0 or int(t.max()) >= 2**32:
        raise ValueError("triples: variants and video indices are 0 .. 2^32 - 1")
    out = np.zeros(len(t), VIDEO_PAIR_VARIANT_DTYPE)
    out["variant"], out["a"], out["b"] = t[:, 0], t[:, 1], t[:, 2]
    return out


def triple_list_problem(triples: np.ndarray, n_a: int, n_b: int, self_mode: bool):
    """What vdf_align_windows_variants_pairs* refuses in a list, in the library's order and words - the first entry that breaks a rule, and of
    its rules the first; None: the list is fine (pair_list_problem's twin for triples)."""
    v, a, b = (triples[k].astype(np.int64) for k in ("variant", "a", "b"))
    code = np.zeros(len(triples), np.uint8)
    code[self_mode & (a >= b)] = 3
    code[(a >= n_a) | (b >= (n_a if self_mode else n_b))] = 2
    code[(v < 1) | (v > 7)] = 4
    key = (v[1:] < v[:-1]) | ((v[1:] == v[:-1]) & ((a[1:] < a[:-1]) | ((a[1:] == a[:-1]) & (b[1:] <= b[:-1]))))
    code[1:][key] = 1
    bad = np.flatnonzero(code)
    if not bad.size:
        return None
    i = int(bad[0])
    return {1: f"the triple list is not strictly increasing in (variant, a, b) at entry {i}", 4: f"triple {i} of the list has a variant outside 1 ... 7",
            2: f"triple {i} of the list names a video that does not exist", 3: f"triple {i} of the list has a >= b in self mode"}[int(code[i])]


def align_seed_pairs_variants_host(a_hashes, a_first, a_zero=None, b_hashes=None, b_first=None, b_zero=None, tol_int: int = 350, min_run: int = 1,
                                   variant_mask: int = 2, a_skip=None, b_skip=None, capacity: int = 1024):
    """vdf_align_seed_pairs_variants_host: per variant of variant_mask (bits 1 ... 7) the candidate pairs of align_seed_pairs_host on (A, the
    variant set of B), in plain C++ on the CPU.  -> (triples [min(found, capacity)] of VIDEO_PAIR_VARIANT_DTYPE in (variant, a, b) order, found)."""
    lib = _capi.load()
    keep, args = _align_variants_host_args(a_hashes, a_zero, a_first, b_hashes, b_zero, b_first, a_skip, b_skip)  # keep: holds the arrays alive over the call
    out = np.zeros(max(int(capacity), 0), VIDEO_PAIR_VARIANT_DTYPE)
    n = C.c_size_t(0)
    rc = lib.vdf_align_seed_pairs_variants_host(*args, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run), _variant_mask(variant_mask),
                                                out.ctypes.data if out.size else None, out.size, C.byref(n))
    if rc != _capi.VDF_OK:
        raise VdfError(rc, "vdf_align_seed_pairs_variants_host: bad argument")
    return out[:min(n.value, out.size)], int(n.value)


def align_windows_variants_pairs_host(a_hashes, a_first, triples, a_zero=None, b_hashes=None, b_first=None, b_zero=None, tol_int: int = 350,
                                      min_run: int = 1, a_skip=None, b_skip=None, capacity: int = 1024):
    """vdf_align_windows_variants_pairs_host: align_windows_variants_host on the listed (variant, a, b) triples only (strictly increasing).
    -> (records [min(found, capacity)] of ALIGN_VARIANT_DTYPE in (variant, a, b) order, found)."""
    lib = _capi.load()
    keep, args = _align_variants_host_args(a_hashes, a_zero, a_first, b_hashes, b_zero, b_first, a_skip, b_skip)  # keep: holds the arrays alive over the call
    t = video_pair_variants(triples)
    out = np.zeros(max(int(capacity), 0), ALIGN_VARIANT_DTYPE)
    n = C.c_size_t(0)
    rc = lib.vdf_align_windows_variants_pairs_host(*args, t.ctypes.data if t.size else None, t.size, _align_uint32("tol_int", tol_int),
                                                   _align_uint32("min_run", min_run), out.ctypes.data if out.size else None, out.size, C.byref(n))
    if rc != _capi.VDF_OK:
        raise VdfError(rc, f"vdf_align_windows_variants_pairs_host: {triple_list_problem(t, args[3], args[8], b_hashes is None) or 'bad argument'}")
    return out[:min(n.value, out.size)], int(n.value)


CLASS_SEED_DWORDS, CLASS_ROW_DWORDS = 36, 72   # a seed / a row of B in the class-major layout (include/vdf.h: vdf_window_class_layout_*)


def window_class_layout_host(hashes, first, zero=None, skip=None, min_run: int = 1) -> np.ndarray:
    """vdf_window_class_layout_host: the class-major rows the seeded flipped alignment reads, on the CPU.  zero None: the seeds of the set at
    min_run, [n_seeds, 36] u32; otherwise its rows with their planes, [n_rows, 72] u32."""
    lib = _capi.load()
    h = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1, HASH_WORDS)
    f = np.ascontiguousarray(first, dtype=np.uint32)
    z = _zero_arg(zero, h.shape[0])
    sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8)
    width = CLASS_SEED_DWORDS if z is None else CLASS_ROW_DWORDS
    out = np.zeros((max(len(h), 1), width), np.uint32)
    n = C.c_size_t(0)
    rc = lib.vdf_window_class_layout_host(h.ctypes.data or f.ctypes.data, None if z is None else (z.ctypes.data or f.ctypes.data), f.ctypes.data, len(f) - 1,
                                          None if sk is None else sk.ctypes.data, _align_uint32("min_run", min_run), out.ctypes.data, len(out), C.byref(n))
    if rc != _capi.VDF_OK:
        raise VdfError(rc, "vdf_window_class_layout_host: bad argument")
    return out[:n.value]


def window_variants_host(hashes, zero, first, variant: int, skip=None):
    """vdf_window_variants_host: the variant of a set of window hashes (hashes / zero [windows, 16] u64, first [videos + 1]) on the CPU ->
    hashes [windows, 16] (and the skip bytes carried along, if skip is given).  Rows outside [first[0], first[-1]) come back zero."""
    lib = _capi.load()
    h = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1, HASH_WORDS)
    z = np.ascontiguousarray(zero, dtype=np.uint64).reshape(-1, HASH_WORDS)
    f = np.ascontiguousarray(first, dtype=np.uint32).reshape(-1)
    if f.size == 0 or z.shape != h.shape or int(f.max()) > h.shape[0]:
        raise ValueError("hashes and zero [windows, 16], first [videos + 1] within them")
    k = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8).reshape(-1)
    if k is not None and k.size != h.shape[0]:
        raise ValueError("one skip byte per window")
    rows = h.shape[0]
    if rows == 0:  # videos without windows: numpy gives an empty array a null address, which the library takes for a missing argument
        h, z, k = np.zeros((1, HASH_WORDS), np.uint64), np.zeros((1, HASH_WORDS), np.uint64), None if k is None else np.zeros(1, np.uint8)
    out = np.zeros_like(h)
    out_k = None if k is None else np.zeros_like(k)
    rc = lib.vdf_window_variants_host(h.ctypes.data, z.ctypes.data, f.ctypes.data, f.size - 1, None if k is None else k.ctypes.data,
                                      _align_uint32("variant", variant), out.ctypes.data, None if k is None else out_k.ctypes.data)
    if rc != _capi.VDF_OK:
        raise VdfError(rc, "vdf_window_variants_host: bad argument")
    out = out[:rows]
    out_k = None if k is None else out_k[:rows]
    return out if k is None else (out, out_k)


class Engine:
    """One context: one GPU (`device`, default LOCAL_RANK or 0), or - `devices=[...]` - ONE context over several GPUs
    of the node (vdf_ctx_create_multi: the host-array calls fan out inside the library, the *_shards methods take
    one device pointer per GPU).  A device may be listed twice to exercise the multi-GPU path on one GPU.

    *_device methods take raw device pointers and a hipStream_t handle (single-GPU contexts only).  stream=0 means the
    context's own non-blocking stream, which does NOT order against work queued elsewhere (e.g. torch's current
    stream): either pass the stream that produced the buffers, or synchronise before the call."""

    def __init__(self, device: Optional[int] = None, devices: Optional[Sequence[int]] = None):
        self.lib = _capi.load()
        ctx = C.c_void_p()
        if devices is not None:
            devs = [int(d) for d in devices]
            arr = (C.c_int * len(devs))(*devs)
            rc = self.lib.vdf_ctx_create_multi(arr, len(devs), C.byref(ctx))
            device = devs[0] if devs else 0
        else:
            if device is None:
                device = int(os.environ.get("LOCAL_RANK", "0"))
            rc = self.lib.vdf_ctx_create(int(device), C.byref(ctx))
        if rc != _capi.VDF_OK:
            msg = self.lib.vdf_last_error(None)
            raise VdfError(rc, (msg or b"").decode() or "vdf_ctx_create failed (is a GPU visible?)")
        self.ctx = ctx
        # the library read VDF_NO_HIT_FILTER when the context was made: without the filter a replay launch makes no exchange calls
        self.hit_filter_enabled = _atoi(os.environ.get("VDF_NO_HIT_FILTER", "0")) == 0
        self.device = int(device)
        self.n_devices = int(self.lib.vdf_ctx_device_count(ctx))
        self.devices = [int(self.lib.vdf_ctx_device_at(ctx, k)) for k in range(self.n_devices)]

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.vdf_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _hit_buffer(self, capacity: int) -> np.ndarray:
        """Reusable host staging buffer for hit lists (a fresh 32 MB allocation per call costs ~10 ms)."""
        buf = getattr(self, "_hits", None)
        if buf is None or buf.shape[0] < max(capacity, 1):
            buf = np.empty((max(capacity, 1), 2), np.uint32)
            self._hits = buf
        return buf

    def _check(self, rc: int):
        if rc != _capi.VDF_OK:
            raise VdfError(rc, (self.lib.vdf_last_error(self.ctx) or b"").decode())

    def set_hit_capacity(self, capacity: int):
        self._check(self.lib.vdf_ctx_set_hit_capacity(self.ctx, int(capacity)))

    def last_stats(self) -> dict:
        s = VdfSearchStats()
        self._check(self.lib.vdf_ctx_last_search_stats(self.ctx, C.byref(s)))
        return {k: getattr(s, k) for k, _ in VdfSearchStats._fields_}

    def last_timing(self) -> dict:
        """Where the time of the last search call went (vdf_search_timing: ms per phase, suspect-queue fill)."""
        t = VdfSearchTiming()
        self._check(self.lib.vdf_ctx_last_search_timing(self.ctx, C.byref(t)))
        return {k: getattr(t, k) for k, _ in VdfSearchTiming._fields_}

    def device_stats(self, slot: int) -> dict:
        s = VdfSearchStats()
        self._check(self.lib.vdf_ctx_device_search_stats(self.ctx, int(slot), C.byref(s)))
        return {k: getattr(s, k) for k, _ in VdfSearchStats._fields_}

    def rccl_ranks(self) -> int:
        """RCCL communicators (one per GPU) this context has initialised (0: every replication so far was plain device copies)."""
        return int(self.lib.vdf_ctx_rccl_ranks(self.ctx))

    def device_timing(self, slot: int) -> dict:
        t = VdfSearchTiming()
        self._check(self.lib.vdf_ctx_device_search_timing(self.ctx, int(slot), C.byref(t)))
        return {k: getattr(t, k) for k, _ in VdfSearchTiming._fields_}

    # ------------------------------------------------------- multi-GPU contexts: device-resident shards
    def search_self_shards(self, d_hash_shards: Sequence[int], d_dur_shards: Sequence[int], shard_n: Sequence[int],
                           tol_int: int, as_arrays: bool = False):
        """search() over a sorted database cut into consecutive shards, shard k resident on the GPU of slot k (device
        pointers); the library replicates it with one all-gather (RCCL over xGMI) and searches on all GPUs.
        as_arrays: the CSR form (offsets, members) instead of Python lists (100 k members cost 2 ms to convert)."""
        g = VdfGroups()
        self._check(self.lib.vdf_search_self_shards(self.ctx, _ptr_array(d_hash_shards), _ptr_array(d_dur_shards),
                                                    _size_array(shard_n), int(tol_int), C.byref(g)))
        try:
            if as_arrays:
                return groups_to_arrays(g)[:2]
            return [m for _, m in _groups_to_lists(g)]
        finally:
            self.lib.vdf_groups_free(C.byref(g))

    def search_refs_shards(self, d_cand_hash_shards, d_cand_dur_shards, cand_shard_n, d_ref_hash_shards, d_ref_dur_shards,
                           ref_shard_n, tol_int: int):
        g = VdfGroups()
        self._check(self.lib.vdf_search_refs_shards(self.ctx, _ptr_array(d_cand_hash_shards), _ptr_array(d_cand_dur_shards),
                                                    _size_array(cand_shard_n), _ptr_array(d_ref_hash_shards),
                                                    _ptr_array(d_ref_dur_shards), _size_array(ref_shard_n), int(tol_int),
                                                    C.byref(g)))
        try:
            return _groups_to_lists(g)
        finally:
            self.lib.vdf_groups_free(C.byref(g))

    def hash_frames_shards(self, d_frames: Sequence[int], n_clips: Sequence[int], frames_per_clip: int, w: int, h: int,
                           d_out: Sequence[int], d_dontcare: Optional[Sequence[int]] = None):
        fs = w * h
        self._check(self.lib.vdf_hash_frames_u8_shards(self.ctx, _ptr_array(d_frames), _size_array(n_clips), frames_per_clip,
                                                       w, h, fs, fs * frames_per_clip, _ptr_array(d_out),
                                                       _ptr_array(d_dontcare) if d_dontcare is not None else None))

    # ------------------------------------------------------------------ hashing
    def hash_frames(self, frames: np.ndarray, want_dontcare: bool = False):
        """frames [n_clips, n_frames, H, W] u8 (host) -> hashes [n_clips, 16] u64.
        Raises VdfError(VDF_E_NOT_ENOUGH_FRAMES) when n_frames < 16 (video_hash.rs:53,61)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim != 4:
            raise ValueError("frames must be [n_clips, n_frames, H, W]")
        nc, nf, h, w = frames.shape
        out = np.zeros((nc, HASH_WORDS), np.uint64)
        dc = np.zeros(nc, np.uint32) if want_dontcare else None
        rc = self.lib.vdf_hash_frames_u8(self.ctx, frames.ctypes.data, nc, nf, w, h, w * h, nf * w * h,
                                         out.ctypes.data, dc.ctypes.data if want_dontcare else None)
        self._check(rc)
        return (out, dc) if want_dontcare else out

    def hash_frames_device(self, d_frames: int, n_clips: int, frames_per_clip: int, w: int, h: int, d_out: int,
                           d_dontcare: int = 0, frame_stride: Optional[int] = None,
                           clip_stride: Optional[int] = None, stream: int = 0):
        fs = w * h if frame_stride is None else frame_stride
        cs = fs * frames_per_clip if clip_stride is None else clip_stride
        self._check(self.lib.vdf_hash_frames_u8_device(self.ctx, d_frames, n_clips, frames_per_clip, w, h, fs, cs,
                                                       d_out, d_dontcare or None, stream or None))

    # --------------------------------------------- every 16-frame window of a clip (include/vdf.h)
    def hash_windows(self, frames: np.ndarray, stride: int = 1, want_dontcare: bool = False):
        """frames [n_clips, n_frames, H, W] u8 (host) -> hashes [n_clips, n_win, 16] u64: window k = frames [k * stride, k * stride + 16),
        n_win = (n_frames - 16) // stride + 1; every frame is read, resized and spatially transformed once (vdf_hash_windows_u8)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim != 4:
            raise ValueError("frames must be [n_clips, n_frames, H, W]")
        nc, nf, h, w = frames.shape
        stride = _window_stride(stride)
        n_win = int(self.lib.vdf_hash_window_count(nf, stride))
        out = np.zeros((nc, n_win, HASH_WORDS), np.uint64)
        dc = np.zeros((nc, n_win), np.uint32) if want_dontcare else None
        self._check(self.lib.vdf_hash_windows_u8(self.ctx, frames.ctypes.data, nc, nf, w, h, w * h, nf * w * h, stride, out.ctypes.data,
                                                 dc.ctypes.data if want_dontcare else None))
        return (out, dc) if want_dontcare else out

    def hash_windows_device(self, d_frames: int, n_clips: int, frames_per_clip: int, w: int, h: int, stride: int, d_out: int,
                            d_dontcare: int = 0, frame_stride: Optional[int] = None, clip_stride: Optional[int] = None, stream: int = 0):
        """d_out: n_clips x n_win x 16 words (window_count(frames_per_clip, stride) windows per clip); all frames_per_clip frames are used."""
        stride = _window_stride(stride)
        fs = w * h if frame_stride is None else frame_stride
        cs = fs * frames_per_clip if clip_stride is None else clip_stride
        self._check(self.lib.vdf_hash_windows_u8_device(self.ctx, d_frames, n_clips, frames_per_clip, w, h, fs, cs, stride, d_out,
                                                        d_dontcare or None, stream or None))

    # --------------------------------------------- retimed windows: a copy at another frame rate or speed (include/vdf.h)
    def hash_windows_retimed(self, frames: np.ndarray, rate, stride: int = 1, want_dontcare: bool = False):
        """hash_windows at rate = (num, den), 1 <= den <= num <= 2 den: window k = the 16 frames k * stride + (i * num) // den, i = 0 .. 15,
        n_win = (n_frames - span) // stride + 1 with span = (15 * num) // den + 1 (vdf_hash_windows_u8_retimed).  If B[j] = A[c + (j * num) // den],
        window c + num * m of A at this rate is the plain window den * m of B.  Retime the side with more frames per second."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim != 4:
            raise ValueError("frames must be [n_clips, n_frames, H, W]")
        nc, nf, h, w = frames.shape
        stride = _window_stride(stride)
        num, den = _window_rate(rate)
        n_win = int(self.lib.vdf_hash_window_count_retimed(nf, stride, num, den))
        out = np.zeros((nc, n_win, HASH_WORDS), np.uint64)
        dc = np.zeros((nc, n_win), np.uint32) if want_dontcare else None
        self._check(self.lib.vdf_hash_windows_u8_retimed(self.ctx, frames.ctypes.data, nc, nf, w, h, w * h, nf * w * h, stride, num, den,
                                                         out.ctypes.data, dc.ctypes.data if want_dontcare else None))
        return (out, dc) if want_dontcare else out

    def hash_windows_retimed_device(self, d_frames: int, n_clips: int, frames_per_clip: int, w: int, h: int, stride: int, rate, d_out: int,
                                    d_dontcare: int = 0, frame_stride: Optional[int] = None, clip_stride: Optional[int] = None, stream: int = 0):
        """d_out: n_clips x n_win x 16 words (vdf_hash_window_count_retimed windows per clip); all frames_per_clip frames are used."""
        stride = _window_stride(stride)
        num, den = _window_rate(rate)
        fs = w * h if frame_stride is None else frame_stride
        cs = fs * frames_per_clip if clip_stride is None else clip_stride
        self._check(self.lib.vdf_hash_windows_u8_retimed_device(self.ctx, d_frames, n_clips, frames_per_clip, w, h, fs, cs, stride, num, den, d_out,
                                                                d_dontcare or None, stream or None))

    # --------------------------------------------- retimed windows at several rates from one read of the frames (include/vdf.h)
    def _windows_rates_job(self, frames_ptr, n_clips, frames_per_clip, w, h, fs, cs, stride, rates, out_ptr, dc_ptr, stream):
        """(job, arrays it points to): the caller keeps the arrays alive until the call has returned"""
        num, den = _window_rates(rates)
        job = _capi.VdfWindowsRatesJob(frames_ptr or None, n_clips, frames_per_clip, w, h, fs, cs, _window_stride(stride), len(num), num.ctypes.data,
                                       den.ctypes.data, out_ptr or None, dc_ptr or None, stream or None)
        return job, (num, den)

    def hash_windows_rates(self, frames: np.ndarray, rates, stride: int = 1, dontcare: bool = False):
        """hash_windows_retimed at up to 8 rates [(num, den), ...] from ONE upload, one resize and one spatial transform of the frames
        (vdf_hash_windows_u8_rates) -> a list with one [n_clips, n_win_r, 16] u64 array per listed rate - word for word what
        hash_windows_retimed(frames, rate, stride) gives; (1, 1) gives the plain windows - and, with dontcare, a second list with the
        [n_clips, n_win_r] u32 don't-care counts."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim != 4:
            raise ValueError("frames must be [n_clips, n_frames, H, W]")
        nc, nf, h, w = frames.shape
        total, first = hash_window_count_rates(nc, nf, stride, rates)
        out = np.zeros((total, HASH_WORDS), np.uint64)
        dc = np.zeros(total, np.uint32) if dontcare else None
        job, keep = self._windows_rates_job(frames.ctypes.data, nc, nf, w, h, w * h, nf * w * h, stride, rates, out.ctypes.data,
                                            dc.ctypes.data if dontcare else 0, 0)
        self._check(self.lib.vdf_hash_windows_u8_rates(self.ctx, C.byref(job)))
        del keep
        cut = lambda a, tail: [a[first[r]:first[r + 1]].reshape((nc, -1) + tail) if nc else a[:0].reshape((0, 0) + tail) for r in range(len(first) - 1)]
        return (cut(out, (HASH_WORDS,)), cut(dc, ())) if dontcare else cut(out, (HASH_WORDS,))

    def hash_windows_rates_device(self, d_frames: int, n_clips: int, frames_per_clip: int, w: int, h: int, stride: int, rates, d_out: int,
                                  d_dontcare: int = 0, frame_stride: Optional[int] = None, clip_stride: Optional[int] = None, stream: int = 0):
        """The device form (vdf_hash_windows_u8_rates_device), ordered on `stream`.  d_out: 16 words for each of the rows
        hash_window_count_rates(n_clips, frames_per_clip, stride, rates) counts, rate-major; d_dontcare (optional): one u32 per row.
        -> first [n_rates + 1]: rows first[r] ... first[r + 1] are rate r's block, a [n_clips, n_win_r, 16] array in d_out."""
        fs = w * h if frame_stride is None else frame_stride
        cs = fs * frames_per_clip if clip_stride is None else clip_stride
        job, keep = self._windows_rates_job(d_frames, n_clips, frames_per_clip, w, h, fs, cs, stride, rates, d_out, d_dontcare, stream)
        self._check(self.lib.vdf_hash_windows_u8_rates_device(self.ctx, C.byref(job)))
        del keep
        return hash_window_count_rates(n_clips, frames_per_clip, stride, rates)[1]

    def hash_windows_planes(self, frames: np.ndarray, stride: int = 1, want_dontcare: bool = False):
        """hash_windows plus the zero plane of every window (vdf_hash_windows_u8_planes): -> (hashes [n_clips, n_win, 16] u64, zero
        [n_clips, n_win, 16] u64 [, dontcare]); bit i of a plane is set iff coefficient i of the window is exactly 0.0.  The hashes are
        hash_windows'."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim != 4:
            raise ValueError("frames must be [n_clips, n_frames, H, W]")
        nc, nf, h, w = frames.shape
        stride = _window_stride(stride)
        n_win = int(self.lib.vdf_hash_window_count(nf, stride))
        out = np.zeros((nc, n_win, HASH_WORDS), np.uint64)
        zero = np.zeros((nc, n_win, HASH_WORDS), np.uint64)
        dc = np.zeros((nc, n_win), np.uint32) if want_dontcare else None
        self._check(self.lib.vdf_hash_windows_u8_planes(self.ctx, frames.ctypes.data, nc, nf, w, h, w * h, nf * w * h, stride, out.ctypes.data,
                                                        dc.ctypes.data if want_dontcare else None, zero.ctypes.data))
        return (out, zero, dc) if want_dontcare else (out, zero)

    def hash_windows_planes_device(self, d_frames: int, n_clips: int, frames_per_clip: int, w: int, h: int, stride: int, d_out: int, d_zero: int,
                                   d_dontcare: int = 0, frame_stride: Optional[int] = None, clip_stride: Optional[int] = None, stream: int = 0):
        """d_out and d_zero: n_clips x n_win x 16 words each."""
        stride = _window_stride(stride)
        fs = w * h if frame_stride is None else frame_stride
        cs = fs * frames_per_clip if clip_stride is None else clip_stride
        self._check(self.lib.vdf_hash_windows_u8_planes_device(self.ctx, d_frames, n_clips, frames_per_clip, w, h, fs, cs, stride, d_out,
                                                               d_dontcare or None, d_zero or None, stream or None))

    # --------------------------------------------- windows of videos of different sizes and lengths (include/vdf.h)
    @staticmethod
    def _pack_videos(stacks: Sequence[np.ndarray], crops=None):
        """ALL frames of every video one after the other in one buffer, every video on a 64-byte boundary: (buffer, CLIP_DTYPE records,
        frame counts [n] u32)."""
        stacks = [np.ascontiguousarray(s, dtype=np.uint8) for s in stacks]
        n = len(stacks)
        if any(s.ndim != 3 for s in stacks):
            raise ValueError("every video must be [n_frames, H, W]")
        clips = np.zeros(n, CLIP_DTYPE)
        n_frames = np.array([s.shape[0] for s in stacks], np.uint32)
        at = 0
        for i, s in enumerate(stacks):
            clips[i]["offset"], clips[i]["frame_stride"], clips[i]["w"], clips[i]["h"] = at, s.shape[1] * s.shape[2], s.shape[2], s.shape[1]
            at += (s.size + 63) & ~63
        buf = np.zeros(max(at, 1), np.uint8)
        for i, s in enumerate(stacks):
            buf[int(clips[i]["offset"]):int(clips[i]["offset"]) + s.size] = s.reshape(-1)
        if crops is not None:
            clips["crop"] = np.asarray(crops, dtype=np.uint32).reshape(n, 4)
        return buf, clips, n_frames

    def _hash_windows_clips(self, stacks, stride, crops, want_dontcare, planes):
        stride = _window_stride(stride)
        buf, clips, n_frames = self._pack_videos(stacks, crops)
        n = len(clips)
        # a video of fewer than 16 frames has no window: the library names it (first would not); the buffers are sized without it
        first = hash_windows_first(np.maximum(n_frames, 16), stride)
        rows = int(first[-1])
        out = np.zeros((rows, HASH_WORDS), np.uint64)
        zero = np.zeros((rows, HASH_WORDS), np.uint64) if planes else None
        dc = np.zeros(rows, np.uint32) if want_dontcare else None
        args = (self.ctx, buf.ctypes.data, buf.size, clips.ctypes.data if n else None, n_frames.ctypes.data if n else None, n, stride, out.ctypes.data,
                dc.ctypes.data if want_dontcare else None)
        if planes:
            self._check(self.lib.vdf_hash_windows_clips_u8_planes(*args, zero.ctypes.data))
        else:
            self._check(self.lib.vdf_hash_windows_clips_u8(*args))
        return out, zero, dc, first

    def hash_windows_clips(self, stacks: Sequence[np.ndarray], stride: int = 1, crops=None, want_dontcare: bool = False):
        """Every 16-frame window of videos of DIFFERENT frame sizes and lengths in one call (vdf_hash_windows_clips_u8): stacks = a list of
        [F_i >= 16, H_i, W_i] u8 arrays; crops (optional) = [n, 4] u32 left, right, top, bottom per video, read in place.
        -> (words [n_total, 16] u64, first [n + 1] u32 [, dontcare [n_total] u32]): video i's windows are rows first[i] ... first[i + 1], the
        layout align_windows* reads.  The words are hash_windows' for each video alone."""
        out, _, dc, first = self._hash_windows_clips(stacks, stride, crops, want_dontcare, False)
        return (out, first, dc) if want_dontcare else (out, first)

    def hash_windows_clips_planes(self, stacks: Sequence[np.ndarray], stride: int = 1, crops=None, want_dontcare: bool = False):
        """hash_windows_clips plus every window's zero plane (vdf_hash_windows_clips_u8_planes): -> (words [n_total, 16], zero [n_total, 16],
        first [n + 1] [, dontcare]).  Words and don't-care counts are the plain form's."""
        out, zero, dc, first = self._hash_windows_clips(stacks, stride, crops, want_dontcare, True)
        return (out, zero, first, dc) if want_dontcare else (out, zero, first)

    def hash_windows_clips_device(self, d_buf: int, buf_bytes: int, clips: np.ndarray, n_frames, stride: int, d_out: int, d_dontcare: int = 0,
                                  stream: int = 0):
        """vdf_hash_windows_clips_u8_device: clips = HOST array of CLIP_DTYPE records (offsets relative to d_buf), n_frames = HOST frame counts;
        every address is checked against buf_bytes before anything is queued.  d_out: hash_windows_first(n_frames, stride)[-1] x 16 words;
        ordered on `stream`."""
        c = np.ascontiguousarray(clips, dtype=CLIP_DTYPE).reshape(-1)
        nf = np.ascontiguousarray(n_frames, dtype=np.uint32).reshape(-1)
        if nf.size != c.size:
            raise ValueError("one frame count per video")
        self._check(self.lib.vdf_hash_windows_clips_u8_device(self.ctx, d_buf or None, int(buf_bytes), c.ctypes.data if c.size else None,
                                                              nf.ctypes.data if nf.size else None, c.size, _window_stride(stride), d_out or None,
                                                              d_dontcare or None, stream or None))

    def hash_windows_clips_planes_device(self, d_buf: int, buf_bytes: int, clips: np.ndarray, n_frames, stride: int, d_out: int, d_zero: int,
                                         d_dontcare: int = 0, stream: int = 0):
        """vdf_hash_windows_clips_u8_planes_device: d_out and d_zero hold hash_windows_first(n_frames, stride)[-1] x 16 words each."""
        c = np.ascontiguousarray(clips, dtype=CLIP_DTYPE).reshape(-1)
        nf = np.ascontiguousarray(n_frames, dtype=np.uint32).reshape(-1)
        if nf.size != c.size:
            raise ValueError("one frame count per video")
        self._check(self.lib.vdf_hash_windows_clips_u8_planes_device(self.ctx, d_buf or None, int(buf_bytes), c.ctypes.data if c.size else None,
                                                                     nf.ctypes.data if nf.size else None, c.size, _window_stride(stride), d_out or None,
                                                                     d_dontcare or None, d_zero or None, stream or None))

    # --------------------------------------------- retimed windows of a whole library in one call (include/vdf.h)
    def hash_windows_clips_retimed(self, stacks: Sequence[np.ndarray], rate, stride: int = 1, crops=None, want_dontcare: bool = False):
        """hash_windows_clips at rate = (num, den): the RETIMED windows (hash_windows_retimed) of videos of different frame sizes and lengths in
        one call (vdf_hash_windows_clips_u8_retimed).  stacks = a list of [F_i >= span, H_i, W_i] u8 arrays, span = (15 * num) // den + 1;
        crops (optional) = [n, 4] u32 left, right, top, bottom per video, read in place.
        -> (words [n_total, 16] u64, first [n + 1] u32 [, dontcare [n_total] u32]): video i's windows are rows first[i] ... first[i + 1]
        (hash_windows_first_retimed), the layout align_windows_retimed* reads.  The words are hash_windows_retimed's for each video alone."""
        stride = _window_stride(stride)
        num, den = _library_rate(rate)
        buf, clips, n_frames = self._pack_videos(stacks, crops)
        n = len(clips)
        # a video shorter than a window's span has no window: the library names it (first would not); the buffers are sized without it
        first = hash_windows_first_retimed(np.maximum(n_frames, (15 * num) // den + 1), (num, den), stride)
        rows = int(first[-1])
        out = np.zeros((rows, HASH_WORDS), np.uint64)
        dc = np.zeros(rows, np.uint32) if want_dontcare else None
        self._check(self.lib.vdf_hash_windows_clips_u8_retimed(self.ctx, buf.ctypes.data, buf.size, clips.ctypes.data if n else None,
                                                               n_frames.ctypes.data if n else None, n, stride, num, den, out.ctypes.data,
                                                               dc.ctypes.data if want_dontcare else None))
        return (out, first, dc) if want_dontcare else (out, first)

    def hash_windows_clips_retimed_device(self, d_buf: int, buf_bytes: int, clips: np.ndarray, n_frames, stride: int, rate, d_out: int,
                                          d_dontcare: int = 0, stream: int = 0):
        """vdf_hash_windows_clips_u8_retimed_device: clips = HOST array of CLIP_DTYPE records (offsets relative to d_buf), n_frames = HOST frame
        counts; every address is checked against buf_bytes before anything is queued.  d_out: hash_windows_first_retimed(n_frames, rate,
        stride)[-1] x 16 words; ordered on `stream`."""
        c = np.ascontiguousarray(clips, dtype=CLIP_DTYPE).reshape(-1)
        nf = np.ascontiguousarray(n_frames, dtype=np.uint32).reshape(-1)
        if nf.size != c.size:
            raise ValueError("one frame count per video")
        num, den = _window_rate(rate)
        self._check(self.lib.vdf_hash_windows_clips_u8_retimed_device(self.ctx, d_buf or None, int(buf_bytes), c.ctypes.data if c.size else None,
                                                                      nf.ctypes.data if nf.size else None, c.size, _window_stride(stride), num, den,
                                                                      d_out or None, d_dontcare or None, stream or None))

    # --------------------------------------------- retimed windows of a whole library at several rates in one call (include/vdf.h)
    def _windows_clips_rates_job(self, buf_ptr, buf_bytes, clips, n_frames, stride, rates, out_ptr, dc_ptr, stream):
        """(job, what it points into): the job of vdf_hash_windows_clips_u8_rates[_device]; the arrays must outlive the call."""
        num, den = _window_rates(rates)
        n = int(clips.size)
        job = _capi.VdfWindowsClipsRatesJob(buf_ptr or None, int(buf_bytes), clips.ctypes.data if n else None, n_frames.ctypes.data if n else None, n,
                                            _window_stride(stride), len(num), num.ctypes.data if len(num) else None, den.ctypes.data if len(num) else None,
                                            out_ptr or None, dc_ptr or None, stream or None)
        return job, (num, den, clips, n_frames)

    def hash_windows_clips_rates(self, stacks: Sequence[np.ndarray], rates, stride: int = 1, crops=None, want_dontcare: bool = False):
        """hash_windows_clips_retimed at up to 8 rates [(num, den), ...] from ONE upload, one resize and one spatial transform of every frame
        (vdf_hash_windows_clips_u8_rates).  stacks = a list of [F_i, H_i, W_i] u8 arrays, every F_i at least the longest span of the list; crops
        (optional) = [n, 4] u32 left, right, top, bottom per video, read in place.
        -> (words, first [, dontcare]): words = one [n_total_r, 16] u64 array per listed rate, first [n_rates, n + 1] u32 (hash_windows_first_rates),
        dontcare = one [n_total_r] u32 array per rate.  (words[r], first[r]) is what hash_windows_clips_retimed(stacks, rates[r], stride) gives and
        what align_windows_retimed* reads as its A side; the (1, 1) block is a B side."""
        stride = _window_stride(stride)
        buf, clips, n_frames = self._pack_videos(stacks, crops)
        # a video shorter than a span has no window at that rate and a bad list has no layout: the library names both (first would not), and
        # then writes nothing; the buffers are sized without them
        spans = [(15 * n) // d + 1 for n, d in (_window_rate(r) for r in rates) if 1 <= d <= n <= 2 * d and n <= 65535]
        try:
            first, rate_first = hash_windows_first_rates(np.maximum(n_frames, max(spans, default=16)), rates, stride)
        except VdfError:
            first, rate_first = np.zeros((0, len(clips) + 1), np.uint32), np.zeros(1, np.int64)
        rows = int(rate_first[-1])
        out = np.zeros((rows, HASH_WORDS), np.uint64)
        dc = np.zeros(rows, np.uint32) if want_dontcare else None
        job, keep = self._windows_clips_rates_job(buf.ctypes.data, buf.size, clips, n_frames, stride, rates, out.ctypes.data if first.shape[0] else 0,
                                                  dc.ctypes.data if want_dontcare and first.shape[0] else 0, 0)
        self._check(self.lib.vdf_hash_windows_clips_u8_rates(self.ctx, C.byref(job)))
        del keep
        if first.shape[0] == 0:
            raise VdfError(_capi.VDF_E_INVAL, "vdf_hash_windows_clips_u8_rates took a list of rates that has no layout")
        words = [out[rate_first[r]:rate_first[r + 1]] for r in range(first.shape[0])]
        return (words, first, [dc[rate_first[r]:rate_first[r + 1]] for r in range(first.shape[0])]) if want_dontcare else (words, first)

    def hash_windows_clips_rates_device(self, d_buf: int, buf_bytes: int, clips: np.ndarray, n_frames, stride: int, rates, d_out: int,
                                        d_dontcare: int = 0, stream: int = 0):
        """vdf_hash_windows_clips_u8_rates_device: clips = HOST array of CLIP_DTYPE records (offsets relative to d_buf), n_frames = HOST frame
        counts, rates = HOST list; every address is checked against buf_bytes before anything is queued.  d_out: 16 words for each of the
        hash_windows_first_rates(n_frames, rates, stride)[1][-1] rows, rate-major; d_dontcare (optional): one u32 per row.  Ordered on `stream`."""
        c = np.ascontiguousarray(clips, dtype=CLIP_DTYPE).reshape(-1)
        nf = np.ascontiguousarray(n_frames, dtype=np.uint32).reshape(-1)
        if nf.size != c.size:
            raise ValueError("one frame count per video")
        job, keep = self._windows_clips_rates_job(d_buf, buf_bytes, c, nf, stride, rates, d_out, d_dontcare, stream)
        self._check(self.lib.vdf_hash_windows_clips_u8_rates_device(self.ctx, C.byref(job)))
        del keep

    # --------------------------------------------- flipped and reversed stretches (include/vdf.h)
    def window_variants(self, d_hashes: int, d_zero: int, d_first: int, n_videos: int, variant: int, d_out: int, d_skip: int = 0, d_out_skip: int = 0,
                        stream: int = 0):
        """vdf_window_variants_device: d_out (and d_out_skip) = the variant set of the window hashes at d_hashes / d_zero / d_first - with
        bit 2 of the variant every video's rows in reversed order.  Device pointers; ordered on stream."""
        self._check(self.lib.vdf_window_variants_device(self.ctx, d_hashes or None, d_zero or None, d_first or None, int(n_videos), d_skip or None,
                                                        _align_uint32("variant", variant), d_out or None, d_out_skip or None, stream or None))

    def align_windows_variants(self, a_hashes, a_first, a_zero=None, b_hashes=None, b_first=None, b_zero=None, tol_int: int = 350, min_run: int = 1,
                               variant_mask: int = 2, a_skip=None, b_skip=None, capacity: int = 1024):
        """align_windows against the variants of B named by variant_mask (vdf_align_windows_variants; bits 1 ... 7): b_zero is B's zero planes;
        b_hashes None: self mode, B = A with a_zero.  offset and start_a + offset count in the DERIVED order of b (reversed with bit 2).
        -> (records [min(found, capacity)] of ALIGN_VARIANT_DTYPE in (variant, a, b) order, found)."""
        keep, args = _align_variants_host_args(a_hashes, a_zero, a_first, b_hashes, b_zero, b_first, a_skip, b_skip)
        out = np.zeros(max(int(capacity), 0), ALIGN_VARIANT_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows_variants(self.ctx, *args, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run),
                                                        _variant_mask(variant_mask), out.ctypes.data if out.size else None, out.size, C.byref(n)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_variants_device(self, d_a_hashes: int, d_a_first: int, n_a: int, d_a_zero: int = 0, d_b_hashes: int = 0, d_b_first: int = 0,
                                      n_b: int = 0, d_b_zero: int = 0, tol_int: int = 350, min_run: int = 1, variant_mask: int = 2, d_a_skip: int = 0,
                                      d_b_skip: int = 0, capacity: int = 1024, stream: int = 0):
        """The same on device arrays (d_b_hashes 0: self mode); the records come back to the host, the call waits for its own work."""
        out = np.zeros(max(int(capacity), 0), ALIGN_VARIANT_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows_variants_device(self.ctx, d_a_hashes or None, d_a_zero or None, d_a_first or None, int(n_a), d_a_skip or None,
                                                               d_b_hashes or None, d_b_zero or None, d_b_first or None, int(n_b), d_b_skip or None,
                                                               _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run),
                                                               _variant_mask(variant_mask), out.ctypes.data if out.size else None, out.size, C.byref(n),
                                                               stream or None))
        return out[:min(n.value, out.size)], int(n.value)

    # --------------------------------------------- videos aligned on their window hashes (include/vdf.h)
    def align_windows(self, a_hashes, a_first, b_hashes=None, b_first=None, tol_int: int = 350, min_run: int = 1, a_skip=None, b_skip=None,
                      capacity: int = 1024):
        """The longest shared stretch of every pair of videos (vdf_align_windows).  a_hashes [windows, 16] u64 = the window hashes of the
        videos one after the other, a_first [videos + 1] u32; b_hashes None: self mode, the pairs a < b of A.  skip: one byte per window,
        non-zero = the window abstains.  -> (records [min(found, capacity)] of ALIGN_DTYPE in (a, b) order, found); found > capacity: call
        again with a larger capacity."""
        keep, args = _align_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)
        out = np.zeros(max(int(capacity), 0), ALIGN_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows(self.ctx, *args, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run),
                                               out.ctypes.data if out.size else None, out.size, C.byref(n)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_device(self, d_a_hashes: int, d_a_first: int, n_a: int, d_b_hashes: int = 0, d_b_first: int = 0, n_b: int = 0,
                             tol_int: int = 350, min_run: int = 1, d_a_skip: int = 0, d_b_skip: int = 0, capacity: int = 1024, stream: int = 0):
        """The same on device arrays (d_b_hashes 0: self mode); the records come back to the host, the call waits for its own work."""
        out = np.zeros(max(int(capacity), 0), ALIGN_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows_device(self.ctx, d_a_hashes or None, d_a_first or None, int(n_a), d_a_skip or None, d_b_hashes or None,
                                                      d_b_first or None, int(n_b), d_b_skip or None, _align_uint32("tol_int", tol_int),
                                                      _align_uint32("min_run", min_run), out.ctypes.data if out.size else None, out.size, C.byref(n),
                                                      stream or None))
        return out[:min(n.value, out.size)], int(n.value)

    # --------------------------------------------- every shared stretch of a pair (include/vdf.h)
    def align_windows_stretches(self, a_hashes, a_first, b_hashes=None, b_first=None, tol_int: int = 350, min_run: int = 1, max_stretches: int = 4,
                                guard: int = 0, a_skip=None, b_skip=None, capacity: int = 1024):
        """Every shared stretch of every pair of videos (vdf_align_windows_stretches): align_windows' record as rank 0, then per rank the best
        run of the pair's matrix with the rectangles of the earlier ranks - their rows of A x their rows of B, widened by guard windows -
        masked; at most max_stretches (1 ... 8) per pair.  -> (records [min(found, capacity)] of ALIGN_STRETCH_DTYPE in (a, b, rank) order,
        found); found > capacity: call again with a larger capacity."""
        keep, args = _align_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)
        out = np.zeros(max(int(capacity), 0), ALIGN_STRETCH_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows_stretches(self.ctx, *args, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run),
                                                         _align_uint32("max_stretches", max_stretches), _align_uint32("guard", guard),
                                                         out.ctypes.data if out.size else None, out.size, C.byref(n)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_stretches_device(self, d_a_hashes: int, d_a_first: int, n_a: int, d_b_hashes: int = 0, d_b_first: int = 0, n_b: int = 0,
                                       tol_int: int = 350, min_run: int = 1, max_stretches: int = 4, guard: int = 0, d_a_skip: int = 0,
                                       d_b_skip: int = 0, capacity: int = 1024, stream: int = 0):
        """The same on device arrays (d_b_hashes 0: self mode); the records come back to the host, the call waits for its own work."""
        out = np.zeros(max(int(capacity), 0), ALIGN_STRETCH_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows_stretches_device(self.ctx, d_a_hashes or None, d_a_first or None, int(n_a), d_a_skip or None,
                                                                d_b_hashes or None, d_b_first or None, int(n_b), d_b_skip or None,
                                                                _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run),
                                                                _align_uint32("max_stretches", max_stretches), _align_uint32("guard", guard),
                                                                out.ctypes.data if out.size else None, out.size, C.byref(n), stream or None))
        return out[:min(n.value, out.size)], int(n.value)

    def window_class_layout_device(self, d_hashes: int, d_first: int, n_videos: int, d_out: int, capacity_rows: int, d_zero: int = 0, d_skip: int = 0,
                                   min_run: int = 1, stream: int = 0) -> int:
        """vdf_window_class_layout_device: the class-major seeds (d_zero 0; 36 dwords each) or rows (72 dwords each) of a set into the device
        buffer d_out - what align_class_layout_kernel writes for the seeded flipped alignment.  -> the number of rows written."""
        n = C.c_size_t(0)
        self._check(self.lib.vdf_window_class_layout_device(self.ctx, d_hashes or None, d_zero or None, d_first or None, int(n_videos), d_skip or None,
                                                            _align_uint32("min_run", min_run), d_out or None, int(capacity_rows), C.byref(n), stream or None))
        return int(n.value)

    # --------------------------------------------- the flipped alignment seeded and on a list of triples (include/vdf.h)
    def align_seed_pairs_variants(self, a_hashes, a_first, a_zero=None, b_hashes=None, b_first=None, b_zero=None, tol_int: int = 350, min_run: int = 1,
                                  variant_mask: int = 2, a_skip=None, b_skip=None, capacity: int = 1024):
        """The candidate pairs of align_windows_variants under every variant of variant_mask, from ONE pass over the seeds
        (vdf_align_seed_pairs_variants).  -> (triples [min(found, capacity)] of VIDEO_PAIR_VARIANT_DTYPE in (variant, a, b) order, found)."""
        keep, args = _align_variants_host_args(a_hashes, a_zero, a_first, b_hashes, b_zero, b_first, a_skip, b_skip)  # keep: holds the arrays alive
        out = np.zeros(max(int(capacity), 0), VIDEO_PAIR_VARIANT_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_seed_pairs_variants(self.ctx, *args, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run),
                                                           _variant_mask(variant_mask), out.ctypes.data if out.size else None, out.size, C.byref(n)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_seed_pairs_variants_device(self, d_a_hashes: int, d_a_first: int, n_a: int, d_a_zero: int = 0, d_b_hashes: int = 0, d_b_first: int = 0,
                                         n_b: int = 0, d_b_zero: int = 0, tol_int: int = 350, min_run: int = 1, variant_mask: int = 2, d_a_skip: int = 0,
                                         d_b_skip: int = 0, capacity: int = 1024, stream: int = 0):
        """The same on device arrays (d_b_hashes 0: self mode); the triples come back to the host, the call waits for its own work."""
        out = np.zeros(max(int(capacity), 0), VIDEO_PAIR_VARIANT_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_seed_pairs_variants_device(self.ctx, d_a_hashes or None, d_a_zero or None, d_a_first or None, int(n_a),
                                                                  d_a_skip or None, d_b_hashes or None, d_b_zero or None, d_b_first or None, int(n_b),
                                                                  d_b_skip or None, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run),
                                                                  _variant_mask(variant_mask), out.ctypes.data if out.size else None, out.size,
                                                                  C.byref(n), stream or None))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_variants_pairs(self, a_hashes, a_first, triples, a_zero=None, b_hashes=None, b_first=None, b_zero=None, tol_int: int = 350,
                                     min_run: int = 1, a_skip=None, b_skip=None, capacity: int = 1024):
        """align_windows_variants on the listed (variant, a, b) triples only (vdf_align_windows_variants_pairs): VIDEO_PAIR_VARIANT_DTYPE records
        or [n, 3] integers, strictly increasing.  The records are align_windows_variants' for those triples, field for field."""
        keep, args = _align_variants_host_args(a_hashes, a_zero, a_first, b_hashes, b_zero, b_first, a_skip, b_skip)  # keep: holds the arrays alive
        t = video_pair_variants(triples)
        out = np.zeros(max(int(capacity), 0), ALIGN_VARIANT_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows_variants_pairs(self.ctx, *args, t.ctypes.data if t.size else None, t.size, _align_uint32("tol_int", tol_int),
                                                              _align_uint32("min_run", min_run), out.ctypes.data if out.size else None, out.size,
                                                              C.byref(n)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_variants_pairs_device(self, d_a_hashes: int, d_a_first: int, n_a: int, triples, d_a_zero: int = 0, d_b_hashes: int = 0,
                                            d_b_first: int = 0, n_b: int = 0, d_b_zero: int = 0, tol_int: int = 350, min_run: int = 1, d_a_skip: int = 0,
                                            d_b_skip: int = 0, capacity: int = 1024, stream: int = 0):
        """The same on device arrays (the triple list stays a host array)."""
        t = video_pair_variants(triples)
        out = np.zeros(max(int(capacity), 0), ALIGN_VARIANT_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows_variants_pairs_device(self.ctx, d_a_hashes or None, d_a_zero or None, d_a_first or None, int(n_a),
                                                                     d_a_skip or None, d_b_hashes or None, d_b_zero or None, d_b_first or None, int(n_b),
                                                                     d_b_skip or None, t.ctypes.data if t.size else None, t.size,
                                                                     _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run),
                                                                     out.ctypes.data if out.size else None, out.size, C.byref(n), stream or None))
        return out[:min(n.value, out.size)], int(n.value)

    # --------------------------------------------- seeded candidate pairs, the align calls on a list of pairs (include/vdf.h)
    def align_seed_pairs(self, a_hashes, a_first, b_hashes=None, b_first=None, tol_int: int = 350, min_run: int = 1, a_skip=None, b_skip=None,
                         capacity: int = 1024):
        """The candidate pairs of the align calls (vdf_align_seed_pairs): the pairs (a, b) with a matching cell (ka, kb), ka % min_run == 0 -
        every pair align_windows has a record for, and perhaps a few more.  -> (pairs [min(found, capacity)] of VIDEO_PAIR_DTYPE in (a, b)
        order, found); found > capacity: call again with a larger capacity."""
        keep, args = _align_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)
        out = np.zeros(max(int(capacity), 0), VIDEO_PAIR_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_seed_pairs(self.ctx, *args, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run),
                                                  out.ctypes.data if out.size else None, out.size, C.byref(n)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_seed_pairs_device(self, d_a_hashes: int, d_a_first: int, n_a: int, d_b_hashes: int = 0, d_b_first: int = 0, n_b: int = 0,
                                tol_int: int = 350, min_run: int = 1, d_a_skip: int = 0, d_b_skip: int = 0, capacity: int = 1024, stream: int = 0):
        """The same on device arrays (d_b_hashes 0: self mode); the pairs come back to the host, the call waits for its own work."""
        out = np.zeros(max(int(capacity), 0), VIDEO_PAIR_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_seed_pairs_device(self.ctx, d_a_hashes or None, d_a_first or None, int(n_a), d_a_skip or None, d_b_hashes or None,
                                                         d_b_first or None, int(n_b), d_b_skip or None, _align_uint32("tol_int", tol_int),
                                                         _align_uint32("min_run", min_run), out.ctypes.data if out.size else None, out.size, C.byref(n),
                                                         stream or None))
        return out[:min(n.value, out.size)], int(n.value)

    def align_seed_pairs_rates(self, a_hashes, a_first, b_hashes, b_first, rates, tol_int: int = 350, min_run: int = 1, a_rate_first=None, a_skip=None,
                               b_skip=None, exclude_same: bool = False, capacity: int = 1024):
        """The candidates of the retimed alignment at every rate of `rates`, every phase, from ONE pass (vdf_align_seed_pairs_rates; DESIGN.md
        4.22): arguments and result as align_seed_pairs_rates_host - A rate-major, as hash_windows_clips_rates writes it.  found > capacity: call
        again with a larger capacity."""
        keep, args = _seed_rates_host_args(a_hashes, a_first, a_rate_first, a_skip, b_hashes, b_first, b_skip, len(rates))
        job, out, n, keep2 = _seed_rates_job(rates=rates, a_rate_first=a_rate_first, tol_int=tol_int, min_run=min_run, exclude_same=exclude_same,
                                             capacity=capacity, **args)
        self._check(self.lib.vdf_align_seed_pairs_rates(self.ctx, C.byref(job)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_seed_pairs_rates_device(self, d_a_hashes: int, d_a_first: int, n_a: int, d_b_hashes: int, d_b_first: int, n_b: int, rates, tol_int: int = 350,
                                      min_run: int = 1, a_rate_first=None, d_a_skip: int = 0, d_b_skip: int = 0, exclude_same: bool = False,
                                      capacity: int = 1024, stream: int = 0):
        """The same on device arrays - d_a_first: n_rates x (n_a + 1) u32; rates and a_rate_first stay HOST lists; the triples come back to the host,
        the call is ordered on `stream` and waits for its own work."""
        job, out, n, keep = _seed_rates_job(d_a_hashes, d_a_first, n_a, a_rate_first, d_a_skip, d_b_hashes, d_b_first, n_b, d_b_skip, rates, tol_int, min_run,
                                            exclude_same, capacity, stream)
        self._check(self.lib.vdf_align_seed_pairs_rates_device(self.ctx, C.byref(job)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_rates(self, a_hashes, a_first, b_hashes, b_first, rates, tol_int: int = 350, min_run: int = 1, a_rate_first=None, a_skip=None,
                            b_skip=None, triples=None, seed: bool = False, exclude_same: bool = False, capacity: int = 1024):
        """The retimed alignment at every rate of `rates` in ONE call (vdf_align_windows_rates): arguments and result as
        align_windows_rates_host.  The arrays go up once - with seed=True for the seed pass and the band walk alike - and the triples of all rates
        are one launch set.  found > capacity: call again with a larger capacity."""
        keep, args = _seed_rates_host_args(a_hashes, a_first, a_rate_first, a_skip, b_hashes, b_first, b_skip, len(rates))
        job, out, n, keep2 = _align_rates_job(rates=rates, a_rate_first=a_rate_first, tol_int=tol_int, min_run=min_run, triples=triples, seed=seed,
                                              exclude_same=exclude_same, capacity=capacity, **args)
        self._check(self.lib.vdf_align_windows_rates(self.ctx, C.byref(job)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_rates_device(self, d_a_hashes: int, d_a_first: int, n_a: int, d_b_hashes: int, d_b_first: int, n_b: int, rates, tol_int: int = 350,
                                   min_run: int = 1, a_rate_first=None, d_a_skip: int = 0, d_b_skip: int = 0, triples=None, seed: bool = False,
                                   exclude_same: bool = False, capacity: int = 1024, stream: int = 0):
        """The same on device arrays - d_a_first: n_rates x (n_a + 1) u32; rates, a_rate_first and triples stay HOST data; the records come back to
        the host, the call is ordered on `stream` and waits for its own work."""
        job, out, n, keep = _align_rates_job(d_a_hashes, d_a_first, n_a, a_rate_first, d_a_skip, d_b_hashes, d_b_first, n_b, d_b_skip, rates, tol_int, min_run,
                                             triples, seed, exclude_same, capacity, stream)
        self._check(self.lib.vdf_align_windows_rates_device(self.ctx, C.byref(job)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_rates_stretches(self, a_hashes, a_first, b_hashes, b_first, rates, tol_int: int = 350, min_run: int = 1, max_stretches: int = 4,
                                      guard: int = 15, a_rate_first=None, a_skip=None, b_skip=None, triples=None, seed: bool = False,
                                      exclude_same: bool = False, capacity: int = 1024):
        """Every stretch of every (rate, a, b) triple, ranked, in ONE call (vdf_align_windows_rates_stretches): arguments and result as
        align_windows_rates_stretches_host.  The arrays go up once, for the seed pass and every round; round k walks only the triples that had a
        record in round k - 1.  found > capacity: call again with a larger capacity."""
        keep, args = _seed_rates_host_args(a_hashes, a_first, a_rate_first, a_skip, b_hashes, b_first, b_skip, len(rates))
        job, out, n, keep2 = _align_rates_stretches_job(rates=rates, a_rate_first=a_rate_first, tol_int=tol_int, min_run=min_run, triples=triples, seed=seed,
                                                        exclude_same=exclude_same, max_stretches=max_stretches, guard=guard, capacity=capacity, **args)
        self._check(self.lib.vdf_align_windows_rates_stretches(self.ctx, C.byref(job)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_rates_stretches_device(self, d_a_hashes: int, d_a_first: int, n_a: int, d_b_hashes: int, d_b_first: int, n_b: int, rates,
                                             tol_int: int = 350, min_run: int = 1, max_stretches: int = 4, guard: int = 15, a_rate_first=None,
                                             d_a_skip: int = 0, d_b_skip: int = 0, triples=None, seed: bool = False, exclude_same: bool = False,
                                             capacity: int = 1024, stream: int = 0):
        """The same on device arrays - d_a_first: n_rates x (n_a + 1) u32; rates, a_rate_first and triples stay HOST data; the records come back to
        the host, the call is ordered on `stream` and waits for its own work."""
        job, out, n, keep = _align_rates_stretches_job(d_a_hashes, d_a_first, n_a, a_rate_first, d_a_skip, d_b_hashes, d_b_first, n_b, d_b_skip, rates, tol_int,
                                                       min_run, triples, seed, exclude_same, max_stretches, guard, capacity, stream)
        self._check(self.lib.vdf_align_windows_rates_stretches_device(self.ctx, C.byref(job)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_pairs(self, a_hashes, a_first, pairs, b_hashes=None, b_first=None, tol_int: int = 350, min_run: int = 1, a_skip=None, b_skip=None,
                            capacity: int = 1024):
        """align_windows on the listed pairs only (vdf_align_windows_pairs): pairs = VIDEO_PAIR_DTYPE records or [n, 2] integers, strictly
        increasing in (a, b), a < b in self mode.  The records are align_windows' for those pairs, field for field."""
        keep, args = _align_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)
        p = video_pairs(pairs)
        out = np.zeros(max(int(capacity), 0), ALIGN_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows_pairs(self.ctx, *args, p.ctypes.data if p.size else None, p.size, _align_uint32("tol_int", tol_int),
                                                     _align_uint32("min_run", min_run), out.ctypes.data if out.size else None, out.size, C.byref(n)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_pairs_device(self, d_a_hashes: int, d_a_first: int, n_a: int, pairs, d_b_hashes: int = 0, d_b_first: int = 0, n_b: int = 0,
                                   tol_int: int = 350, min_run: int = 1, d_a_skip: int = 0, d_b_skip: int = 0, capacity: int = 1024, stream: int = 0):
        """The same on device arrays (the pair list stays a host array)."""
        p = video_pairs(pairs)
        out = np.zeros(max(int(capacity), 0), ALIGN_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows_pairs_device(self.ctx, d_a_hashes or None, d_a_first or None, int(n_a), d_a_skip or None, d_b_hashes or None,
                                                            d_b_first or None, int(n_b), d_b_skip or None, p.ctypes.data if p.size else None, p.size,
                                                            _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run),
                                                            out.ctypes.data if out.size else None, out.size, C.byref(n), stream or None))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_stretches_pairs(self, a_hashes, a_first, pairs, b_hashes=None, b_first=None, tol_int: int = 350, min_run: int = 1,
                                      max_stretches: int = 4, guard: int = 0, a_skip=None, b_skip=None, capacity: int = 1024):
        """align_windows_stretches on the listed pairs only (vdf_align_windows_stretches_pairs)."""
        keep, args = _align_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)
        p = video_pairs(pairs)
        out = np.zeros(max(int(capacity), 0), ALIGN_STRETCH_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows_stretches_pairs(self.ctx, *args, p.ctypes.data if p.size else None, p.size, _align_uint32("tol_int", tol_int),
                                                               _align_uint32("min_run", min_run), _align_uint32("max_stretches", max_stretches),
                                                               _align_uint32("guard", guard), out.ctypes.data if out.size else None, out.size,
                                                               C.byref(n)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_stretches_pairs_device(self, d_a_hashes: int, d_a_first: int, n_a: int, pairs, d_b_hashes: int = 0, d_b_first: int = 0,
                                             n_b: int = 0, tol_int: int = 350, min_run: int = 1, max_stretches: int = 4, guard: int = 0,
                                             d_a_skip: int = 0, d_b_skip: int = 0, capacity: int = 1024, stream: int = 0):
        """The same on device arrays (the pair list stays a host array)."""
        p = video_pairs(pairs)
        out = np.zeros(max(int(capacity), 0), ALIGN_STRETCH_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows_stretches_pairs_device(self.ctx, d_a_hashes or None, d_a_first or None, int(n_a), d_a_skip or None,
                                                                      d_b_hashes or None, d_b_first or None, int(n_b), d_b_skip or None,
                                                                      p.ctypes.data if p.size else None, p.size, _align_uint32("tol_int", tol_int),
                                                                      _align_uint32("min_run", min_run), _align_uint32("max_stretches", max_stretches),
                                                                      _align_uint32("guard", guard), out.ctypes.data if out.size else None, out.size,
                                                                      C.byref(n), stream or None))
        return out[:min(n.value, out.size)], int(n.value)

    # --------------------------------------------- retimed windows aligned in one call (include/vdf.h)
    def align_windows_retimed(self, a_hashes, a_first, b_hashes, b_first, rate, tol_int: int = 350, min_run: int = 1, a_skip=None, b_skip=None,
                              capacity: int = 1024):
        """Which video of A is a copy of which video of B at num / den of its frames, and where (vdf_align_windows_retimed): a_hashes = RETIMED
        windows at stride 1 (hash_windows(..., rate=rate)), b_hashes = plain windows at stride 1, rate = (num, den).  Every phase of the rate in
        one call: per pair the best run over the sub-sampled windows p + num i of a against den j of b.  No self mode.
        -> (records [min(found, capacity)] of ALIGN_RETIMED_DTYPE in (a, b) order, found); found > capacity: call again with a larger capacity."""
        keep, args = _align_retimed_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)
        out = np.zeros(max(int(capacity), 0), ALIGN_RETIMED_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows_retimed(self.ctx, *args, _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run),
                                                       *_align_rate(rate), out.ctypes.data if out.size else None, out.size, C.byref(n)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_retimed_device(self, d_a_hashes: int, d_a_first: int, n_a: int, d_b_hashes: int, d_b_first: int, n_b: int, rate,
                                     tol_int: int = 350, min_run: int = 1, d_a_skip: int = 0, d_b_skip: int = 0, capacity: int = 1024, stream: int = 0):
        """The same on device arrays; the records come back to the host, the call waits for its own work."""
        out = np.zeros(max(int(capacity), 0), ALIGN_RETIMED_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows_retimed_device(self.ctx, d_a_hashes or None, d_a_first or None, int(n_a), d_a_skip or None,
                                                              d_b_hashes or None, d_b_first or None, int(n_b), d_b_skip or None,
                                                              _align_uint32("tol_int", tol_int), _align_uint32("min_run", min_run), *_align_rate(rate),
                                                              out.ctypes.data if out.size else None, out.size, C.byref(n), stream or None))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_retimed_pairs(self, a_hashes, a_first, pairs, b_hashes, b_first, rate, tol_int: int = 350, min_run: int = 1, a_skip=None,
                                    b_skip=None, capacity: int = 1024):
        """align_windows_retimed on the listed pairs only (vdf_align_windows_retimed_pairs): pairs = VIDEO_PAIR_DTYPE records or [n, 2] integers,
        strictly increasing in (a, b).  The records are align_windows_retimed's for those pairs, field for field."""
        keep, args = _align_retimed_host_args(a_hashes, a_first, b_hashes, b_first, a_skip, b_skip)
        p = video_pairs(pairs)
        out = np.zeros(max(int(capacity), 0), ALIGN_RETIMED_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows_retimed_pairs(self.ctx, *args, p.ctypes.data if p.size else None, p.size, _align_uint32("tol_int", tol_int),
                                                             _align_uint32("min_run", min_run), *_align_rate(rate),
                                                             out.ctypes.data if out.size else None, out.size, C.byref(n)))
        return out[:min(n.value, out.size)], int(n.value)

    def align_windows_retimed_pairs_device(self, d_a_hashes: int, d_a_first: int, n_a: int, pairs, d_b_hashes: int, d_b_first: int, n_b: int, rate,
                                           tol_int: int = 350, min_run: int = 1, d_a_skip: int = 0, d_b_skip: int = 0, capacity: int = 1024,
                                           stream: int = 0):
        """The same on device arrays (the pair list stays a host array)."""
        p = video_pairs(pairs)
        out = np.zeros(max(int(capacity), 0), ALIGN_RETIMED_DTYPE)
        n = C.c_size_t(0)
        self._check(self.lib.vdf_align_windows_retimed_pairs_device(self.ctx, d_a_hashes or None, d_a_first or None, int(n_a), d_a_skip or None,
                                                                    d_b_hashes or None, d_b_first or None, int(n_b), d_b_skip or None,
                                                                    p.ctypes.data if p.size else None, p.size, _align_uint32("tol_int", tol_int),
                                                                    _align_uint32("min_run", min_run), *_align_rate(rate),
                                                                    out.ctypes.data if out.size else None, out.size, C.byref(n), stream or None))
        return out[:min(n.value, out.size)], int(n.value)

    # --------------------------------------------- the zero plane and the flipped hashes (include/vdf.h)
    def hash_frames_planes(self, frames: np.ndarray, want_dontcare: bool = False):
        """hash_frames plus the zero planes (vdf_hash_frames_u8_planes): -> (hashes [n, 16] u64, zero [n, 16] u64 [, dontcare]); bit i of a
        zero plane is set iff coefficient i of the clip is exactly 0.0.  The hashes are the plain call's."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim != 4:
            raise ValueError("frames must be [n_clips, n_frames, H, W]")
        nc, nf, h, w = frames.shape
        out = np.zeros((nc, HASH_WORDS), np.uint64)
        zero = np.zeros((nc, HASH_WORDS), np.uint64)
        dc = np.zeros(nc, np.uint32) if want_dontcare else None
        self._check(self.lib.vdf_hash_frames_u8_planes(self.ctx, frames.ctypes.data, nc, nf, w, h, w * h, nf * w * h, out.ctypes.data,
                                                       dc.ctypes.data if want_dontcare else None, zero.ctypes.data))
        return (out, zero, dc) if want_dontcare else (out, zero)

    def hash_frames_planes_device(self, d_frames: int, n_clips: int, frames_per_clip: int, w: int, h: int, d_out: int, d_zero: int,
                                  d_dontcare: int = 0, frame_stride: Optional[int] = None, clip_stride: Optional[int] = None, stream: int = 0):
        fs = w * h if frame_stride is None else frame_stride
        cs = fs * frames_per_clip if clip_stride is None else clip_stride
        self._check(self.lib.vdf_hash_frames_u8_planes_device(self.ctx, d_frames, n_clips, frames_per_clip, w, h, fs, cs, d_out, d_dontcare or None,
                                                              d_zero or None, stream or None))

    def hash_clips_planes(self, stacks: Sequence[np.ndarray], crops=None, want_dontcare: bool = False):
        """hash_clips plus the zero planes (vdf_hash_clips_u8_planes): -> (hashes [n, 16] u64, zero [n, 16] u64 [, dontcare]).  With crops
        (e.g. the boxes a letterbox call detected) the planes - and every variant derived from them - are those of the CROPPED clips."""
        buf, clips, nf = self._pack_stacks(stacks)
        n = len(clips)
        if crops is not None:
            clips["crop"] = np.asarray(crops, dtype=np.uint32).reshape(n, 4)
        out = np.zeros((n, HASH_WORDS), np.uint64)
        zero = np.zeros((n, HASH_WORDS), np.uint64)
        dc = np.zeros(n, np.uint32) if want_dontcare else None
        self._check(self.lib.vdf_hash_clips_u8_planes(self.ctx, buf.ctypes.data, buf.size, clips.ctypes.data, n, nf, out.ctypes.data,
                                                      dc.ctypes.data if want_dontcare else None, zero.ctypes.data))
        return (out, zero, dc) if want_dontcare else (out, zero)

    def hash_clips_planes_device(self, d_buf: int, buf_bytes: int, clips: np.ndarray, d_out: int, d_zero: int, d_dontcare: int = 0,
                                 frames_per_clip: int = 16, stream: int = 0):
        c = np.ascontiguousarray(clips, dtype=CLIP_DTYPE)
        self._check(self.lib.vdf_hash_clips_u8_planes_device(self.ctx, d_buf, int(buf_bytes), c.ctypes.data if c.size else None, c.size,
                                                             int(frames_per_clip), d_out, d_dontcare or None, d_zero or None, stream or None))

    def hash_variants_device(self, d_hashes: int, d_zero: int, n: int, variant: int, d_out: int, stream: int = 0):
        """d_out[c] = the hash of clip c flipped by `variant` (bit 0 = mirror along W, 1 = flip along H, 2 = reverse the frames)."""
        self._check(self.lib.vdf_hash_variants_device(self.ctx, d_hashes or None, d_zero or None, int(n), int(variant), d_out or None, stream or None))

    def _variant_groups(self, call, variant_mask: int):
        arr = (VdfGroups * 8)()
        try:
            self._check(call(arr))
            return {v: _groups_to_lists(arr[v]) for v in range(1, 8) if variant_mask >> v & 1}
        finally:
            for v in range(8):
                self.lib.vdf_groups_free(C.byref(arr[v]))

    def search_variants_sorted(self, hashes, zero, durations, tol_int: int, variant_mask: int):
        """vdf_search_variants on SoA input in Search::sort order: {v: [(r, [indices whose hash is within tol_int of the variant-v hash of r])]}
        for every v of variant_mask (bits 1 ... 7); (r, r) and empty groups are dropped."""
        h = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1, HASH_WORDS)
        z = np.ascontiguousarray(zero, dtype=np.uint64).reshape(-1, HASH_WORDS)
        d = np.ascontiguousarray(durations, dtype=np.uint32)
        assert h.shape == z.shape and h.shape[0] == d.shape[0]
        return self._variant_groups(lambda arr: self.lib.vdf_search_variants(self.ctx, h.ctypes.data, z.ctypes.data, d.ctypes.data, len(d), int(tol_int),
                                                                             int(variant_mask), arr), int(variant_mask))

    def search_variants_device(self, d_hashes: int, d_zero: int, d_durations: int, n: int, tol_int: int, variant_mask: int, stream: int = 0):
        return self._variant_groups(lambda arr: self.lib.vdf_search_variants_device(self.ctx, d_hashes or None, d_zero or None, d_durations or None, int(n),
                                                                                    int(tol_int), int(variant_mask), arr, stream or None), int(variant_mask))

    @staticmethod
    def _pack_stacks(stacks: Sequence[np.ndarray]):
        """The stacks of a mixed call one after the other in one buffer, every clip on a 64-byte boundary: (buffer, CLIP_DTYPE records, frames)."""
        stacks = [np.ascontiguousarray(s, dtype=np.uint8) for s in stacks]
        n = len(stacks)
        if any(s.ndim != 3 for s in stacks):
            raise ValueError("every clip must be [n_frames, H, W]")
        nf = min((s.shape[0] for s in stacks), default=16)
        clips = np.zeros(n, CLIP_DTYPE)
        at = 0
        for i, s in enumerate(stacks):
            clips[i]["offset"], clips[i]["frame_stride"], clips[i]["w"], clips[i]["h"] = at, s.shape[1] * s.shape[2], s.shape[2], s.shape[1]
            at += (min(s.shape[0], 16) * s.shape[1] * s.shape[2] + 63) & ~63
        buf = np.zeros(max(at, 1), np.uint8)
        for i, s in enumerate(stacks):
            flat = s[:16].reshape(-1)
            buf[int(clips[i]["offset"]):int(clips[i]["offset"]) + flat.size] = flat
        return buf, clips, nf

    def hash_clips_letterbox(self, stacks: Sequence[np.ndarray], want_dontcare: bool = False):
        """crop_video_frames(Cropdetect::Letterbox) + from_frames for clips of DIFFERENT frame sizes in one call (vdf_hash_clips_u8_letterbox):
        stacks = a list of [>= 16, H, W] u8 arrays -> (hashes [n, 16] u64, crops [n, 4] u32 = l, r, t, b [, dontcare [n] u32]), in the order
        of the list."""
        buf, clips, nf = self._pack_stacks(stacks)
        n = len(clips)
        out = np.zeros((n, HASH_WORDS), np.uint64)
        crops = np.zeros((n, 4), np.uint32)
        dc = np.zeros(n, np.uint32) if want_dontcare else None
        self._check(self.lib.vdf_hash_clips_u8_letterbox(self.ctx, buf.ctypes.data, buf.size, clips.ctypes.data, n, nf, out.ctypes.data,
                                                         crops.ctypes.data, dc.ctypes.data if want_dontcare else None))
        return (out, crops, dc) if want_dontcare else (out, crops)

    def hash_clips_letterbox_device(self, d_buf: int, buf_bytes: int, clips: np.ndarray, d_out: int, d_dontcare: int = 0,
                                    frames_per_clip: int = 16, stream: int = 0) -> np.ndarray:
        """vdf_hash_clips_u8_letterbox_device: clips = HOST array of CLIP_DTYPE records with all-zero crop fields; returns the detected boxes
        [n, 4] u32 (the call waits for its detect); clip i's hash goes to d_out + 128 i, ordered on `stream`."""
        c = np.ascontiguousarray(clips, dtype=CLIP_DTYPE)
        crops = np.zeros((c.size, 4), np.uint32)
        self._check(self.lib.vdf_hash_clips_u8_letterbox_device(self.ctx, d_buf, int(buf_bytes), c.ctypes.data if c.size else None, c.size,
                                                                int(frames_per_clip), d_out, d_dontcare or None, crops.ctypes.data, stream or None))
        return crops

    def cropdetect_letterbox_clips_device(self, d_buf: int, buf_bytes: int, clips: np.ndarray, d_crops: int, frames_per_clip: int = 16,
                                          stream: int = 0):
        """vdf_cropdetect_letterbox_clips_device: the boxes of clips of different frame sizes, left on the device (d_crops: [n, 4] u32),
        ordered on `stream`; only queues work."""
        c = np.ascontiguousarray(clips, dtype=CLIP_DTYPE)
        self._check(self.lib.vdf_cropdetect_letterbox_clips_device(self.ctx, d_buf, int(buf_bytes), c.ctypes.data if c.size else None, c.size,
                                                                   int(frames_per_clip), d_crops, stream or None))

    def hash_clips(self, stacks: Sequence[np.ndarray], crops=None, want_dontcare: bool = False):
        """Clips of DIFFERENT frame sizes in one call (vdf_hash_clips_u8): stacks = a list of [>= 16, H, W] u8 arrays, each with its own
        H and W; crops (optional) = [n, 4] u32 left, right, top, bottom per clip.  -> hashes [n, 16] u64 [, dontcare [n] u32], in the
        order of the list.  Raises VdfError(VDF_E_NOT_ENOUGH_FRAMES) when a stack has fewer than 16 frames."""
        buf, clips, nf = self._pack_stacks(stacks)
        n = len(clips)
        if crops is not None:
            clips["crop"] = np.asarray(crops, dtype=np.uint32).reshape(n, 4)
        out = np.zeros((n, HASH_WORDS), np.uint64)
        dc = np.zeros(n, np.uint32) if want_dontcare else None
        self._check(self.lib.vdf_hash_clips_u8(self.ctx, buf.ctypes.data, buf.size, clips.ctypes.data, n, nf, out.ctypes.data,
                                               dc.ctypes.data if want_dontcare else None))
        return (out, dc) if want_dontcare else out

    def hash_clips_device(self, d_buf: int, buf_bytes: int, clips: np.ndarray, d_out: int, d_dontcare: int = 0,
                          frames_per_clip: int = 16, stream: int = 0):
        """vdf_hash_clips_u8_device: clips = HOST array of CLIP_DTYPE records (offsets relative to d_buf), every address checked against
        buf_bytes before anything is queued; clip i's hash goes to d_out + 128 i, ordered on `stream`."""
        c = np.ascontiguousarray(clips, dtype=CLIP_DTYPE)
        self._check(self.lib.vdf_hash_clips_u8_device(self.ctx, d_buf, int(buf_bytes), c.ctypes.data if c.size else None, c.size,
                                                      int(frames_per_clip), d_out, d_dontcare or None, stream or None))

    def hash_frames_letterbox(self, frames: np.ndarray, want_dontcare: bool = False):
        """crop_video_frames(Cropdetect::Letterbox) + from_frames (video_hash_builder.rs:188-223) for a batch:
        frames [n_clips, n_frames >= 16, H, W] u8 -> (hashes [n_clips, 16] u64, crops [n_clips, 4] u32 = l, r, t, b
        [, dontcare])."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim != 4:
            raise ValueError("frames must be [n_clips, n_frames, H, W]")
        nc, nf, h, w = frames.shape
        out = np.zeros((nc, HASH_WORDS), np.uint64)
        crops = np.zeros((nc, 4), np.uint32)
        dc = np.zeros(nc, np.uint32) if want_dontcare else None
        self._check(self.lib.vdf_hash_frames_u8_letterbox(self.ctx, frames.ctypes.data, nc, nf, w, h, w * h, nf * w * h,
                                                          out.ctypes.data, crops.ctypes.data,
                                                          dc.ctypes.data if want_dontcare else None))
        return (out, crops, dc) if want_dontcare else (out, crops)

    def cropdetect_letterbox_device(self, d_frames: int, n_clips: int, frames_per_clip: int, w: int, h: int,
                                    d_crops: int, stream: int = 0, frame_stride: Optional[int] = None,
                                    clip_stride: Optional[int] = None):
        fs = w * h if frame_stride is None else frame_stride
        cs = fs * frames_per_clip if clip_stride is None else clip_stride
        self._check(self.lib.vdf_cropdetect_letterbox_device(self.ctx, d_frames, n_clips, frames_per_clip, w, h, fs, cs,
                                                             d_crops, stream or None))

    def hash_frames_cropped_device(self, d_frames: int, n_clips: int, frames_per_clip: int, w: int, h: int,
                                   crops: Optional[np.ndarray], d_out: int, d_dontcare: int = 0, stream: int = 0):
        c = None if crops is None else np.ascontiguousarray(crops, dtype=np.uint32).reshape(n_clips, 4)
        self._check(self.lib.vdf_hash_frames_u8_cropped_device(self.ctx, d_frames, n_clips, frames_per_clip, w, h, w * h,
                                                               w * h * frames_per_clip,
                                                               c.ctypes.data if c is not None else None, d_out,
                                                               d_dontcare or None, stream or None))

    def hash_frames_letterbox_device(self, d_frames: int, n_clips: int, frames_per_clip: int, w: int, h: int,
                                     d_out: int, d_dontcare: int = 0, stream: int = 0,
                                     frame_stride: Optional[int] = None, clip_stride: Optional[int] = None,
                                     d_crops: Optional[int] = None) -> Optional[np.ndarray]:
        """Cropdetect::Letterbox + from_frames on device frames.  Default: returns the boxes as a host array (the call then ends with a
        wait for its own work).  d_crops = device pointer to n_clips x 4 uint32 (0: the boxes are not wanted): the boxes stay on the
        device, ordered on `stream` like the hashes, and the call only queues work (vdf_hash_frames_u8_letterbox_device_async)."""
        fs = w * h if frame_stride is None else frame_stride
        cs = fs * frames_per_clip if clip_stride is None else clip_stride
        if d_crops is not None:
            self._check(self.lib.vdf_hash_frames_u8_letterbox_device_async(self.ctx, d_frames, n_clips, frames_per_clip, w, h, fs, cs,
                                                                           d_out, d_dontcare or None, d_crops or None, stream or None))
            return None
        crops = np.zeros((n_clips, 4), np.uint32)
        self._check(self.lib.vdf_hash_frames_u8_letterbox_device(self.ctx, d_frames, n_clips, frames_per_clip, w, h,
                                                                 fs, cs, d_out, d_dontcare or None, crops.ctypes.data,
                                                                 stream or None))
        return crops

    # ------------------------------------------------------------------- search
    def search_self_sorted(self, hashes, durations, tol_int: int) -> List[List[int]]:
        """search() on SoA input already in Search::sort order; groups of sorted indices."""
        h = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1, HASH_WORDS)
        d = np.ascontiguousarray(durations, dtype=np.uint32)
        assert h.shape[0] == d.shape[0]
        g = VdfGroups()
        self._check(self.lib.vdf_search_self(self.ctx, h.ctypes.data, d.ctypes.data, len(d), int(tol_int), C.byref(g)))
        try:
            return [m for _, m in _groups_to_lists(g)]
        finally:
            self.lib.vdf_groups_free(C.byref(g))

    def search_refs_sorted(self, cand_hashes, cand_durations, ref_hashes, ref_durations, tol_int: int):
        """search_with_references() on sorted candidates; [(ref_input_index, [candidate indices])]."""
        ch = np.ascontiguousarray(cand_hashes, dtype=np.uint64).reshape(-1, HASH_WORDS)
        cd = np.ascontiguousarray(cand_durations, dtype=np.uint32)
        rh = np.ascontiguousarray(ref_hashes, dtype=np.uint64).reshape(-1, HASH_WORDS)
        rd = np.ascontiguousarray(ref_durations, dtype=np.uint32)
        g = VdfGroups()
        self._check(self.lib.vdf_search_refs(self.ctx, ch.ctypes.data, cd.ctypes.data, len(cd), rh.ctypes.data,
                                             rd.ctypes.data, len(rd), int(tol_int), C.byref(g)))
        try:
            return _groups_to_lists(g)
        finally:
            self.lib.vdf_groups_free(C.byref(g))

    def groups_max_distance(self, hashes, groups: Sequence[Sequence[int]], ref_hashes=None,
                            ref_index: Optional[Sequence[int]] = None) -> np.ndarray:
        """The app's Sorting::Distance key (search_output.rs:43-60): per group, the max Hamming distance over all
        pairs of its members (indices into `hashes`) plus, if given, its reference ref_hashes[ref_index[g]]."""
        h = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1, HASH_WORDS)
        ng = len(groups)
        offs = np.zeros(ng + 1, np.uint64)
        offs[1:] = np.cumsum([len(g) for g in groups]) if ng else []
        mem = np.array([m for g in groups for m in g], dtype=np.uint64)
        if not len(mem):
            mem = np.zeros(1, np.uint64)
        g = VdfGroups()
        g.n_groups = ng
        g.offsets = offs.ctypes.data_as(C.POINTER(C.c_uint64))
        g.members = mem.ctypes.data_as(C.POINTER(C.c_uint64))
        rh = ri = None
        if ref_hashes is not None and ref_index is not None:
            rh = np.ascontiguousarray(ref_hashes, dtype=np.uint64).reshape(-1, HASH_WORDS)
            ri = np.ascontiguousarray(ref_index, dtype=np.int64)
            g.ref_index = ri.ctypes.data_as(C.POINTER(C.c_int64))
        out = np.zeros(ng, np.uint32)
        self._check(self.lib.vdf_groups_max_distance(self.ctx, h.ctypes.data, len(h),
                                                     rh.ctypes.data if rh is not None else None,
                                                     len(rh) if rh is not None else 0, C.byref(g), out.ctypes.data))
        return out

    def pin_database(self, d_hashes: int, n: int):
        """Promise that the n x 16 words at d_hashes stay unchanged (until pin_database(0, 0)): searches against exactly this
        database reuse its operand expansion."""
        self._check(self.lib.vdf_ctx_pin_database(self.ctx, d_hashes or None, int(n)))

    def sort_order_device(self, d_durations: int, n: int, d_perm_out: int, d_path_rank: int = 0, stream: int = 0):
        """Search::sort's permutation (stable by (duration, path rank)) of n device-resident entries into d_perm_out (u32)."""
        self._check(self.lib.vdf_sort_order_device(self.ctx, d_durations, d_path_rank or None, n, d_perm_out, stream or None))

    def apply_order_device(self, d_hashes: int, d_durations: int, d_perm: int, n: int, d_hashes_out: int,
                           d_durations_out: int = 0, stream: int = 0):
        self._check(self.lib.vdf_apply_order_device(self.ctx, d_hashes, d_durations or None, d_perm, n, d_hashes_out,
                                                    d_durations_out or None, stream or None))

    def search_self_device(self, d_hashes: int, d_durations: int, n: int, tol_int: int, shard_index: int = 0,
                           shard_count: int = 1, row_begin: int = 0, row_end: int = UINT32_MAX, d_matched: int = 0,
                           capacity: int = 1 << 22, stream: int = 0):
        """Thresholded adjacency of this shard's row tiles: (hits [k,2] u32 sorted, n_hits, overflow_row)."""
        hits = self._hit_buffer(capacity)  # filled by the library up to n_hits
        n_hits = C.c_uint64(0)
        overflow = C.c_uint32(0)
        self._check(self.lib.vdf_search_self_device(self.ctx, d_hashes, d_durations, n, int(tol_int), shard_index,
                                                    shard_count, row_begin, min(row_end, UINT32_MAX),
                                                    d_matched or None, hits.ctypes.data, capacity, C.byref(n_hits),
                                                    C.byref(overflow), stream or None))
        k = min(int(n_hits.value), capacity)
        return hits[:k].copy(), int(n_hits.value), int(overflow.value)

    def search_self_device_replay(self, d_hashes: int, d_durations: int, n: int, tol_int: int, shard_index: int = 0,
                                  shard_count: int = 1, row_begin: int = 0, row_end: int = UINT32_MAX, d_matched: int = 0,
                                  capacity: int = 1 << 22, stream: int = 0, exchange=None):
        """search_self_device for a caller that only replays the hits (vdf_search_self_device_replay): rows that can never
        become targets are dropped on the device.  `exchange` (sharded launches) is how the shards meet for that:
            exchange.agree(complete: bool, total_hits: int) -> (all_complete, total_hits_of_all_shards)
            exchange.or_bitmap(engine, d_bitmap: int, n_words: int, stream: int)   # OR over the shards, in place, on the device
        Returns (hits [k, 2] u32 sorted, hits kept, overflow_row)."""
        hits = self._hit_buffer(capacity)
        n_hits = C.c_uint64(0)
        overflow = C.c_uint32(0)
        x = None
        errors = []
        if exchange is not None:
            def _agree(_user, p_complete, p_total):
                try:
                    c, t = exchange.agree(bool(p_complete[0]), int(p_total[0]))
                    p_complete[0] = 1 if c else 0
                    p_total[0] = int(t)
                    return 0
                except Exception as e:  # noqa: BLE001 - an exception must not unwind through the C frames
                    errors.append(e)
                    return _capi.VDF_E_INVAL

            def _or(_user, d_bitmap, n_words, strm):
                try:
                    exchange.or_bitmap(self, int(d_bitmap or 0), int(n_words), int(strm or 0))
                    return 0
                except Exception as e:  # noqa: BLE001
                    errors.append(e)
                    return _capi.VDF_E_INVAL

            x = _capi.VdfShardExchange(None, _capi.AGREE_FN(_agree), _capi.OR_BITMAP_FN(_or))
        rc = self.lib.vdf_search_self_device_replay(self.ctx, d_hashes, d_durations, n, int(tol_int), shard_index, shard_count,
                                                    row_begin, min(row_end, UINT32_MAX), d_matched or None, hits.ctypes.data,
                                                    capacity, C.byref(n_hits), C.byref(overflow),
                                                    C.byref(x) if x is not None else None, stream or None)
        if errors:
            raise errors[0]
        self._check(rc)
        k = min(int(n_hits.value), capacity)
        return hits[:k].copy(), int(n_hits.value), int(overflow.value)

    def bitmap_or_device(self, d_dst: int, d_srcs: int, n_words: int, n_srcs: int, stream: int = 0):
        """d_dst[w] |= OR over n_srcs bitmaps of n_words u32 words laid out back to back at d_srcs (device pointers)."""
        self._check(self.lib.vdf_bitmap_or_device(self.ctx, d_dst, d_srcs, int(n_words), int(n_srcs), stream or None))

    def search_refs_device(self, d_cand_hashes: int, d_cand_durations: int, n_cand: int, d_ref_hashes: int,
                           d_ref_durations: int, n_ref: int, tol_int: int, ref_index_base: int = 0,
                           capacity: int = 1 << 22, stream: int = 0):
        """(hits [k,2] u32 sorted by (ref, cand), n_hits).  Grows the buffer once if it was too small."""
        for _ in range(6):
            hits = self._hit_buffer(capacity)
            n_hits = C.c_uint64(0)
            rc = self.lib.vdf_search_refs_device(self.ctx, d_cand_hashes, d_cand_durations, n_cand, d_ref_hashes,
                                                 d_ref_durations, n_ref, int(tol_int), ref_index_base,
                                                 hits.ctypes.data, capacity, C.byref(n_hits), stream or None)
            if rc == _capi.VDF_E_OVERFLOW and int(n_hits.value) > capacity:
                capacity = int(n_hits.value)
                continue
            self._check(rc)
            return hits[: int(n_hits.value)].copy(), int(n_hits.value)
        raise VdfError(_capi.VDF_E_OVERFLOW, "hit buffer overflow")


# ---------------------------------------------------------------- host-only helpers (no GPU needed)
def hamming_distance_words(a, b) -> int:
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(HASH_WORDS)
    b = np.ascontiguousarray(b, dtype=np.uint64).reshape(HASH_WORDS)
    return int(_capi.load().vdf_hamming_u1024(a.ctypes.data_as(C.POINTER(C.c_uint64)),
                                              b.ctypes.data_as(C.POINTER(C.c_uint64))))


def hash_variant(hash_words, zero_words, variant: int) -> np.ndarray:
    """vdf_hash_variant: the hash of the clip flipped by `variant` (0 ... 7) from its hash and zero plane, [16] u64."""
    h = np.ascontiguousarray(hash_words, dtype=np.uint64).reshape(HASH_WORDS)
    z = np.ascontiguousarray(zero_words, dtype=np.uint64).reshape(HASH_WORDS)
    out = np.zeros(HASH_WORDS, np.uint64)
    rc = _capi.load().vdf_hash_variant(h.ctypes.data, z.ctypes.data, int(variant), out.ctypes.data)
    if rc:
        raise VdfError(rc, "vdf_hash_variant: variant must be 0 ... 7")
    return out


def tolerance_int(tolerance: float) -> int:
    return int(_capi.load().vdf_tolerance_int(float(tolerance)))


def count_pairs_self(sorted_durations) -> int:
    d = np.ascontiguousarray(sorted_durations, dtype=np.uint32)
    return int(_capi.load().vdf_count_pairs_self(d.ctypes.data_as(C.POINTER(C.c_uint32)), len(d)))


def count_pairs_refs(sorted_cand_durations, ref_durations) -> int:
    c = np.ascontiguousarray(sorted_cand_durations, dtype=np.uint32)
    r = np.ascontiguousarray(ref_durations, dtype=np.uint32)
    return int(_capi.load().vdf_count_pairs_refs(c.ctypes.data_as(C.POINTER(C.c_uint32)), len(c),
                                                 r.ctypes.data_as(C.POINTER(C.c_uint32)), len(r)))


def replay_self(n: int, hits: np.ndarray, matched: Optional[np.ndarray] = None, row_begin: int = 0,
                row_end: int = UINT32_MAX, groups: Optional[VdfGroups] = None) -> VdfGroups:
    """Host replay of search_self's consumption (search_algorithm.rs:131-170) over hits sorted by (row, col).
    Appends to `groups` (ascending target order); finish with finish_self()."""
    lib = _capi.load()
    hits = np.ascontiguousarray(hits, dtype=np.uint32).reshape(-1, 2)
    g = groups if groups is not None else VdfGroups()
    rc = lib.vdf_replay_self(n, hits.ctypes.data, len(hits), row_begin, min(row_end, UINT32_MAX),
                             matched.ctypes.data if matched is not None else None, C.byref(g))
    if rc:
        raise VdfError(rc, "vdf_replay_self failed")
    return g


def finish_self(groups: VdfGroups) -> List[List[int]]:
    lib = _capi.load()
    rc = lib.vdf_groups_finish_self(C.byref(groups))
    if rc:
        raise VdfError(rc, "vdf_groups_finish_self failed")
    try:
        return [m for _, m in _groups_to_lists(groups)]
    finally:
        lib.vdf_groups_free(C.byref(groups))


def sort_hits(hits: np.ndarray) -> np.ndarray:
    """[k, 2] uint32 hits into (row, col) order (C++ radix sort; np.lexsort needs seconds for 1e7 hits)."""
    hits = np.ascontiguousarray(hits, dtype=np.uint32).reshape(-1, 2)
    if not hits.flags.writeable:
        hits = hits.copy()
    rc = _capi.load().vdf_sort_hits(hits.ctypes.data, len(hits))
    if rc:
        raise VdfError(rc, "vdf_sort_hits failed")
    return hits


def ref_groups_csr(hits: np.ndarray):
    """search_with_references groups as arrays (offsets u64[g + 1], members u64[m], ref_index i64[g]) from sorted hits."""
    lib = _capi.load()
    hits = np.ascontiguousarray(hits, dtype=np.uint32).reshape(-1, 2)
    g = VdfGroups()
    rc = lib.vdf_groups_from_ref_hits(hits.ctypes.data, len(hits), C.byref(g))
    if rc:
        raise VdfError(rc, "vdf_groups_from_ref_hits failed")
    try:
        return groups_to_arrays(g)
    finally:
        lib.vdf_groups_free(C.byref(g))


def groups_from_ref_hits(hits: np.ndarray) -> List[Tuple[int, List[int]]]:
    lib = _capi.load()
    hits = np.ascontiguousarray(hits, dtype=np.uint32).reshape(-1, 2)
    g = VdfGroups()
    rc = lib.vdf_groups_from_ref_hits(hits.ctypes.data, len(hits), C.byref(g))
    if rc:
        raise VdfError(rc, "vdf_groups_from_ref_hits failed")
    try:
        return _groups_to_lists(g)
    finally:
        lib.vdf_groups_free(C.byref(g))


class HashQueue:
    """Thread-safe batching of per-clip hash requests (vdf_hash_queue_*): concurrent submit()
    calls from many threads share one batched GPU launch.  One queue per frame size."""

    def __init__(self, engine: Engine, w: int, h: int, max_batch: int = 256, max_wait_us: int = 2000,
                 letterbox: bool = False):
        self.engine = engine
        self.w, self.h = int(w), int(h)
        q = C.c_void_p()
        engine._check(engine.lib.vdf_hash_queue_create(engine.ctx, self.w, self.h, int(max_batch), int(max_wait_us),
                                                       1 if letterbox else 0, C.byref(q)))
        self.q = q

    def submit(self, frames: np.ndarray):
        """frames [>=16, H, W] u8 -> (hash [16] u64, crop (l, r, t, b)).  Blocks; releases the GIL while waiting."""
        f = np.ascontiguousarray(frames[:16], dtype=np.uint8)
        if f.shape != (16, self.h, self.w):
            raise ValueError("a queue takes 16 frames of its own frame size")
        out = np.zeros(HASH_WORDS, np.uint64)
        crop = np.zeros(4, np.uint32)
        self.engine._check(self.engine.lib.vdf_hash_queue_submit(self.q, f.ctypes.data, out.ctypes.data, crop.ctypes.data))
        return out, tuple(int(x) for x in crop)

    def stats(self):
        nb, nc = C.c_uint64(0), C.c_uint64(0)
        self.engine.lib.vdf_hash_queue_stats(self.q, C.byref(nb), C.byref(nc))
        return int(nb.value), int(nc.value)

    def in_flight_max(self) -> int:
        v = C.c_uint32(0)
        self.engine.lib.vdf_hash_queue_in_flight_max(self.q, C.byref(v))
        return int(v.value)

    def close(self):
        if getattr(self, "q", None):
            self.engine.lib.vdf_hash_queue_destroy(self.q)
            self.q = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MixedHashQueue:
    """HashQueue for clips of ANY frame size (vdf_hash_queue_mixed_*): one queue serves a whole library.  A batch closes at max_batch clips,
    at staging_bytes of frames, or when its first caller has waited max_wait_us."""

    def __init__(self, engine: Engine, staging_bytes: int = 64 << 20, max_batch: int = 256, max_wait_us: int = 2000, slots_per_gpu: int = 0,
                 letterbox: bool = False):
        self.engine = engine
        self.letterbox = bool(letterbox)
        q = C.c_void_p()
        create = engine.lib.vdf_hash_queue_create_mixed_letterbox if self.letterbox else engine.lib.vdf_hash_queue_create_mixed
        engine._check(create(engine.ctx, int(staging_bytes), int(max_batch), int(max_wait_us), int(slots_per_gpu), C.byref(q)))
        self.q = q

    def submit(self, frames: np.ndarray):
        """frames [>=16, H, W] u8 -> hash [16] u64; a letterbox queue: (hash, crop (l, r, t, b)), as HashQueue.submit.  Blocks; releases the
        GIL while waiting."""
        if self.letterbox:
            return self.submit_crop(frames)
        f = np.ascontiguousarray(frames[:16], dtype=np.uint8)
        if f.ndim != 3 or f.shape[0] != 16:
            raise ValueError("a clip is at least 16 frames of [H, W]")
        out = np.zeros(HASH_WORDS, np.uint64)
        rc = self.engine.lib.vdf_hash_queue_mixed_submit(self.q, f.ctypes.data, f.shape[2], f.shape[1], out.ctypes.data)
        if rc != 0:
            raise VdfError(rc, "mixed hash queue: clip of %d x %d refused or its batch failed" % (f.shape[2], f.shape[1]))
        return out

    def submit_crop(self, frames: np.ndarray):
        """vdf_hash_queue_mixed_submit_crop on either kind of queue: (hash [16] u64, crop (l, r, t, b)); a plain queue's crop is all zero."""
        f = np.ascontiguousarray(frames[:16], dtype=np.uint8)
        if f.ndim != 3 or f.shape[0] != 16:
            raise ValueError("a clip is at least 16 frames of [H, W]")
        out = np.zeros(HASH_WORDS, np.uint64)
        crop = np.zeros(4, np.uint32)
        rc = self.engine.lib.vdf_hash_queue_mixed_submit_crop(self.q, f.ctypes.data, f.shape[2], f.shape[1], out.ctypes.data, crop.ctypes.data)
        if rc != 0:
            raise VdfError(rc, "mixed hash queue: clip of %d x %d refused or its batch failed" % (f.shape[2], f.shape[1]))
        return out, tuple(int(x) for x in crop)

    def stats(self):
        nb, nc = C.c_uint64(0), C.c_uint64(0)
        self.engine.lib.vdf_hash_queue_mixed_stats(self.q, C.byref(nb), C.byref(nc))
        return int(nb.value), int(nc.value)

    def in_flight_max(self) -> int:
        v = C.c_uint32(0)
        self.engine.lib.vdf_hash_queue_mixed_in_flight_max(self.q, C.byref(v))
        return int(v.value)

    def close(self):
        if getattr(self, "q", None):
            self.engine.lib.vdf_hash_queue_mixed_destroy(self.q)
            self.q = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
