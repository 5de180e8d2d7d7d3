"""Python mirror of the reference crate's public surface for the hot path
(vid_dup_finder_lib/src/lib.rs:132-140): VideoHash, MatchGroup, Error, search,
search_with_references.  Same names, argument meaning and error behaviour; the compute goes
through the C ABI to the GPU.  The Rust-side shim a maintainer would add is in INTEGRATION.md.

Out of scope here (callers of the path, decode-bound): VideoHashBuilder / CreationOptions
(video_hash_builder.rs) -- their output contract (16 equal-size gray frames + duration in
seconds) is exactly the input of VideoHash.from_frames below.
"""
from __future__ import annotations

import enum
import itertools
import os
import math
from typing import Iterable, Iterator, List, NamedTuple, Optional, Sequence

import numpy as np

from . import _capi
from ._capi import DEFAULT_SEARCH_TOLERANCE, HASH_BITS, HASH_WORDS, TOLERANCE_SCALING_FACTOR, VdfError
from .engine import (ALIGN_DTYPE, ALIGN_STRETCH_DTYPE, ALIGN_VARIANT_DTYPE, Engine, align_windows_host, align_windows_stretches_host, align_windows_variants_host, hamming_distance_words, hash_variant,
                     tolerance_int, video_pairs, align_seed_pairs_host, align_windows_pairs_host, align_windows_stretches_pairs_host,
                     ALIGN_RETIMED_DTYPE, VIDEO_PAIR_DTYPE, align_windows_retimed_host, align_windows_retimed_pairs_host,
                     pair_list_problem, VIDEO_PAIR_VARIANT_DTYPE, align_seed_pairs_variants_host, align_windows_variants_pairs_host,
                     VIDEO_PAIR_RATE_DTYPE, align_seed_pairs_rates_host, ALIGN_RATE_DTYPE, align_windows_rates_host, ALIGN_RATE_STRETCH_DTYPE,
                     align_windows_rates_stretches_host)

__all__ = ["Crop", "Cropdetect", "cropdetect_letterbox", "gen_hashes", "VideoHash", "MatchGroup", "Error", "NotEnoughFrames", "NotVideo", "VidProc", "TooFewEntries", "search",
           "search_with_references", "search_flipped", "Flip", "default_engine", "hash_frame_stacks", "hash_frame_windows", "align_rates", "best_rates", "align_rates_all", "best_rates_all", "RetimedAlignmentStretch", "candidate_pairs_rates", "locate", "rust_path_key", "sort_order",
           "DEFAULT_SEARCH_TOLERANCE", "TOLERANCE_SCALING_FACTOR"]


# ---- Error (vid_dup_finder_lib/src/video_hashing/mod.rs:17-28) --------------------------------------
class Error(Exception):
    """An error that prevented a video hash from being created."""


class NotVideo(Error):
    def __init__(self):
        super().__init__("File is not a video")


class VidProc(Error):
    def __init__(self, msg: str):
        super().__init__(f"Video processing error: {msg}")


class NotEnoughFrames(Error):
    def __init__(self):
        super().__init__("Could not extract enough frames")


class Cropdetect(enum.Enum):
    """vid_dup_finder_lib/src/definitions.rs:47-54.  Motion-based detection (vid_dup_finder_common/src/motioncrop/)
    is not on the accelerated path."""
    NONE = "none"
    LETTERBOX = "letterbox"
    MOTION = "motion"


class Flip(enum.IntFlag):
    """Which way a clip is flipped: X = mirrored along the width, Y = flipped along the height, T = its 16 frames reversed; any
    combination (the `variant` of include/vdf.h: vdf_hash_variant)."""
    X = 1
    Y = 2
    T = 4


class Crop:
    """The crop box of a frame as edge offsets (vid_dup_finder_common/src/crop.rs:3-10): what the letterbox detection yields and
    what crop_resize_buf takes.  On the C ABI a box is the four u32 {left, right, top, bottom} (`out_crops`); this is its host-side
    type with the reference's constructors, checks and accessors.  Ordered like the derive: orig_res, left, right, top, bottom."""

    __slots__ = ("orig_res", "left", "right", "top", "bottom")
    _U32 = 0xFFFFFFFF

    def __init__(self, orig_res, left: int, right: int, top: int, bottom: int):
        self.orig_res = (int(orig_res[0]), int(orig_res[1]))
        self.left, self.right, self.top, self.bottom = int(left), int(right), int(top), int(bottom)

    @classmethod
    def from_edge_offsets(cls, orig_res, left: int, right: int, top: int, bottom: int) -> "Crop":
        """crop.rs:13-30: a box that leaves no pixel is a panic there, an AssertionError here."""
        assert left + right < orig_res[0], "crop box leaves no columns"
        assert top + bottom < orig_res[1], "crop box leaves no rows"
        return cls(orig_res, left, right, top, bottom)

    @classmethod
    def from_topleft_and_dims(cls, orig_res, x: int, y: int, width: int, height: int) -> "Crop":
        """crop.rs:32-50 (u32 arithmetic: a box that sticks out of the frame underflows there; refused here)."""
        right, bottom = orig_res[0] - width - x, orig_res[1] - height - y
        if right < 0 or bottom < 0:
            raise OverflowError("box outside the frame")
        return cls(orig_res, x, right, y, bottom)

    @classmethod
    def from_abi(cls, orig_res, box) -> "Crop":
        """One row {left, right, top, bottom} of the C ABI's `out_crops`."""
        return cls.from_edge_offsets(orig_res, int(box[0]), int(box[1]), int(box[2]), int(box[3]))

    @classmethod
    def default(cls) -> "Crop":
        """crop.rs:183-194: an 'enormous' crop to start a fold of unions with."""
        return cls((cls._U32, cls._U32), cls._U32 // 8, cls._U32 // 8, cls._U32 // 8, cls._U32 // 8)

    def union(self, other: "Crop") -> "Crop":
        """crop.rs:53-68: per-edge minimum (what unites the crops of the probed frames; the resolutions are not compared)."""
        return Crop.from_edge_offsets(self.orig_res, min(self.left, other.left), min(self.right, other.right),
                                      min(self.top, other.top), min(self.bottom, other.bottom))

    def as_view_args(self):
        """crop.rs:92-103: (x, y, width, height) of the box - the arguments of crop_resize_buf's .crop()."""
        w, h = self.orig_res[0] - (self.left + self.right), self.orig_res[1] - (self.top + self.bottom)
        if w < 0 or h < 0:
            raise OverflowError("crop offsets exceed the frame")  # checked_sub(..).unwrap()
        return (self.left, self.top, w, h)

    def as_abi(self) -> np.ndarray:
        return np.array([self.left, self.right, self.top, self.bottom], np.uint32)

    def width(self) -> int:
        return self.orig_res[0] - (self.left + self.right)

    def height(self) -> int:
        return self.orig_res[1] - (self.top + self.bottom)

    def area(self) -> int:
        return self.width() * self.height()

    def aspect_ratio(self) -> float:
        return float(self.width()) / float(self.height())

    def enumerate_coords(self) -> Iterator:
        """crop.rs:121-135: the box's (x, y), x outermost."""
        for x in range(self.left, self.orig_res[0] - self.right):
            for y in range(self.top, self.orig_res[1] - self.bottom):
                yield (x, y)

    def enumerate_coords_excluded(self) -> Iterator:
        """crop.rs:137-161: the (x, y) outside the box, the eight surrounding regions clockwise from the top left."""
        xs = (0, self.left, self.orig_res[0] - self.right, self.orig_res[0])
        ys = (0, self.top, self.orig_res[1] - self.bottom, self.orig_res[1])
        for xi, yi in ((0, 0), (1, 0), (2, 0), (2, 1), (0, 2), (1, 2), (2, 2), (0, 1)):
            for x in range(xs[xi], xs[xi + 1]):
                for y in range(ys[yi], ys[yi + 1]):
                    yield (x, y)

    def eroded(self) -> Optional["Crop"]:
        """crop.rs:163-176: one pixel more off every edge, None when nothing would be left."""
        if self.left + self.right + 2 >= self.orig_res[0] or self.top + self.bottom + 2 >= self.orig_res[1]:
            return None
        return Crop(self.orig_res, self.left + 1, self.right + 1, self.top + 1, self.bottom + 1)

    def is_uncropped(self) -> bool:
        return self.left == 0 and self.right == 0 and self.top == 0 and self.bottom == 0

    def _key(self):
        return (self.orig_res, self.left, self.right, self.top, self.bottom)

    def __eq__(self, other):
        return isinstance(other, Crop) and self._key() == other._key()

    def __lt__(self, other):
        return self._key() < other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"Crop(orig_res={self.orig_res}, left={self.left}, right={self.right}, top={self.top}, bottom={self.bottom})"


class TooFewEntries(Exception):
    """match_group.rs:15-16"""


_default_engine: Optional[Engine] = None


def default_engine() -> Engine:
    """Process-wide engine on GPU LOCAL_RANK (or 0).  Fails loudly without a GPU or the built library."""
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine()
    return _default_engine


# ---- Rust `PathBuf: Ord` --------------------------------------------------------------------------
def rust_path_key(path) -> tuple:
    """Key reproducing std::path::Path's component-wise ordering on Unix (Search::sort uses
    (duration, src_path.to_owned()) as its key, search_algorithm.rs:55-61).  Components:
    RootDir < CurDir < ParentDir < Normal(bytes); repeated '/' and inner '.' are not components."""
    b = path if isinstance(path, bytes) else os.fsencode(path)
    comps = []
    if b.startswith(b"/"):
        comps.append((1, b""))
    elif b == b"." or b.startswith(b"./"):
        comps.append((2, b""))
    for part in b.split(b"/"):
        if part in (b"", b"."):
            continue
        comps.append((3, b"") if part == b".." else (4, part))
    return tuple(comps)


def sort_order(hashes: Sequence["VideoHash"], engine: Optional[Engine] = None) -> List[int]:
    """Stable permutation that Search::sort applies (search_algorithm.rs:55-61).  With an engine and more than a handful of hashes the
    order comes from the library (vdf_sort_order_paths: the path half on the device for plain paths, the native component comparator
    otherwise - the same order): a million Python keys cost seconds beside a 0.1 s search."""
    if engine is not None and len(hashes) >= 2048:
        from .cache import sort_order_paths

        order, _used_device = sort_order_paths(engine, [h.duration() for h in hashes], [h.src_path() for h in hashes])
        return order.tolist()
    idx = list(range(len(hashes)))
    idx.sort(key=lambda i: (hashes[i].duration(), rust_path_key(hashes[i].src_path())))
    return idx


# ---- VideoHash (video_hash.rs:26-32) ----------------------------------------------------------------
class VideoHash:
    """hash: 16 x u64 (1024 bits, Lsb0; bits 1000..1023 are zero when built from frames),
    src_path, duration in seconds.
    zero (optional, not in the reference): the clip's zero plane, 16 x u64 with bit i set iff DCT coefficient i is exactly 0.0 -
    what flipped() needs.  Hashes made with zero_plane=True carry it; the hash cache's wire format has no room for it, so hashes
    loaded from a cache cannot be flipped.  It takes no part in comparisons or ordering."""

    __slots__ = ("hash", "_src_path", "_duration", "zero")

    def __init__(self, hash_words=None, src_path="", duration: int = 0, zero=None):
        if hash_words is None:
            hash_words = np.zeros(HASH_WORDS, np.uint64)  # Default, video_hash.rs:34-42
        self.hash = np.ascontiguousarray(hash_words, dtype=np.uint64).reshape(HASH_WORDS).copy()
        self._src_path = src_path
        self._duration = int(duration)
        self.zero = None if zero is None else np.ascontiguousarray(zero, dtype=np.uint64).reshape(HASH_WORDS).copy()

    def flipped(self, flip) -> "VideoHash":
        """The VideoHash the same pipeline gives for the flipped clip (Flip.X: mirrored, Flip.Y: upside down, Flip.T: reversed, or any
        combination), derived from this hash and its zero plane alone - bit for bit what hashing the flipped frames gives.  Same path
        and duration; the zero plane of a flipped clip is the clip's own."""
        if self.zero is None:
            raise VidProc("this VideoHash carries no zero plane (hash with zero_plane=True; hashes loaded from a cache have none)")
        v = int(flip)
        if not 0 <= v <= 7:
            raise ValueError("flip must be a combination of Flip.X, Flip.Y, Flip.T")
        return VideoHash(hash_variant(self.hash, self.zero, v), self._src_path, self._duration, self.zero)

    @classmethod
    def from_frames(cls, frames: Iterable[np.ndarray], src_path, duration: int,
                    engine: Optional[Engine] = None) -> "VideoHash":
        """video_hash.rs:45-73.  frames: iterable of equal-size 2-D u8 arrays (gray, row-major).
        Empty or fewer than 16 -> NotEnoughFrames; only the first 16 are used (dct_3d.rs:25)."""
        taken = list(itertools.islice(iter(frames), _capi.DCT_SIZE))
        if len(taken) < _capi.DCT_SIZE:
            raise NotEnoughFrames()
        first = np.asarray(taken[0])
        for f in taken:
            if np.asarray(f).shape != first.shape or np.asarray(f).ndim != 2:
                raise VidProc("frames must be equal-size 2-D gray images")
        stack = np.stack([np.ascontiguousarray(f, dtype=np.uint8) for f in taken])[None]
        try:
            words = (engine or default_engine()).hash_frames(stack)[0]
        except VdfError as e:
            if e.code == _capi.VDF_E_NOT_ENOUGH_FRAMES:
                raise NotEnoughFrames() from e
            if e.code == _capi.VDF_E_BAD_DIMS:
                raise VidProc(str(e)) from e
            raise
        return cls(words, src_path, duration)

    def src_path(self):
        return self._src_path

    def duration(self) -> int:
        return self._duration

    def hamming_distance(self, other: "VideoHash") -> int:
        """video_hash.rs:190-192: raw distance over all 16 words."""
        return hamming_distance_words(self.hash, other.hash)

    def normalized_hamming_distance(self, other: "VideoHash") -> float:
        """video_hash.rs:200-204 (feature app_only_fns)."""
        return float(self.hamming_distance(other)) / TOLERANCE_SCALING_FACTOR

    def hash_bits(self) -> np.ndarray:
        """The 1000 hash bits as a bool array (video_hash.rs:226-228)."""
        bits = np.unpackbits(self.hash.view(np.uint8), bitorder="little")
        return bits[:HASH_BITS].astype(bool)

    # test_util-style constructors (video_hash.rs:240-308) that need no RNG
    def with_duration(self, duration: int) -> "VideoHash":
        return VideoHash(self.hash, self._src_path, duration, self.zero)

    def with_src_path(self, src_path) -> "VideoHash":
        return VideoHash(self.hash, src_path, self._duration, self.zero)

    @classmethod
    def full_hash(cls, name) -> "VideoHash":
        return cls(np.full(HASH_WORDS, np.uint64(0xFFFFFFFFFFFFFFFF)), name, 0)

    @classmethod
    def empty_hash(cls, name) -> "VideoHash":
        return cls(np.zeros(HASH_WORDS, np.uint64), name, 0)

    # test_util constructors that draw random bits (video_hash.rs:272-306); rng = numpy Generator in place of StdRng
    @classmethod
    def random_hash(cls, rng: np.random.Generator) -> "VideoHash":
        """1000 fair bits, padding bits 1000..1023 zero, empty path, duration 0 (video_hash.rs:293-306)."""
        bits = rng.integers(0, 2, size=HASH_WORDS * 64, dtype=np.uint8)
        bits[HASH_BITS:] = 0
        return cls(np.packbits(bits, bitorder="little").view(np.uint64).copy(), "", 0)

    def hash_with_spatial_distance(self, target_distance: int, rng: np.random.Generator) -> "VideoHash":
        """A hash at exactly `target_distance` bits from this one; any of the 1024 positions may flip, padding included
        (video_hash.rs:272-291).  Upstream random-walks single flips until the distance is first reached, which never
        terminates in practice beyond the 512-bit equilibrium; by symmetry the first-hit point is uniform on the sphere of
        that radius, which `target_distance` distinct random positions sample directly."""
        if not 0 <= target_distance <= HASH_WORDS * 64:
            raise ValueError("target_distance must be within 0..1024")
        bits = np.unpackbits(self.hash.view(np.uint8), bitorder="little")
        bits[rng.choice(HASH_WORDS * 64, size=target_distance, replace=False)] ^= 1
        out = VideoHash(np.packbits(bits, bitorder="little").view(np.uint64).copy(), self._src_path, self._duration)
        assert self.hamming_distance(out) == target_distance
        return out

    def _key(self):
        return (tuple(int(x) for x in self.hash), rust_path_key(self._src_path), self._duration)

    def __eq__(self, other):
        return isinstance(other, VideoHash) and self._key() == other._key()

    def __lt__(self, other):  # derive(Ord): field order hash, src_path, duration
        return self._key() < other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"VideoHash(src_path={self._src_path!r}, duration={self._duration}, hash=0x{int(self.hash[0]):016x}..)"


# ---- MatchGroup (matches/match_group.rs) --------------------------------------------------------------
class MatchGroup:
    __slots__ = ("_reference", "_duplicates")

    def __init__(self, reference, duplicates: List):
        self._reference = reference
        self._duplicates = list(duplicates)

    @classmethod
    def new(cls, entries: Iterable) -> "MatchGroup":
        dups = list(entries)
        if len(dups) < 2:  # match_group.rs:25
            raise TooFewEntries()
        return cls(None, dups)

    @classmethod
    def new_with_reference(cls, reference, entries: Iterable) -> "MatchGroup":
        dups = list(entries)
        if not dups:  # match_group.rs:41
            raise TooFewEntries()
        return cls(reference, dups)

    def len(self) -> int:
        return len(self._duplicates)

    __len__ = len

    def reference(self):
        return self._reference

    def duplicates(self) -> Iterator:
        return iter(self._duplicates)

    def contained_paths(self) -> Iterator:
        """duplicates, then the reference if there is one (match_group.rs:68-81)."""
        yield from self._duplicates
        if self._reference is not None:
            yield self._reference

    def dup_combinations(self) -> List["MatchGroup"]:
        """match_group.rs:87-105."""
        if self._reference is not None:
            return [MatchGroup.new_with_reference(self._reference, [d]) for d in self._duplicates]
        return [MatchGroup.new([a, b]) for a, b in itertools.combinations(self._duplicates, 2)]

    def __eq__(self, other):
        return (isinstance(other, MatchGroup) and self._reference == other._reference
                and self._duplicates == other._duplicates)

    def __repr__(self):
        return f"MatchGroup(reference={self._reference!r}, duplicates={self._duplicates!r})"


# ---- search / search_with_references (video_dup_finder.rs) -------------------------------------------
def _soa(hashes: Sequence[VideoHash], order: Sequence[int]):
    if not order:
        return np.zeros((0, HASH_WORDS), np.uint64), np.zeros(0, np.uint32)
    # (one bytes object of all words: half the time of np.stack over a million 16-word arrays)
    words = np.frombuffer(b"".join([hashes[i].hash.tobytes() for i in order]), np.uint64).reshape(-1, HASH_WORDS)
    dur = np.array([hashes[i].duration() for i in order], dtype=np.uint32)
    return words, dur


def search(hashes: Iterable[VideoHash], tolerance: float, engine: Optional[Engine] = None) -> List[MatchGroup]:
    """video_dup_finder.rs:7-13.  Sort (host, needs paths), GPU all-pairs search inside the one-sided
    x1.1 duration window, host replay of the greedy consumption; groups come back in the reference's order."""
    hashes = list(hashes)
    if not hashes:
        return []  # search_algorithm.rs:89-91
    engine = engine or default_engine()
    order = sort_order(hashes, engine)
    words, dur = _soa(hashes, order)
    groups = engine.search_self_sorted(words, dur, tolerance_int(tolerance))
    out = []
    for g in groups:
        try:
            out.append(MatchGroup.new(hashes[order[m]].src_path() for m in g))
        except TooFewEntries:  # filter_map(.. .ok()), video_dup_finder.rs:11
            pass
    return out


def search_with_references(ref_hashes: Iterable[VideoHash], new_hashes: Iterable[VideoHash], tolerance: float,
                           engine: Optional[Engine] = None) -> List[MatchGroup]:
    """video_dup_finder.rs:19-46: one group per reference with >= 1 match, in reference input order."""
    refs = list(ref_hashes)
    news = list(new_hashes)
    if not refs or not news:
        return []
    engine = engine or default_engine()
    order = sort_order(news, engine)
    words, dur = _soa(news, order)
    rwords, rdur = _soa(refs, list(range(len(refs))))
    res = engine.search_refs_sorted(words, dur, rwords, rdur, tolerance_int(tolerance))
    return [MatchGroup.new_with_reference(refs[r].src_path(), [news[order[m]].src_path() for m in ms])
            for r, ms in res]


def search_flipped(hashes: Iterable[VideoHash], tolerance: float, flips: Sequence = (Flip.X,), engine: Optional[Engine] = None) -> dict:
    """Mirrored / flipped / reversed duplicates, which the reference cannot see (vid_dup_finder_lib/src/lib.rs:102-111):
    {flip: [MatchGroup]} for every flip of `flips`.  A group's reference is the path of an entry r, its duplicates the paths of the
    entries whose hash is within `tolerance` of the hash of r FLIPPED, inside r's +-5 % duration window (search_one's, as
    search_with_references); r itself is never among them, and entries whose flip matches nothing have no group.  Groups are in
    Search::sort order of their reference.  A pair usually shows from both sides (a in the group of b and b in the group of a).
    Every hash needs its zero plane (zero_plane=True when hashing), else VidProc."""
    hashes = list(hashes)
    flips = [Flip(int(f)) for f in flips]
    if any(not 1 <= int(f) <= 7 for f in flips):
        raise ValueError("flips are non-empty combinations of Flip.X, Flip.Y, Flip.T")
    if any(h.zero is None for h in hashes):
        raise VidProc("search_flipped needs the zero plane of every hash (hash with zero_plane=True)")
    if not hashes or not flips:
        return {f: [] for f in flips}
    engine = engine or default_engine()
    order = sort_order(hashes, engine)
    words, dur = _soa(hashes, order)
    zero = np.stack([hashes[i].zero for i in order])
    mask = 0
    for f in flips:
        mask |= 1 << int(f)
    res = engine.search_variants_sorted(words, zero, dur, tolerance_int(tolerance), mask)
    return {f: [MatchGroup.new_with_reference(hashes[order[r]].src_path(), [hashes[order[m]].src_path() for m in ms]) for r, ms in res[int(f)]]
            for f in flips}


def _with_planes(call):
    try:
        return call()
    except VdfError as e:
        if e.code == _capi.VDF_E_NOT_ENOUGH_FRAMES:
            raise NotEnoughFrames() from e
        if e.code == _capi.VDF_E_BAD_DIMS:
            raise VidProc(str(e)) from e
        raise


def hash_frame_stacks(frames: np.ndarray, src_paths: Sequence, durations: Sequence[int],
                      engine: Optional[Engine] = None, zero_plane: bool = False) -> List[VideoHash]:
    """Batched VideoHash.from_frames: frames [n_clips, n_frames >= 16, H, W] u8 -> one VideoHash per clip
    (the batching a caller of VideoHashBuilder::hash would do to feed the GPU).
    frames may also be a LIST of [n_frames >= 16, H, W] stacks of different frame sizes (files arrive in whatever resolution they
    have): they are hashed by one call all the same (Engine.hash_clips).
    zero_plane: the hashes also carry their zero plane (VideoHash.zero; Engine.hash_frames_planes / hash_clips_planes), so that
    VideoHash.flipped and search_flipped work on them; the hash words are the same."""
    if zero_plane:
        eng = engine or default_engine()
        words, zero = _with_planes(lambda: eng.hash_clips_planes(frames) if isinstance(frames, (list, tuple)) else eng.hash_frames_planes(frames))
        return [VideoHash(words[i], src_paths[i], durations[i], zero[i]) for i in range(len(words))]
    try:
        eng = engine or default_engine()
        words = eng.hash_clips(frames) if isinstance(frames, (list, tuple)) else eng.hash_frames(frames)
    except VdfError as e:
        if e.code == _capi.VDF_E_NOT_ENOUGH_FRAMES:
            raise NotEnoughFrames() from e
        raise
    return [VideoHash(words[i], src_paths[i], durations[i]) for i in range(len(words))]


def _hash_frame_windows_mixed(stacks, src_paths, durations, stride, engine, zero_plane, crops, letterbox) -> List[List[VideoHash]]:
    """hash_frame_windows on a list of stacks: one Engine.hash_windows_clips[_planes] call, cut into per-video lists at first[]."""
    if crops is not None and letterbox:
        raise ValueError("crops and letterbox=True are two sources of the same boxes")
    eng = engine or default_engine()
    stacks = list(stacks)

    def call():
        boxes = None
        if crops is not None:
            if len(crops) != len(stacks):
                raise ValueError("a Crop per video")
            boxes = np.stack([c.as_abi() if isinstance(c, Crop) else np.asarray(c, np.uint32).reshape(4) for c in crops]).reshape(-1, 4) if len(stacks) else None
        elif letterbox and stacks:  # the boxes of frames 0 and 8 of every video, by the mixed letterbox call (which hashes frames 0 .. 15 beside them)
            boxes = eng.hash_clips_letterbox(stacks)[1]
        if zero_plane:
            words, zero, first = eng.hash_windows_clips_planes(stacks, stride, crops=boxes)
        else:
            (words, first), zero = eng.hash_windows_clips(stacks, stride, crops=boxes), None
        return words, zero, first

    words, zero, first = _with_planes(call)
    return [[VideoHash(words[r], src_paths[i], durations[i], None if zero is None else zero[r]) for r in range(int(first[i]), int(first[i + 1]))]
            for i in range(len(stacks))]


def _hash_frame_windows_retimed(frames, src_paths, durations, stride, engine, rate):
    """hash_frame_windows at a rate: one Engine.hash_windows_retimed call for a 4-D array, one uniform call per video for a list of stacks."""
    eng = engine or default_engine()
    try:
        if isinstance(frames, (list, tuple)):
            words = [eng.hash_windows_retimed(np.asarray(st)[None], rate, stride)[0] for st in frames]
        else:
            words = eng.hash_windows_retimed(frames, rate, stride)
    except VdfError as e:
        if e.code == _capi.VDF_E_NOT_ENOUGH_FRAMES:
            raise NotEnoughFrames() from e
        raise
    return [[VideoHash(w[k], src_paths[i], durations[i]) for k in range(len(w))] for i, w in enumerate(words)]


def _hash_frame_windows_rates(frames, src_paths, durations, stride, engine, rates) -> dict:
    """hash_frame_windows at several rates: one Engine.hash_windows_rates call for a 4-D array, one uniform call per video for a list of stacks."""
    eng = engine or default_engine()
    rates = [tuple(r) for r in rates]
    try:
        if isinstance(frames, (list, tuple)):
            per_video = [eng.hash_windows_rates(np.asarray(st)[None], rates, stride) for st in frames]
            words = [[pv[r][0] for pv in per_video] for r in range(len(rates))]
        else:
            words = eng.hash_windows_rates(frames, rates, stride)
    except VdfError as e:
        if e.code == _capi.VDF_E_NOT_ENOUGH_FRAMES:
            raise NotEnoughFrames() from e
        raise
    return {rate: [[VideoHash(w[k], src_paths[i], durations[i]) for k in range(len(w))] for i, w in enumerate(words[r])] for r, rate in enumerate(rates)}


def _hash_frame_windows_retimed_library(stacks, src_paths, durations, stride, engine, rate, crops, letterbox) -> List[List[VideoHash]]:
    """hash_frame_windows(list, rate=, one_call=True): ONE Engine.hash_windows_clips_retimed call for the library, cut into per-video lists at
    first[].  The boxes as _hash_frame_windows_mixed finds them."""
    if crops is not None and letterbox:
        raise ValueError("crops and letterbox=True are two sources of the same boxes")
    eng = engine or default_engine()
    stacks = list(stacks)

    def call():
        boxes = None
        if crops is not None:
            if len(crops) != len(stacks):
                raise ValueError("a Crop per video")
            boxes = np.stack([c.as_abi() if isinstance(c, Crop) else np.asarray(c, np.uint32).reshape(4) for c in crops]).reshape(-1, 4) if len(stacks) else None
        elif letterbox and stacks:  # the boxes of frames 0 and 8 of every video, by the mixed letterbox call
            boxes = eng.hash_clips_letterbox(stacks)[1]
        return eng.hash_windows_clips_retimed(stacks, rate, stride, crops=boxes)

    words, first = _with_planes(call)
    return [[VideoHash(words[r], src_paths[i], durations[i]) for r in range(int(first[i]), int(first[i + 1]))] for i in range(len(stacks))]


def _hash_frame_windows_rates_library(stacks, src_paths, durations, stride, engine, rates, crops, letterbox) -> dict:
    """hash_frame_windows(list, rates=, one_call=True): ONE Engine.hash_windows_clips_rates call for the library and all its rates, every block
    cut into per-video lists at first[r].  The boxes as _hash_frame_windows_retimed_library finds them."""
    if crops is not None and letterbox:
        raise ValueError("crops and letterbox=True are two sources of the same boxes")
    eng = engine or default_engine()
    stacks = list(stacks)
    rates = [tuple(r) for r in rates]

    def call():
        boxes = None
        if crops is not None:
            if len(crops) != len(stacks):
                raise ValueError("a Crop per video")
            boxes = np.stack([c.as_abi() if isinstance(c, Crop) else np.asarray(c, np.uint32).reshape(4) for c in crops]).reshape(-1, 4) if len(stacks) else None
        elif letterbox and stacks:  # the boxes of frames 0 and 8 of every video, by the mixed letterbox call
            boxes = eng.hash_clips_letterbox(stacks)[1]
        return eng.hash_windows_clips_rates(stacks, rates, stride, crops=boxes)

    words, first = _with_planes(call)
    return {rate: [[VideoHash(words[r][k], src_paths[i], durations[i]) for k in range(int(first[r, i]), int(first[r, i + 1]))] for i in range(len(stacks))]
            for r, rate in enumerate(rates)}


def hash_frame_windows(frames: np.ndarray, src_paths: Sequence, durations: Sequence[int], stride: int = 1,
                       engine: Optional[Engine] = None, zero_plane: bool = False, crops: Optional[Sequence] = None,
                       letterbox: bool = False, rate=None, one_call: bool = False, rates=None):
    """Every 16-frame window of every video (Engine.hash_windows): frames [n_videos, n_frames >= 16, H, W] u8 -> per video the VideoHash of
    frames [k * stride, k * stride + 16) for k = 0 .. (n_frames - 16) // stride, each carrying the video's src_paths[i] and durations[i].
    What finds a duplicate that is shifted in time (`locate`); the reference hashes one 16-frame stack per file (definitions.rs:31-34).
    zero_plane: every window's hash also carries its zero plane (VideoHash.zero; Engine.hash_windows_planes), which align_flipped needs;
    the hash words are the same.
    frames may also be a LIST of [F_i >= 16, H_i, W_i] stacks of different frame sizes AND lengths, as a library's files are: they are hashed
    by one call (Engine.hash_windows_clips[_planes]) and the per-video lists differ in length.  List input only: crops = a Crop (or four
    edge offsets l, r, t, b) per video, read in place; letterbox=True detects every video's box on its frames 0 and 8 (Engine.hash_clips_letterbox,
    as gen_hashes does) and hashes the windows inside it.
    rate=(num, den), 1 <= den <= num <= 2 den: RETIMED windows (Engine.hash_windows_retimed) - window k = the 16 frames k * stride +
    (i * num) // den, which is what a copy of the video at den / num of its frame rate (or sped up num / den) holds in its plain windows;
    align_retimed aligns the two.  Give it for the side with more frames per second.  No zero planes with a rate; a list of stacks is hashed by
    one call per video, without crops or letterbox.
    one_call=True (a list of stacks and a rate only): the whole library's retimed windows by ONE call (Engine.hash_windows_clips_retimed), the
    same words; crops and letterbox=True are then taken as the plain list form takes them.
    rates=[(num, den), ...], up to 8: the retimed windows at EVERY listed rate from one upload, one resize and one spatial transform of the
    frames (Engine.hash_windows_rates) -> {(num, den): the list rate=(num, den) would return}; (1, 1) gives the plain windows.  For whoever does
    not know the rate of a copy: align_rates and best_rates take it from there.  Not together with rate= or zero_plane=; a list of stacks is
    hashed by one call per video, without crops or letterbox.
    rates= with one_call=True (a list of stacks only): the whole library at every listed rate by ONE call (Engine.hash_windows_clips_rates) - every
    frame read, resized and transformed once - the same dict of the same words; crops and letterbox=True are then taken as the plain list form
    takes them."""
    if len(src_paths) < len(frames) or len(durations) < len(frames):
        raise ValueError("a path and a duration per video")
    if rates is not None:
        if rate is not None or zero_plane:
            raise ValueError("rates= goes with neither rate= nor zero_plane=")
        if one_call and isinstance(frames, (list, tuple)):
            return _hash_frame_windows_rates_library(frames, src_paths, durations, stride, engine, rates, crops, letterbox)
        if one_call or crops is not None or letterbox:
            raise ValueError("rates= takes one_call=, crops= and letterbox= only for a list of stacks with one_call=True")
        return _hash_frame_windows_rates(frames, src_paths, durations, stride, engine, rates)
    if one_call and (rate is None or not isinstance(frames, (list, tuple))):
        raise ValueError("one_call=True takes a list of stacks and a rate")
    if rate is not None:
        if zero_plane:
            raise ValueError("retimed windows have no zero planes")
        if one_call:
            return _hash_frame_windows_retimed_library(frames, src_paths, durations, stride, engine, rate, crops, letterbox)
        if crops is not None or letterbox:
            raise ValueError("retimed windows take crops or letterbox only for a list of stacks with one_call=True")
        return _hash_frame_windows_retimed(frames, src_paths, durations, stride, engine, rate)
    if isinstance(frames, (list, tuple)):
        return _hash_frame_windows_mixed(frames, src_paths, durations, stride, engine, zero_plane, crops, letterbox)
    if crops is not None or letterbox:
        raise ValueError("crops and letterbox take a list of stacks")
    if zero_plane:
        eng = engine or default_engine()
        words, zero = _with_planes(lambda: eng.hash_windows_planes(frames, stride))
        return [[VideoHash(words[i, k], src_paths[i], durations[i], zero[i, k]) for k in range(words.shape[1])] for i in range(words.shape[0])]
    try:
        words = (engine or default_engine()).hash_windows(frames, stride)
    except VdfError as e:
        if e.code == _capi.VDF_E_NOT_ENOUGH_FRAMES:
            raise NotEnoughFrames() from e
        raise
    return [[VideoHash(words[i, k], src_paths[i], durations[i]) for k in range(words.shape[1])] for i in range(words.shape[0])]


def locate(needles: Sequence[VideoHash], windows: List[List[VideoHash]], tolerance: float, stride: int = 1,
           engine: Optional[Engine] = None) -> List[List[tuple]]:
    """Where do the needles occur in the videos?  windows: hash_frame_windows' result at the same `stride`.  Per needle, ascending, the
    (video index, first frame = k * stride, hamming distance) of every window within `tolerance` of it.  The existing reference search
    with every duration set to 0, so that search_one's +-5 % duration window admits every entry: where in a video a clip sits says
    nothing about how long the clip is."""
    needles = list(needles)
    flat = [(v, k) for v, ws in enumerate(windows) for k in range(len(ws))]
    if not needles or not flat:
        return [[] for _ in needles]
    engine = engine or default_engine()
    words = np.stack([windows[v][k].hash for v, k in flat])
    rwords = np.stack([n.hash for n in needles])
    res = engine.search_refs_sorted(words, np.zeros(len(flat), np.uint32), rwords, np.zeros(len(needles), np.uint32), tolerance_int(tolerance))
    out: List[List[tuple]] = [[] for _ in needles]
    for r, ms in res:
        out[r] = sorted((flat[m][0], flat[m][1] * stride, hamming_distance_words(needles[r].hash, words[m])) for m in ms)
    return out


class Alignment(NamedTuple):
    """The longest stretch two videos share (align): video indices into windows_a / windows_b, the shift and the stretch in frames,
    the mean hamming distance of its windows, and the two videos' paths."""
    a: int
    b: int
    offset_frames: int     # first_frame_b - first_frame_a
    first_frame_a: int
    first_frame_b: int
    n_frames: int          # (n_windows - 1) * stride + 16
    n_windows: int
    mean_distance: float
    path_a: object = None
    path_b: object = None


ALIGN_MAX_PAIRS = 1 << 24       # pairs of videos one call of the C ABI takes (include/vdf.h); align splits above it
ALIGN_FIRST_CAPACITY = 4096     # records the first try of a call makes room for; a call that finds more is repeated with room for all
ALIGN_HOST_CELLS = 1 << 16      # with no engine given, inputs of at most this many cells are walked on the CPU (vdf_align_windows_host)
ALIGN_STATIC_DONTCARE = 900     # a window of identical frames has no temporal content: its 900 coefficients of temporal frequency > 0 are 0


def static_windows(dontcare, threshold: int = ALIGN_STATIC_DONTCARE) -> np.ndarray:
    """Per-window skip flags for align from the don't-care counts of Engine.hash_windows(..., want_dontcare=True): a window with at least
    `threshold` of its 1000 coefficients at zero is static - its hash is rounding noise and like every other static window's."""
    return (np.asarray(dontcare) >= threshold).astype(np.uint8)


def _align_csr(windows, static):
    counts = [len(ws) for ws in windows]
    first = np.zeros(len(windows) + 1, np.uint32)
    first[1:] = np.cumsum(counts)
    words = np.zeros((int(first[-1]), HASH_WORDS), np.uint64)
    k = 0
    for ws in windows:
        for h in ws:
            words[k] = h.hash
            k += 1
    skip = None
    if static is not None:
        if len(static) != len(windows) or any(len(f) != n for f, n in zip(static, counts)):
            raise ValueError("one static flag per window of every video")
        skip = np.concatenate([np.asarray(f, dtype=bool).astype(np.uint8).reshape(-1) for f in static] + [np.zeros(0, np.uint8)])
    return words, first, skip, counts


def _align_call(engine, a, b, tol_int, min_run, plist=None):
    """One call of the C ABI, repeated with a larger buffer if the first try's was too small.  a, b: (words, first, skip); b None: self.
    plist: only these pairs of the call's videos (the *_pairs form); None: all of them."""
    def once(capacity):
        kw = dict(tol_int=tol_int, min_run=min_run, a_skip=a[2], capacity=capacity)
        if b is not None:
            kw.update(b_hashes=b[0], b_first=b[1], b_skip=b[2])
        if plist is not None:
            return align_windows_pairs_host(a[0], a[1], plist, **kw) if engine is None else engine.align_windows_pairs(a[0], a[1], plist, **kw)
        return align_windows_host(a[0], a[1], **kw) if engine is None else engine.align_windows(a[0], a[1], **kw)
    rec, found = once(ALIGN_FIRST_CAPACITY)
    if found > len(rec):
        rec, found = once(found)
    return rec


def _seed_call(engine, a, b, tol_int, min_run):
    """_align_call for the seed calls: the candidate pairs of one call, VIDEO_PAIR_DTYPE in (a, b) order."""
    def once(capacity):
        kw = dict(tol_int=tol_int, min_run=min_run, a_skip=a[2], capacity=capacity)
        if b is not None:
            kw.update(b_hashes=b[0], b_first=b[1], b_skip=b[2])
        return align_seed_pairs_host(a[0], a[1], **kw) if engine is None else engine.align_seed_pairs(a[0], a[1], **kw)
    p, found = once(ALIGN_FIRST_CAPACITY)
    if found > len(p):
        p, found = once(found)
    return p


def _align_pair_list(pairs, n_a, n_b, self_mode):
    """The `pairs` keyword of align / align_all as VIDEO_PAIR_DTYPE, checked as the library checks the list of a *_pairs call."""
    if pairs is None:
        return None
    p = video_pairs(pairs if isinstance(pairs, np.ndarray) else np.asarray(list(pairs), dtype=np.int64))
    problem = pair_list_problem(p, n_a, n_b, self_mode)
    if problem:
        raise ValueError(problem)
    return p


def _block_pairs(engine, A, B, a0, a1, b0, b1, tol_int, min_run, pair_list, seed):
    """The pairs of one block of videos [a0, a1) x [b0, b1) that are aligned, counted inside the block: those of the caller's list, the seeded
    candidates (vdf_align_seed_pairs), or the candidates that are on the list.  None: every pair of the block."""
    plist = None
    if pair_list is not None:
        sel = (pair_list["a"] >= a0) & (pair_list["a"] < a1) & (pair_list["b"] >= b0) & (pair_list["b"] < b1)
        plist = pair_list[sel].copy()
        plist["a"] -= a0
        plist["b"] -= b0
        if not len(plist):
            return plist
    if seed:
        cand = _seed_call(engine, A, B, tol_int, min_run)
        if plist is None:
            return cand
        key = lambda p: (p["a"].astype(np.uint64) << np.uint64(32)) | p["b"].astype(np.uint64)
        plist = plist[np.isin(key(plist), key(cand))]
    return plist


def candidate_pairs(windows_a: List[List[VideoHash]], windows_b: Optional[List[List[VideoHash]]] = None, tolerance: float = DEFAULT_SEARCH_TOLERANCE,
                    min_run: int = 1, static_a=None, static_b=None, engine: Optional[Engine] = None) -> List[tuple]:
    """Which pairs of videos can share a stretch at all?  Arguments as `align`; -> [(a, b)] in (a, b) order: the pairs with a window ka of a,
    ka a multiple of min_run, and a window of b within `tolerance` of each other, neither static (include/vdf.h: vdf_align_seed_pairs).  A run of
    min_run windows holds such a window, so every pair `align` reports is among them - and a library of unrelated videos costs 1 / min_run of
    the distances of `align` at several times its rate instead of a walk of every pair."""
    self_mode = windows_b is None
    tol_int = tolerance_int(tolerance)
    wa, fa, ka, ca = _align_csr(windows_a, static_a)
    wb, fb, kb, cb = (wa, fa, ka, ca) if self_mode else _align_csr(windows_b, static_b)
    if engine is None:
        cells = (sum(ca) ** 2 - sum(n * n for n in ca)) // 2 if self_mode else sum(ca) * sum(cb)
        if cells > ALIGN_HOST_CELLS:
            engine = default_engine()

    def block(words, first, skip, lo, hi):
        w0, w1 = int(first[lo]), int(first[hi])
        return words[w0:w1], first[lo:hi + 1] - first[lo], None if skip is None else skip[w0:w1]

    step = max(1, math.isqrt(ALIGN_MAX_PAIRS))
    out = []
    for a0 in range(0, len(ca), step):
        a1 = min(a0 + step, len(ca))
        A = block(wa, fa, ka, a0, a1)
        for b0 in range(a0 if self_mode else 0, len(cb), step):
            b1 = min(b0 + step, len(cb))
            p = _seed_call(engine, A, None if (self_mode and b0 == a0) else block(wb, fb, kb, b0, b1), tol_int, int(min_run))
            out += [(int(a) + a0, int(b) + b0) for a, b in zip(p["a"], p["b"])]
    return sorted(out)


def align(windows_a: List[List[VideoHash]], windows_b: Optional[List[List[VideoHash]]] = None, tolerance: float = DEFAULT_SEARCH_TOLERANCE,
          min_run: int = 1, stride: int = 1, static_a=None, static_b=None, engine: Optional[Engine] = None, pairs=None,
          seed: bool = False) -> List[Alignment]:
    """Which videos share a stretch, at what offset, and for how long?  windows_a / windows_b: hash_frame_windows' results at the same
    `stride` (videos may differ in length); windows_b None: the videos of windows_a against each other, every pair once (a < b).
    Per pair of videos at most ONE Alignment, ordered by (a, b): the run of consecutive windows within `tolerance` on one diagonal
    (first_frame_b - first_frame_a constant) that maximises n_windows * (tol_int + 1) - sum of distances, of at least min_run windows
    (include/vdf.h: vdf_align_windows; a video that holds two separate excerpts of another reports the better one - align_all reports both).
    static_a / static_b: per video, one flag per window (static_windows); flagged windows abstain - static stretches match each other
    everywhere.  Calls of more than ALIGN_MAX_PAIRS pairs are split.  With no engine given, tiny inputs are walked on the CPU.
    pairs: only these (a, b) are aligned - strictly increasing in (a, b), a < b when windows_b is None (vdf_align_windows_pairs).
    seed=True: every block of videos is seeded first (candidate_pairs) and only its candidates are aligned; the result is the same list, and
    a library in which few videos share anything is not walked pair by pair.  With both, the candidates on the list."""
    self_mode = windows_b is None
    s = int(stride)
    if s != stride or s < 1:
        raise ValueError("stride must be a positive integer")
    tol_int = tolerance_int(tolerance)
    wa, fa, ka, ca = _align_csr(windows_a, static_a)
    wb, fb, kb, cb = (wa, fa, ka, ca) if self_mode else _align_csr(windows_b, static_b)
    pair_list = _align_pair_list(pairs, len(ca), len(cb), self_mode)
    if engine is None:
        cells = (sum(ca) ** 2 - sum(n * n for n in ca)) // 2 if self_mode else sum(ca) * sum(cb)
        if cells > ALIGN_HOST_CELLS:
            engine = default_engine()

    def block(words, first, skip, lo, hi):
        w0, w1 = int(first[lo]), int(first[hi])
        return words[w0:w1], first[lo:hi + 1] - first[lo], None if skip is None else skip[w0:w1]

    step = max(1, math.isqrt(ALIGN_MAX_PAIRS))
    parts = []
    for a0 in range(0, len(ca), step):
        a1 = min(a0 + step, len(ca))
        A = block(wa, fa, ka, a0, a1)
        for b0 in range(a0 if self_mode else 0, len(cb), step):
            b1 = min(b0 + step, len(cb))
            B = None if (self_mode and b0 == a0) else block(wb, fb, kb, b0, b1)
            plist = _block_pairs(engine, A, B, a0, a1, b0, b1, tol_int, int(min_run), pair_list, seed)
            if plist is not None and not len(plist):
                continue
            rec = _align_call(engine, A, B, tol_int, int(min_run), plist).copy()
            rec["a"] += a0
            rec["b"] += b0
            parts.append(rec)
    rec = np.concatenate(parts) if parts else np.zeros(0, ALIGN_DTYPE)
    rec = rec[np.lexsort((rec["b"], rec["a"]))]
    pa = [ws[0].src_path() if ws else None for ws in windows_a]
    pb = pa if self_mode else [ws[0].src_path() if ws else None for ws in windows_b]
    out = []
    for r in rec:
        a, b, off, st, n, ds = (int(r[k]) for k in ("a", "b", "offset", "start_a", "n_windows", "dist_sum"))
        out.append(Alignment(a, b, off * s, st * s, (st + off) * s, (n - 1) * s + _capi.DCT_SIZE, n, ds / n, pa[a], pb[b]))
    return out


class RetimedAlignment(NamedTuple):
    """The longest stretch a video shares with a copy at num / den of its frames (align_retimed): video indices, the rate in lowest terms,
    where the stretch starts in each video and how many of each video's frames it covers, the number of (sub-sampled) windows that matched,
    their mean hamming distance, and the two videos' paths."""
    a: int
    b: int
    num: int
    den: int
    first_frame_a: int
    first_frame_b: int
    n_frames_a: int        # (n_windows - 1) * num + span
    n_frames_b: int        # (n_windows - 1) * den + 16
    n_windows: int
    mean_distance: float
    path_a: object = None
    path_b: object = None


ALIGN_RETIMED_MAX_NUM = 32  # align_retimed makes `num` align calls; = VDF_ALIGN_RETIMED_MAX_NUM (include/vdf.h), the native call's limit
assert ALIGN_RETIMED_MAX_NUM == _capi.ALIGN_RETIMED_MAX_NUM


def _retimed_call(engine, a, b, tol_int, min_run, rate, plist=None):
    """_align_call for the retimed calls: one call of the C ABI (vdf_align_windows_retimed[_pairs][_host]), ALIGN_RETIMED_DTYPE in (a, b) order."""
    def once(capacity):
        kw = dict(tol_int=tol_int, min_run=min_run, a_skip=a[2], b_skip=b[2], capacity=capacity)
        if plist is not None:
            return (align_windows_retimed_pairs_host(a[0], a[1], plist, b[0], b[1], rate, **kw) if engine is None
                    else engine.align_windows_retimed_pairs(a[0], a[1], plist, b[0], b[1], rate, **kw))
        return align_windows_retimed_host(a[0], a[1], b[0], b[1], rate, **kw) if engine is None else engine.align_windows_retimed(a[0], a[1], b[0], b[1], rate, **kw)
    rec, found = once(ALIGN_FIRST_CAPACITY)
    if found > len(rec):
        rec, found = once(found)
    return rec


def _align_retimed_native(windows_a, windows_b, num, den, tolerance, min_run, static_a, static_b, engine, seed, pairs):
    """align_retimed(native=True): the CSR of both sides once, one call of vdf_align_windows_retimed* per block of at most ALIGN_MAX_PAIRS pairs.
    -> ALIGN_RETIMED_DTYPE records in (a, b) order."""
    tol_int = tolerance_int(tolerance)
    wa, fa, ka, ca = _align_csr(windows_a, static_a)
    wb, fb, kb, cb = _align_csr(windows_b, static_b)
    pair_list = _align_pair_list(pairs, len(ca), len(cb), False)
    if engine is None and sum(ca) * sum(cb) // den > ALIGN_HOST_CELLS:  # the cells a call walks: Na x Nb / den per pair
        engine = default_engine()

    def block(words, first, skip, lo, hi):
        w0, w1 = int(first[lo]), int(first[hi])
        return words[w0:w1], first[lo:hi + 1] - first[lo], None if skip is None else skip[w0:w1]

    def sub(side, p, step):
        """the windows p, p + step, ... of every video of a block - what ws[p::step] is to the lists - cut out of its arrays"""
        words, first, skip = side
        counts = np.diff(first.astype(np.int64))
        video = np.repeat(np.arange(len(counts)), counts)
        keep = (np.arange(len(words)) - first[:-1].astype(np.int64)[video]) % step == p
        sub_first = np.zeros(len(first), np.uint32)
        sub_first[1:] = np.cumsum(np.bincount(video[keep], minlength=len(counts)))
        return words[keep], sub_first, None if skip is None else skip[keep]

    key = lambda p: (p["a"].astype(np.uint64) << np.uint64(32)) | p["b"].astype(np.uint64)

    def seeded(A, B, plist):
        """the candidates of the block: the union over the phases of candidate_pairs' call (vdf_align_seed_pairs) on the sub-sampled sets - exact per
        phase, so no pair with a record is lost - and of those the pairs on the caller's list"""
        B0 = sub(B, 0, den)
        keys = np.unique(np.concatenate([key(_seed_call(engine, sub(A, p, num), B0, tol_int, int(min_run))) for p in range(num)]))
        cand = np.zeros(len(keys), VIDEO_PAIR_DTYPE)
        cand["a"], cand["b"] = keys >> np.uint64(32), keys & np.uint64(0xFFFFFFFF)
        return cand if plist is None else plist[np.isin(key(plist), keys)]

    step = max(1, math.isqrt(ALIGN_MAX_PAIRS))
    parts = []
    for a0 in range(0, len(ca), step):
        a1 = min(a0 + step, len(ca))
        A = block(wa, fa, ka, a0, a1)
        for b0 in range(0, len(cb), step):
            b1 = min(b0 + step, len(cb))
            B = block(wb, fb, kb, b0, b1)
            plist = _block_pairs(engine, A, None, a0, a1, b0, b1, tol_int, int(min_run), pair_list, False)
            if seed and (plist is None or len(plist)):
                plist = seeded(A, B, plist)
            if plist is not None and not len(plist):
                continue
            rec = _retimed_call(engine, A, B, tol_int, int(min_run), (num, den), plist).copy()
            rec["a"] += a0
            rec["b"] += b0
            parts.append(rec)
    rec = np.concatenate(parts) if parts else np.zeros(0, ALIGN_RETIMED_DTYPE)
    return rec[np.lexsort((rec["b"], rec["a"]))]


def align_retimed(windows_a: List[List[VideoHash]], windows_b: List[List[VideoHash]], rate, tolerance: float = DEFAULT_SEARCH_TOLERANCE,
                  min_run: int = 1, static_a=None, static_b=None, engine: Optional[Engine] = None, seed: bool = False, native: bool = False,
                  pairs=None) -> List[RetimedAlignment]:
    """Which videos of A share a stretch with a video of B that runs at den / num of A's frames - a re-encode from 30 to 25 fps (rate 6/5), a
    1.5 x re-upload (3/2), every other frame (2/1)?  windows_a: hash_frame_windows(..., rate=rate) at stride 1; windows_b: plain windows at
    stride 1.  If B[j] = A[c + (j * num) // den], retimed window c + num * m of A equals plain window den * m of B: the matching cells of the
    pair lie on a line of slope num / den, which `align` does not follow.  So for every phase p = 0 .. num - 1 the windows p, p + num, ... of A
    are aligned (`align`, diagonals) with the windows 0, den, 2 den, ... of B, static flags sub-sampled alike, and per pair of videos the
    record that maximises n_windows * (tol_int + 1) - sum of distances is kept (ties: the smaller first_frame_a, then first_frame_b).
    A true stretch holds a window of B at a multiple of den, so B's phase 0 is enough: the stretch is found with its ends rounded inward by
    less than den frames of B, and Na * Nb / den cells are walked.  min_run counts sub-sampled windows.  The rate is reduced by its gcd;
    num > 32 is refused (the call makes num sub-calls).  No self mode.  -> one RetimedAlignment per pair at most, ordered by (a, b).
    native=True: the same list from ONE call of the C ABI per block of at most ALIGN_MAX_PAIRS pairs (vdf_align_windows_retimed*):
    the CSR is built once and every phase of every pair is a unit of one launch.  With seed=True the candidates of the sub-sampled sets
    (candidate_pairs) are united over the phases and one call on that list is made.  With no engine given, tiny inputs are walked on the CPU.
    pairs: only these (a, b) are aligned - strictly increasing in (a, b), as `align` takes them."""
    try:
        num, den = (int(x) for x in rate)
        if (num, den) != tuple(rate):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"rate must be a pair of integers (num, den), not {rate!r}") from None
    if not 1 <= den <= num <= 2 * den:
        raise ValueError("rate must have 1 <= den <= num <= 2 den")
    g = math.gcd(num, den)
    num, den = num // g, den // g
    if num > ALIGN_RETIMED_MAX_NUM:
        raise ValueError(f"align_retimed makes num sub-calls: num = {num} is above {ALIGN_RETIMED_MAX_NUM}")
    span = (15 * num) // den + 1
    pa = [ws[0].src_path() if ws else None for ws in windows_a]
    pb = [ws[0].src_path() if ws else None for ws in windows_b]
    if native:
        rec = _align_retimed_native(windows_a, windows_b, num, den, tolerance, min_run, static_a, static_b, engine, seed, pairs)
        out = []
        for r in rec:
            a, b, fa, fb, n, ds = (int(r[k]) for k in ("a", "b", "first_a", "first_b", "n_windows", "dist_sum"))
            out.append(RetimedAlignment(a, b, num, den, fa, fb, (n - 1) * num + span, (n - 1) * den + _capi.DCT_SIZE, n, ds / n, pa[a], pb[b]))
        return out
    tol_int = tolerance_int(tolerance)
    sub_b = [ws[0::den] for ws in windows_b]
    st_b = None if static_b is None else [np.asarray(f).reshape(-1)[0::den] for f in static_b]
    best = {}
    for p in range(num):
        sub_a = [ws[p::num] for ws in windows_a]
        st_a = None if static_a is None else [np.asarray(f).reshape(-1)[p::num] for f in static_a]
        for al in align(sub_a, sub_b, tolerance, min_run=min_run, stride=1, static_a=st_a, static_b=st_b, engine=engine, seed=seed, pairs=pairs):
            n, i0 = al.n_windows, al.first_frame_a
            dist_sum = int(round(al.mean_distance * n))
            rec = (-(n * (tol_int + 1) - dist_sum), p + num * i0, den * al.first_frame_b, n, dist_sum)
            if (al.a, al.b) not in best or rec < best[(al.a, al.b)]:
                best[(al.a, al.b)] = rec
    return [RetimedAlignment(a, b, num, den, fa, fb, (n - 1) * num + span, (n - 1) * den + _capi.DCT_SIZE, n, ds / n, pa[a], pb[b])
            for (a, b), (_, fa, fb, n, ds) in sorted(best.items())]


def _retimed_rate(rate):
    """(num, den) of a rate in lowest terms, refused as align_retimed refuses it."""
    try:
        num, den = (int(x) for x in rate)
        if (num, den) != tuple(rate):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"rate must be a pair of integers (num, den), not {rate!r}") from None
    if not 1 <= den <= num <= 2 * den:
        raise ValueError("rate must have 1 <= den <= num <= 2 den")
    g = math.gcd(num, den)
    num, den = num // g, den // g
    if num > ALIGN_RETIMED_MAX_NUM:
        raise ValueError(f"align_retimed makes num sub-calls: num = {num} is above {ALIGN_RETIMED_MAX_NUM}")
    return num, den


def _rates_csr(windows_by_rate_a, static_a):
    """The A side of the seeded retimed call: one CSR per rate (words, first, skip, counts), every rate over the same videos."""
    rates = list(windows_by_rate_a)
    if not 1 <= len(rates) <= _capi.WINDOWS_MAX_RATES:
        raise ValueError(f"1 .. {_capi.WINDOWS_MAX_RATES} rates in one pass, not {len(rates)}")
    per = [_align_csr(windows_by_rate_a[r], None if static_a is None else static_a.get(r)) for r in rates]
    if len({len(c[3]) for c in per}) != 1:
        raise ValueError("every rate holds the windows of the same videos")
    return rates, per


def _rates_block(per, lo, hi):
    """The videos [lo, hi) of every rate's CSR as ONE rate-major set: (words, first [n_rates, hi - lo + 1], rate_first, skip or None)."""
    cuts = [(int(f[lo]), int(f[hi])) for _, f, _, _ in per]
    first = np.stack([f[lo:hi + 1] - f[lo] for _, f, _, _ in per]).astype(np.uint32)
    rate_first = np.zeros(len(per) + 1, np.int64)
    rate_first[1:] = np.cumsum([w1 - w0 for w0, w1 in cuts])
    words = np.concatenate([w[w0:w1] for (w, _, _, _), (w0, w1) in zip(per, cuts)])
    skip = None
    if any(k is not None for _, _, k, _ in per):
        skip = np.concatenate([np.zeros(w1 - w0, np.uint8) if k is None else k[w0:w1] for (_, _, k, _), (w0, w1) in zip(per, cuts)])
    return words, first, rate_first, skip


def _seed_rates_call(engine, A, B, rates, tol_int, min_run, exclude_same):
    """_seed_call for the seeded retimed call: the (a, b, rate) triples of one call, VIDEO_PAIR_RATE_DTYPE in (rate, a, b) order."""
    def once(capacity):
        kw = dict(tol_int=tol_int, min_run=min_run, a_rate_first=A[2], a_skip=A[3], b_skip=B[2], exclude_same=exclude_same, capacity=capacity)
        call = align_seed_pairs_rates_host if engine is None else engine.align_seed_pairs_rates
        return call(A[0], A[1], B[0], B[1], rates, **kw)
    t, found = once(ALIGN_FIRST_CAPACITY)
    if found > len(t):
        t, found = once(found)
    return t


def _candidate_blocks_rates(per, csr_b, rates, tol_int, min_run, engine, exclude_same):
    """Every block of at most ALIGN_MAX_PAIRS pairs of videos with its triples: yields (a0, a1, b0, b1, B block, triples counted inside the block)."""
    wb, fb, kb, cb = csr_b
    n_a = len(per[0][3])
    if exclude_same and n_a != len(cb):
        raise ValueError("exclude_same takes the same number of videos on both sides")
    step = max(1, math.isqrt(ALIGN_MAX_PAIRS))
    for a0 in range(0, n_a, step):
        a1 = min(a0 + step, n_a)
        A = _rates_block(per, a0, a1)
        for b0 in range(0, len(cb), step):
            b1 = min(b0 + step, len(cb))
            w0, w1 = int(fb[b0]), int(fb[b1])
            B = (wb[w0:w1], fb[b0:b1 + 1] - fb[b0], None if kb is None else kb[w0:w1])
            yield a0, a1, b0, b1, B, _seed_rates_call(engine, A, B, rates, tol_int, min_run, bool(exclude_same) and a0 == b0)


def _rates_engine(engine, rates, per, cb):
    """With no engine given, tiny inputs are walked on the CPU - the rule of align_retimed(native=True), per rate."""
    if engine is None and any(sum(c[3]) * sum(cb) // _retimed_rate(r)[1] > ALIGN_HOST_CELLS for r, c in zip(rates, per)):
        return default_engine()
    return engine


def candidate_pairs_rates(windows_by_rate_a: dict, windows_b: List[List[VideoHash]], tolerance: float = DEFAULT_SEARCH_TOLERANCE, min_run: int = 1,
                          static_a: Optional[dict] = None, static_b=None, engine: Optional[Engine] = None, exclude_same: bool = False) -> dict:
    """Which pairs of videos can be a retimed copy of each other, at which of several rates?  Arguments as align_rates (at most 8 rates);
    -> {rate: [(a, b)] in (a, b) order}: the pairs with a window ka of a at that rate, (ka // num) % min_run == 0, and a window kb of b, kb % den
    == 0, within `tolerance` of each other, neither static (include/vdf.h: vdf_align_seed_pairs_rates).  Every pair align_retimed reports at a
    rate is among that rate's candidates.  Every phase of every rate is seeded by ONE call per block of at most ALIGN_MAX_PAIRS pairs of videos
    (DESIGN.md 4.22).  exclude_same: a pair (i, i) is never a candidate - for a library against itself."""
    tol_int = tolerance_int(tolerance)
    rates, per = _rates_csr(windows_by_rate_a, static_a)
    for r in rates:
        _retimed_rate(r)
    csr_b = _align_csr(windows_b, static_b)
    engine = _rates_engine(engine, rates, per, csr_b[3])
    out = {r: [] for r in rates}
    for a0, _, b0, _, _, t in _candidate_blocks_rates(per, csr_b, rates, tol_int, int(min_run), engine, exclude_same):
        for a, b, r in zip(t["a"], t["b"], t["rate"]):
            out[rates[int(r)]].append((int(a) + a0, int(b) + b0))
    return {r: sorted(p) for r, p in out.items()}


def _align_rates_one_pass(windows_by_rate_a, windows_b, tolerance, min_run, static_a, static_b, engine, pairs):
    """align_rates(one_pass=True): the CSR of B once and of each rate's A once; per block of videos ONE seed call for all rates
    (vdf_align_seed_pairs_rates), then one vdf_align_windows_retimed_pairs call per rate that has candidates."""
    tol_int = tolerance_int(tolerance)
    rates, per = _rates_csr(windows_by_rate_a, static_a)
    reduced = [_retimed_rate(r) for r in rates]
    csr_b = _align_csr(windows_b, static_b)
    pair_list = _align_pair_list(pairs, len(per[0][3]), len(csr_b[3]), False)
    engine = _rates_engine(engine, rates, per, csr_b[3])
    key = lambda p: (p["a"].astype(np.uint64) << np.uint64(32)) | p["b"].astype(np.uint64)
    parts = [[] for _ in rates]
    for a0, a1, b0, b1, B, t in _candidate_blocks_rates(per, csr_b, rates, tol_int, int(min_run), engine, False):
        plist = _block_pairs(engine, None, None, a0, a1, b0, b1, tol_int, int(min_run), pair_list, False)
        for i, (num, den) in enumerate(reduced):
            cand = np.zeros(int(np.count_nonzero(t["rate"] == i)), VIDEO_PAIR_DTYPE)
            cand["a"], cand["b"] = t["a"][t["rate"] == i], t["b"][t["rate"] == i]
            if plist is not None:
                cand = plist[np.isin(key(plist), key(cand))]
            if not len(cand):
                continue
            w, f, k, _ = per[i]
            w0, w1 = int(f[a0]), int(f[a1])
            A = (w[w0:w1], f[a0:a1 + 1] - f[a0], None if k is None else k[w0:w1])
            rec = _retimed_call(engine, A, B, tol_int, int(min_run), (num, den), cand).copy()
            rec["a"] += a0
            rec["b"] += b0
            parts[i].append(rec)
    pb = [ws[0].src_path() if ws else None for ws in windows_b]
    out = {}
    for i, (rate, (num, den)) in enumerate(zip(rates, reduced)):
        rec = np.concatenate(parts[i]) if parts[i] else np.zeros(0, ALIGN_RETIMED_DTYPE)
        rec = rec[np.lexsort((rec["b"], rec["a"]))]
        pa = [ws[0].src_path() if ws else None for ws in windows_by_rate_a[rate]]
        span = (15 * num) // den + 1
        out[rate] = []
        for r in rec:
            a, b, fa, fb, n, ds = (int(r[k]) for k in ("a", "b", "first_a", "first_b", "n_windows", "dist_sum"))
            out[rate].append(RetimedAlignment(a, b, num, den, fa, fb, (n - 1) * num + span, (n - 1) * den + _capi.DCT_SIZE, n, ds / n, pa[a], pb[b]))
    return out


def _rates_call(engine, A, B, rates, tol_int, min_run, triples, seed):
    """_retimed_call for the call over (rate, a, b) triples: one call of the C ABI (vdf_align_windows_rates[_host]), ALIGN_RATE_DTYPE in
    (rate, a, b) order.  A: a _rates_block; triples None: all of them, or with seed the candidates found inside the call."""
    def once(capacity):
        kw = dict(tol_int=tol_int, min_run=min_run, a_rate_first=A[2], a_skip=A[3], b_skip=B[2], triples=triples, seed=seed, capacity=capacity)
        call = align_windows_rates_host if engine is None else engine.align_windows_rates
        return call(A[0], A[1], B[0], B[1], rates, **kw)
    rec, found = once(ALIGN_FIRST_CAPACITY)
    if found > len(rec):
        rec, found = once(found)
    return rec


def _align_rates_one_call(windows_by_rate_a, windows_b, tolerance, min_run, static_a, static_b, engine, pairs, seed):
    """align_rates(one_call=True): the CSR of B once and of each rate's A once; per block of videos ONE vdf_align_windows_rates call for all rates -
    on every triple, on the candidates it finds itself (seed), on the listed pairs at every rate (pairs), or on the candidates that are on the
    list (both: one seed call, intersected as one_pass does, then the list form)."""
    tol_int = tolerance_int(tolerance)
    rates, per = _rates_csr(windows_by_rate_a, static_a)
    reduced = [_retimed_rate(r) for r in rates]
    wb, fb, kb, cb = csr_b = _align_csr(windows_b, static_b)
    n_a = len(per[0][3])
    pair_list = _align_pair_list(pairs, n_a, len(cb), False)
    engine = _rates_engine(engine, rates, per, cb)
    key = lambda p: (p["a"].astype(np.uint64) << np.uint64(32)) | p["b"].astype(np.uint64)
    step = max(1, math.isqrt(ALIGN_MAX_PAIRS))
    parts = []
    for a0 in range(0, n_a, step):
        a1 = min(a0 + step, n_a)
        A = _rates_block(per, a0, a1)
        for b0 in range(0, len(cb), step):
            b1 = min(b0 + step, len(cb))
            w0, w1 = int(fb[b0]), int(fb[b1])
            B = (wb[w0:w1], fb[b0:b1 + 1] - fb[b0], None if kb is None else kb[w0:w1])
            plist = _block_pairs(engine, None, None, a0, a1, b0, b1, tol_int, int(min_run), pair_list, False)
            triples = None
            if plist is not None:
                if seed and len(plist):
                    t = _seed_rates_call(engine, A, B, rates, tol_int, int(min_run), False)
                    cand = np.zeros(len(t), VIDEO_PAIR_DTYPE)
                    cand["a"], cand["b"] = t["a"], t["b"]
                    triples = t[np.isin(key(cand), key(plist))]
                else:
                    triples = np.zeros(len(rates) * len(plist), VIDEO_PAIR_RATE_DTYPE)
                    triples["a"], triples["b"] = np.tile(plist["a"], len(rates)), np.tile(plist["b"], len(rates))
                    triples["rate"] = np.repeat(np.arange(len(rates), dtype=np.uint32), len(plist))
                if not len(triples):
                    continue
            rec = _rates_call(engine, A, B, rates, tol_int, int(min_run), triples, bool(seed) and triples is None).copy()
            rec["a"] += a0
            rec["b"] += b0
            parts.append(rec)
    rec = np.concatenate(parts) if parts else np.zeros(0, ALIGN_RATE_DTYPE)
    rec = rec[np.lexsort((rec["b"], rec["a"], rec["rate"]))]
    pb = [ws[0].src_path() if ws else None for ws in windows_b]
    out = {}
    for i, (rate, (num, den)) in enumerate(zip(rates, reduced)):
        pa = [ws[0].src_path() if ws else None for ws in windows_by_rate_a[rate]]
        span = (15 * num) // den + 1
        out[rate] = []
        for r in rec[rec["rate"] == i]:
            a, b, fa, fb_, n, ds, nfb = (int(r[k]) for k in ("a", "b", "first_a", "first_b", "n_windows", "dist_sum", "n_frames_b"))
            out[rate].append(RetimedAlignment(a, b, num, den, fa, fb_, (n - 1) * num + span, nfb, n, ds / n, pa[a], pb[b]))
    return out


def align_rates(windows_by_rate_a: dict, windows_b: List[List[VideoHash]], tolerance: float = DEFAULT_SEARCH_TOLERANCE, min_run: int = 1,
                static_a: Optional[dict] = None, static_b=None, engine: Optional[Engine] = None, native: bool = True, seed: bool = False,
                pairs=None, one_pass: bool = False, one_call: bool = False) -> dict:
    """Which videos of A are a retimed copy of which video of B, at which of several rates?  windows_by_rate_a: {(num, den): windows of A at that
    rate}, as hash_frame_windows(..., rates=[...]) returns it, stride 1; windows_b: the PLAIN windows of B at stride 1 (the (1, 1) entry of such a
    dict).  One align_retimed call per rate, in the dict's order, with everything else handed through (static_a: {rate: flags per video} or None)
    -> {rate: List[RetimedAlignment]}.  best_rates picks one record per pair from it.
    one_pass=True (needs seed=True and native=True; at most 8 rates): the same dict, but every phase of every rate is seeded by ONE call per block
    of videos (candidate_pairs_rates' call) instead of num calls per rate on sub-sampled copies, and each rate that has candidates then makes its
    one align call on them.
    one_call=True (needs native=True; at most 8 rates): the same dict from ONE vdf_align_windows_rates call per block of videos - the triples of all
    rates are one launch set, and with seed=True the candidates are found inside the call, on arrays that went up once."""
    if one_call:
        if not native or one_pass:
            raise ValueError("one_call=True needs native=True and excludes one_pass")
        return _align_rates_one_call(windows_by_rate_a, windows_b, tolerance, min_run, static_a, static_b, engine, pairs, seed)
    if one_pass:
        if not (seed and native):
            raise ValueError("one_pass=True needs seed=True and native=True")
        return _align_rates_one_pass(windows_by_rate_a, windows_b, tolerance, min_run, static_a, static_b, engine, pairs)
    return {rate: align_retimed(ws, windows_b, rate, tolerance, min_run=min_run, static_a=None if static_a is None else static_a.get(rate), static_b=static_b,
                                engine=engine, seed=seed, native=native, pairs=pairs)
            for rate, ws in windows_by_rate_a.items()}


def best_rates(result: dict, tolerance: float = DEFAULT_SEARCH_TOLERANCE) -> List[RetimedAlignment]:
    """One record per pair (a, b) out of align_rates' result, ordered by (a, b): the one that maximises
    n_frames_b * (tol_int + 1 - mean_distance) - the frames of B the stretch covers times its margin below the tolerance.  That is comparable
    across rates, which n_windows is not: a rate with a larger den sub-samples B more coarsely, and the same stretch counts fewer windows.
    Ties go to the rate that comes first in `result`, the caller's order.  The record's num / den name the rate, in lowest terms."""
    tol_int = tolerance_int(tolerance)
    best = {}
    for recs in result.values():
        for r in recs:
            score = r.n_frames_b * (tol_int + 1 - r.mean_distance)
            if (r.a, r.b) not in best or score > best[(r.a, r.b)][0]:
                best[(r.a, r.b)] = (score, r)
    return [best[k][1] for k in sorted(best)]


class RetimedAlignmentStretch(NamedTuple):
    """One of the stretches a video shares with a copy at num / den of its frames (align_rates_all): RetimedAlignment's fields plus the rank - 0
    is the pair's best stretch at that rate, the one align_rates reports; rank r is the best outside the rectangles of the ranks before it."""
    a: int
    b: int
    num: int
    den: int
    first_frame_a: int
    first_frame_b: int
    n_frames_a: int        # (n_windows - 1) * num + span
    n_frames_b: int        # (n_windows - 1) * den + 16
    n_windows: int
    mean_distance: float
    path_a: object = None
    path_b: object = None
    rank: int = 0


ALIGN_RATES_ALL_GUARD = 15  # frames of b: windows less than 16 frames apart share frames (align_all's default guard at stride 1)


def _rates_stretches_call(engine, A, B, rates, tol_int, min_run, max_stretches, guard, triples, seed):
    """_rates_call for the stretches call: one call of the C ABI (vdf_align_windows_rates_stretches[_host]), ALIGN_RATE_STRETCH_DTYPE in (rate, a, b,
    rank) order."""
    def once(capacity):
        kw = dict(tol_int=tol_int, min_run=min_run, max_stretches=max_stretches, guard=guard, a_rate_first=A[2], a_skip=A[3], b_skip=B[2], triples=triples,
                  seed=seed, capacity=capacity)
        call = align_windows_rates_stretches_host if engine is None else engine.align_windows_rates_stretches
        return call(A[0], A[1], B[0], B[1], rates, **kw)
    rec, found = once(ALIGN_FIRST_CAPACITY)
    if found > len(rec):
        rec, found = once(found)
    return rec


def align_rates_all(windows_by_rate_a: dict, windows_b: List[List[VideoHash]], tolerance: float = DEFAULT_SEARCH_TOLERANCE, min_run: int = 1,
                    max_stretches: int = 4, guard: Optional[int] = None, static_a: Optional[dict] = None, static_b=None, engine: Optional[Engine] = None,
                    pairs=None, seed: bool = False) -> dict:
    """EVERY stretch a video of A shares with a video of B at each of several rates, not only the best one: a copy that was converted to another
    frame rate or sped up AND had an ad break cut out shares two stretches with its source, one that had a scene replaced two runs on one line.
    Arguments as align_rates(one_call=True); per (rate, a, b) up to max_stretches (1 ... 8) RetimedAlignmentStretch
    -> {rate: [RetimedAlignmentStretch] ordered by (a, b, rank)}.  Rank 0 is the record align_rates reports; after every reported stretch its
    rectangle - its frames of a x its frames of b, widened by `guard` frames of b (and guard * num / den of a) - counts as non-matching in EVERY
    phase, and the next rank is the best record of what is left (include/vdf.h: vdf_align_windows_rates_stretches).  guard None: 15 frames.
    One call of the C ABI per block of at most ALIGN_MAX_PAIRS pairs of videos, for all rates; with no engine given, tiny inputs are walked on the
    CPU.  pairs / seed: as in align_rates(one_call=True).  best_rates_all picks one rate per pair from the result."""
    if guard is None:
        guard = ALIGN_RATES_ALL_GUARD
    tol_int = tolerance_int(tolerance)
    rates, per = _rates_csr(windows_by_rate_a, static_a)
    reduced = [_retimed_rate(r) for r in rates]
    wb, fb, kb, cb = _align_csr(windows_b, static_b)
    n_a = len(per[0][3])
    pair_list = _align_pair_list(pairs, n_a, len(cb), False)
    engine = _rates_engine(engine, rates, per, cb)
    key = lambda p: (p["a"].astype(np.uint64) << np.uint64(32)) | p["b"].astype(np.uint64)
    step = max(1, math.isqrt(ALIGN_MAX_PAIRS))
    parts = []
    for a0 in range(0, n_a, step):
        a1 = min(a0 + step, n_a)
        A = _rates_block(per, a0, a1)
        for b0 in range(0, len(cb), step):
            b1 = min(b0 + step, len(cb))
            w0, w1 = int(fb[b0]), int(fb[b1])
            B = (wb[w0:w1], fb[b0:b1 + 1] - fb[b0], None if kb is None else kb[w0:w1])
            plist = _block_pairs(engine, None, None, a0, a1, b0, b1, tol_int, int(min_run), pair_list, False)
            triples = None
            if plist is not None:
                if seed and len(plist):
                    t = _seed_rates_call(engine, A, B, rates, tol_int, int(min_run), False)
                    cand = np.zeros(len(t), VIDEO_PAIR_DTYPE)
                    cand["a"], cand["b"] = t["a"], t["b"]
                    triples = t[np.isin(key(cand), key(plist))]
                else:
                    triples = np.zeros(len(rates) * len(plist), VIDEO_PAIR_RATE_DTYPE)
                    triples["a"], triples["b"] = np.tile(plist["a"], len(rates)), np.tile(plist["b"], len(rates))
                    triples["rate"] = np.repeat(np.arange(len(rates), dtype=np.uint32), len(plist))
                if not len(triples):
                    continue
            rec = _rates_stretches_call(engine, A, B, rates, tol_int, int(min_run), int(max_stretches), int(guard), triples, bool(seed) and triples is None).copy()
            rec["a"] += a0
            rec["b"] += b0
            parts.append(rec)
    rec = np.concatenate(parts) if parts else np.zeros(0, ALIGN_RATE_STRETCH_DTYPE)
    rec = rec[np.lexsort((rec["rank"], rec["b"], rec["a"], rec["rate"]))]
    pb = [ws[0].src_path() if ws else None for ws in windows_b]
    out = {}
    for i, (rate, (num, den)) in enumerate(zip(rates, reduced)):
        pa = [ws[0].src_path() if ws else None for ws in windows_by_rate_a[rate]]
        span = (15 * num) // den + 1
        out[rate] = []
        for r in rec[rec["rate"] == i]:
            a, b, fa, fb_, n, ds, nfb, rank = (int(r[k]) for k in ("a", "b", "first_a", "first_b", "n_windows", "dist_sum", "n_frames_b", "rank"))
            out[rate].append(RetimedAlignmentStretch(a, b, num, den, fa, fb_, (n - 1) * num + span, nfb, n, ds / n, pa[a], pb[b], rank))
    return out


def best_rates_all(result: dict, tolerance: float = DEFAULT_SEARCH_TOLERANCE) -> dict:
    """One rate per pair (a, b) out of align_rates_all's result -> {(a, b): [RetimedAlignmentStretch]} with the keys in (a, b) order and the chosen
    rate's stretches by rank: the rate whose stretches TOGETHER maximise the sum of n_frames_b * (tol_int + 1 - mean_distance) - best_rates' score,
    added up over the stretches, so that a cut copy is judged by all of its parts.  Ties go to the rate that comes first in `result`."""
    tol_int = tolerance_int(tolerance)
    best = {}
    for recs in result.values():
        per_pair = {}
        for r in recs:
            per_pair.setdefault((r.a, r.b), []).append(r)
        for k, rs in per_pair.items():
            score = sum(r.n_frames_b * (tol_int + 1 - r.mean_distance) for r in rs)
            if k not in best or score > best[k][0]:
                best[k] = (score, sorted(rs, key=lambda r: r.rank))
    return {k: best[k][1] for k in sorted(best)}


class AlignmentStretch(NamedTuple):
    """One of the stretches two videos share (align_all): Alignment's fields plus the rank - 0 is the pair's best stretch, the one `align`
    reports; rank r is the best outside the rectangles of the ranks before it."""
    a: int
    b: int
    offset_frames: int     # first_frame_b - first_frame_a
    first_frame_a: int
    first_frame_b: int
    n_frames: int          # (n_windows - 1) * stride + 16
    n_windows: int
    mean_distance: float
    path_a: object = None
    path_b: object = None
    rank: int = 0


def _align_all_call(engine, a, b, tol_int, min_run, max_stretches, guard, plist=None):
    """_align_call for the stretches calls."""
    def once(capacity):
        kw = dict(tol_int=tol_int, min_run=min_run, max_stretches=max_stretches, guard=guard, a_skip=a[2], capacity=capacity)
        if b is not None:
            kw.update(b_hashes=b[0], b_first=b[1], b_skip=b[2])
        if plist is not None:
            if engine is None:
                return align_windows_stretches_pairs_host(a[0], a[1], plist, **kw)
            return engine.align_windows_stretches_pairs(a[0], a[1], plist, **kw)
        return align_windows_stretches_host(a[0], a[1], **kw) if engine is None else engine.align_windows_stretches(a[0], a[1], **kw)
    rec, found = once(ALIGN_FIRST_CAPACITY)
    if found > len(rec):
        rec, found = once(found)
    return rec


def align_all(windows_a: List[List[VideoHash]], windows_b: Optional[List[List[VideoHash]]] = None, tolerance: float = DEFAULT_SEARCH_TOLERANCE,
              min_run: int = 1, stride: int = 1, max_stretches: int = 4, guard: Optional[int] = None, static_a=None, static_b=None,
              engine: Optional[Engine] = None, pairs=None, seed: bool = False) -> List[AlignmentStretch]:
    """EVERY stretch two videos share, not only the best one: a re-upload with an ad break cut out shares two stretches at two offsets with
    its source, a compilation that uses a source twice repeats one.  Arguments as `align`; per pair of videos up to max_stretches (1 ... 8)
    AlignmentStretch, ordered by (a, b, rank).  Rank 0 is the Alignment `align` reports; after every reported stretch its rectangle - its
    windows of a x its windows of b, each widened by `guard` windows - counts as non-matching, and the next rank is the best run of what is
    left (include/vdf.h: vdf_align_windows_stretches).  The same windows of a matched against ANOTHER part of b stay visible.
    guard None: ceil(15 / stride) windows - windows less than 16 frames apart share frames, so in slowly changing content the diagonals
    beside a stretch match too, and what the bare rectangle leaves of them at its ends would be reported as short stretches of their own.
    Calls of more than ALIGN_MAX_PAIRS pairs are split.  With no engine given, tiny inputs are walked on the CPU.
    pairs / seed: as in `align` - only the listed pairs, only the seeded candidates (the same list as without), or the candidates on the list."""
    self_mode = windows_b is None
    s = int(stride)
    if s != stride or s < 1:
        raise ValueError("stride must be a positive integer")
    if guard is None:
        guard = -(-(_capi.DCT_SIZE - 1) // s)
    tol_int = tolerance_int(tolerance)
    wa, fa, ka, ca = _align_csr(windows_a, static_a)
    wb, fb, kb, cb = (wa, fa, ka, ca) if self_mode else _align_csr(windows_b, static_b)
    pair_list = _align_pair_list(pairs, len(ca), len(cb), self_mode)
    if engine is None:
        cells = (sum(ca) ** 2 - sum(n * n for n in ca)) // 2 if self_mode else sum(ca) * sum(cb)
        if cells > ALIGN_HOST_CELLS:
            engine = default_engine()

    def block(words, first, skip, lo, hi):
        w0, w1 = int(first[lo]), int(first[hi])
        return words[w0:w1], first[lo:hi + 1] - first[lo], None if skip is None else skip[w0:w1]

    step = max(1, math.isqrt(ALIGN_MAX_PAIRS))
    parts = []
    for a0 in range(0, len(ca), step):
        a1 = min(a0 + step, len(ca))
        A = block(wa, fa, ka, a0, a1)
        for b0 in range(a0 if self_mode else 0, len(cb), step):
            b1 = min(b0 + step, len(cb))
            B = None if (self_mode and b0 == a0) else block(wb, fb, kb, b0, b1)
            plist = _block_pairs(engine, A, B, a0, a1, b0, b1, tol_int, int(min_run), pair_list, seed)
            if plist is not None and not len(plist):
                continue
            rec = _align_all_call(engine, A, B, tol_int, int(min_run), int(max_stretches), int(guard), plist).copy()
            rec["a"] += a0
            rec["b"] += b0
            parts.append(rec)
    rec = np.concatenate(parts) if parts else np.zeros(0, ALIGN_STRETCH_DTYPE)
    rec = rec[np.lexsort((rec["rank"], rec["b"], rec["a"]))]
    pa = [ws[0].src_path() if ws else None for ws in windows_a]
    pb = pa if self_mode else [ws[0].src_path() if ws else None for ws in windows_b]
    out = []
    for r in rec:
        a, b, off, st, n, ds, rank = (int(r[k]) for k in ("a", "b", "offset", "start_a", "n_windows", "dist_sum", "rank"))
        out.append(AlignmentStretch(a, b, off * s, st * s, (st + off) * s, (n - 1) * s + _capi.DCT_SIZE, n, ds / n, pa[a], pb[b], rank))
    return out


class FlippedAlignment(NamedTuple):
    """The longest stretch video a shares with the FLIPPED video b (align_flipped): Alignment's fields plus the flip.  first_frame_b and
    n_frames describe the stretch in b's ORIGINAL frame numbering: frames [first_frame_b, first_frame_b + n_frames) of b, flipped, are
    frames [first_frame_a, first_frame_a + n_frames) of a.  With Flip.T in the flip b's stretch plays BACKWARDS: frame first_frame_a + i
    of a is frame first_frame_b + n_frames - 1 - i of b, and first_frame_b = (Nb - 1 - (start_a + offset + n_windows - 1)) * stride for
    the record (start_a, offset, n_windows) of the C ABI and the Nb windows of b."""
    a: int
    b: int
    offset_frames: int     # first_frame_b - first_frame_a
    first_frame_a: int
    first_frame_b: int
    n_frames: int          # (n_windows - 1) * stride + 16
    n_windows: int
    mean_distance: float
    path_a: object = None
    path_b: object = None
    flip: Flip = Flip.X


def _align_zero(windows, what):
    planes = [h.zero for ws in windows for h in ws]
    if any(z is None for z in planes):
        raise VidProc(f"align_flipped needs the zero plane of every hash of {what} (hash_frame_windows with zero_plane=True)")
    return np.stack(planes) if planes else np.zeros((0, HASH_WORDS), np.uint64)


def _align_flipped_call(engine, a, b, tol_int, min_run, mask):
    """_align_call for the variants: a = (words, first, skip, zero or None), b likewise or None for self mode."""
    def once(capacity):
        kw = dict(tol_int=tol_int, min_run=min_run, variant_mask=mask, a_skip=a[2], capacity=capacity, a_zero=a[3])
        if b is not None:
            kw.update(b_hashes=b[0], b_first=b[1], b_skip=b[2], b_zero=b[3])
        return align_windows_variants_host(a[0], a[1], **kw) if engine is None else engine.align_windows_variants(a[0], a[1], **kw)
    rec, found = once(ALIGN_FIRST_CAPACITY)
    if found > len(rec):
        rec, found = once(found)
    return rec


def _seed_flipped_call(engine, a, b, tol_int, min_run, mask):
    """_seed_call for the variants: the candidate triples of one call, VIDEO_PAIR_VARIANT_DTYPE in (variant, a, b) order."""
    def once(capacity):
        kw = dict(tol_int=tol_int, min_run=min_run, variant_mask=mask, a_skip=a[2], capacity=capacity, a_zero=a[3])
        if b is not None:
            kw.update(b_hashes=b[0], b_first=b[1], b_skip=b[2], b_zero=b[3])
        return align_seed_pairs_variants_host(a[0], a[1], **kw) if engine is None else engine.align_seed_pairs_variants(a[0], a[1], **kw)
    t, found = once(ALIGN_FIRST_CAPACITY)
    if found > len(t):
        t, found = once(found)
    return t


def _align_flipped_pairs_call(engine, a, b, tol_int, min_run, triples):
    """_align_flipped_call on a list of (variant, a, b) triples."""
    def once(capacity):
        kw = dict(tol_int=tol_int, min_run=min_run, a_skip=a[2], capacity=capacity, a_zero=a[3])
        if b is not None:
            kw.update(b_hashes=b[0], b_first=b[1], b_skip=b[2], b_zero=b[3])
        if engine is None:
            return align_windows_variants_pairs_host(a[0], a[1], triples, **kw)
        return engine.align_windows_variants_pairs(a[0], a[1], triples, **kw)
    rec, found = once(ALIGN_FIRST_CAPACITY)
    if found > len(rec):
        rec, found = once(found)
    return rec


def _flipped_triples(pairs, flips, n_a, n_b, self_mode):
    """The `pairs` keyword of align_flipped - {flip: [(a, b)]} or one list for all flips - as VIDEO_PAIR_VARIANT_DTYPE in (variant, a, b)
    order, every flip's list checked as the library checks the list of a *_pairs call.  None stays None."""
    if pairs is None:
        return None
    parts = []
    for f in sorted(set(flips), key=int):
        one = pairs.get(f, pairs.get(int(f), [])) if isinstance(pairs, dict) else pairs
        p = _align_pair_list(one, n_a, n_b, self_mode)
        t = np.zeros(len(p), VIDEO_PAIR_VARIANT_DTYPE)
        t["a"], t["b"], t["variant"] = p["a"], p["b"], int(f)
        parts.append(t)
    return np.concatenate(parts) if parts else np.zeros(0, VIDEO_PAIR_VARIANT_DTYPE)


def _block_triples(engine, A, B, a0, a1, b0, b1, tol_int, min_run, mask, triple_list, seed):
    """_block_pairs for the variants: the (variant, a, b) of one block of videos that are aligned, counted inside the block - those of the
    caller's list, the seeded candidates (vdf_align_seed_pairs_variants), or the candidates that are on the list."""
    tlist = None
    if triple_list is not None:
        sel = (triple_list["a"] >= a0) & (triple_list["a"] < a1) & (triple_list["b"] >= b0) & (triple_list["b"] < b1)
        tlist = triple_list[sel].copy()
        tlist["a"] -= a0
        tlist["b"] -= b0
        if not len(tlist):
            return tlist
    if seed:
        cand = _seed_flipped_call(engine, A, B, tol_int, min_run, mask)
        if tlist is None:
            return cand
        key = lambda t: (t["variant"].astype(np.uint64) << np.uint64(60)) | (t["a"].astype(np.uint64) << np.uint64(30)) | t["b"].astype(np.uint64)
        tlist = tlist[np.isin(key(tlist), key(cand))]  # (a block holds at most isqrt(2^24) videos per side: 30 bits hold an index)
    return tlist


def candidate_pairs_flipped(windows_a: List[List[VideoHash]], windows_b: Optional[List[List[VideoHash]]] = None,
                            tolerance: float = DEFAULT_SEARCH_TOLERANCE, min_run: int = 1, flips: Sequence = (Flip.X,), static_a=None, static_b=None,
                            engine: Optional[Engine] = None) -> dict:
    """Which pairs of videos can share a flipped stretch at all?  Arguments as `align_flipped`; -> {flip: [(a, b)]}, each list in (a, b) order:
    the pairs with a window ka of a, ka a multiple of min_run, and a window of the flipped b within `tolerance` of each other, neither static
    (include/vdf.h: vdf_align_seed_pairs_variants).  Every pair align_flipped reports under a flip is among that flip's candidates.  On an
    engine all flips come from one pass over the seeds."""
    self_mode = windows_b is None
    flips = [Flip(int(f)) for f in flips]
    if any(not 1 <= int(f) <= 7 for f in flips):
        raise ValueError("flips are non-empty combinations of Flip.X, Flip.Y, Flip.T")
    tol_int = tolerance_int(tolerance)
    wa, fa, ka, ca = _align_csr(windows_a, static_a)
    wb, fb, kb, cb = (wa, fa, ka, ca) if self_mode else _align_csr(windows_b, static_b)
    zb = _align_zero(windows_a if self_mode else windows_b, "windows_a" if self_mode else "windows_b")
    if not flips:
        return {}
    mask = 0
    for f in flips:
        mask |= 1 << int(f)
    if engine is None:
        cells = (sum(ca) ** 2 - sum(n * n for n in ca)) // 2 if self_mode else sum(ca) * sum(cb)
        if cells * len(flips) > ALIGN_HOST_CELLS:
            engine = default_engine()

    def block(words, first, skip, zero, lo, hi):
        w0, w1 = int(first[lo]), int(first[hi])
        return words[w0:w1], first[lo:hi + 1] - first[lo], None if skip is None else skip[w0:w1], None if zero is None else zero[w0:w1]

    step = max(1, math.isqrt(ALIGN_MAX_PAIRS))
    out = {f: [] for f in flips}
    for a0 in range(0, len(ca), step):
        a1 = min(a0 + step, len(ca))
        for b0 in range(a0 if self_mode else 0, len(cb), step):
            b1 = min(b0 + step, len(cb))
            same = self_mode and b0 == a0
            A = block(wa, fa, ka, zb if same else None, a0, a1)
            t = _seed_flipped_call(engine, A, None if same else block(wb, fb, kb, zb, b0, b1), tol_int, int(min_run), mask)
            for v, a, b in zip(t["variant"], t["a"], t["b"]):
                out[Flip(int(v))].append((int(a) + a0, int(b) + b0))
    return {f: sorted(p) for f, p in out.items()}


def align_flipped(windows_a: List[List[VideoHash]], windows_b: Optional[List[List[VideoHash]]] = None, tolerance: float = DEFAULT_SEARCH_TOLERANCE,
                  min_run: int = 1, stride: int = 1, flips: Sequence = (Flip.X,), static_a=None, static_b=None,
                  engine: Optional[Engine] = None, pairs=None, seed: bool = False) -> dict:
    """`align` against the mirrored / flipped / reversed videos of windows_b - the re-upload that is mirrored AND has its intro trimmed, which
    neither search_flipped (frames 0 ... 15 of a file) nor align (unflipped stretches) sees: {flip: [FlippedAlignment]} for every flip of `flips`,
    each list ordered by (a, b) with at most one entry per pair, by align's rules on the window hashes of the flipped b (derived from b's hashes
    and zero planes; include/vdf.h: vdf_align_windows_variants).  windows_b None: the videos of windows_a against each other's flips, every
    pair once (a < b), never a video against its own mirror.  The hashes of the flipped side (windows_b, or windows_a in self mode) need their
    zero planes (hash_frame_windows with zero_plane=True), else VidProc.  With Flip.T the matched stretch of b plays backwards
    (FlippedAlignment); it lies on b's window grid, i.e. reversed b is taken from its last window's last frame.  Near the tolerance a stretch
    can show with b flipped and not with the sides swapped: b's zero plane clears bits of the flipped hash that a may have set.
    pairs: only these are aligned - {flip: [(a, b)]}, or one list of (a, b) for every flip; each list strictly increasing in (a, b), a < b when
    windows_b is None (vdf_align_windows_variants_pairs).  seed=True: every block of videos is seeded first (candidate_pairs_flipped: all flips
    from one pass over the seeds) and only its candidates are aligned; the result is the same dict.  With both, the candidates
    on the list."""
    self_mode = windows_b is None
    s = int(stride)
    if s != stride or s < 1:
        raise ValueError("stride must be a positive integer")
    flips = [Flip(int(f)) for f in flips]
    if any(not 1 <= int(f) <= 7 for f in flips):
        raise ValueError("flips are non-empty combinations of Flip.X, Flip.Y, Flip.T")
    tol_int = tolerance_int(tolerance)
    wa, fa, ka, ca = _align_csr(windows_a, static_a)
    wb, fb, kb, cb = (wa, fa, ka, ca) if self_mode else _align_csr(windows_b, static_b)
    zb = _align_zero(windows_a if self_mode else windows_b, "windows_a" if self_mode else "windows_b")
    triple_list = _flipped_triples(pairs, flips, len(ca), len(cb), self_mode)
    if not flips:
        return {}
    mask = 0
    for f in flips:
        mask |= 1 << int(f)
    if engine is None:
        cells = (sum(ca) ** 2 - sum(n * n for n in ca)) // 2 if self_mode else sum(ca) * sum(cb)
        if cells * len(flips) > ALIGN_HOST_CELLS:
            engine = default_engine()

    def block(words, first, skip, zero, lo, hi):
        w0, w1 = int(first[lo]), int(first[hi])
        return words[w0:w1], first[lo:hi + 1] - first[lo], None if skip is None else skip[w0:w1], None if zero is None else zero[w0:w1]

    step = max(1, math.isqrt(ALIGN_MAX_PAIRS))
    parts = []
    for a0 in range(0, len(ca), step):
        a1 = min(a0 + step, len(ca))
        for b0 in range(a0 if self_mode else 0, len(cb), step):
            b1 = min(b0 + step, len(cb))
            same = self_mode and b0 == a0
            A = block(wa, fa, ka, zb if same else None, a0, a1)
            if triple_list is not None or seed:
                B = None if same else block(wb, fb, kb, zb, b0, b1)
                tlist = _block_triples(engine, A, B, a0, a1, b0, b1, tol_int, int(min_run), mask, triple_list, seed)
                if len(tlist):
                    rec = _align_flipped_pairs_call(engine, A, B, tol_int, int(min_run), tlist).copy()
                    rec["a"] += a0
                    rec["b"] += b0
                    parts.append(rec)
                continue
            rec = _align_flipped_call(engine, A, None if same else block(wb, fb, kb, zb, b0, b1), tol_int, int(min_run), mask).copy()
            rec["a"] += a0
            rec["b"] += b0
            parts.append(rec)
    rec = np.concatenate(parts) if parts else np.zeros(0, ALIGN_VARIANT_DTYPE)
    rec = rec[np.lexsort((rec["b"], rec["a"], rec["variant"]))]
    pa = [ws[0].src_path() if ws else None for ws in windows_a]
    pb = pa if self_mode else [ws[0].src_path() if ws else None for ws in windows_b]
    out = {f: [] for f in flips}
    for r in rec:
        a, b, off, st, n, ds, v = (int(r[k]) for k in ("a", "b", "offset", "start_a", "n_windows", "dist_sum", "variant"))
        j0 = st + off                                                  # the stretch's first window of b in the DERIVED order
        kb0 = cb[b] - 1 - (j0 + n - 1) if v & int(Flip.T) else j0      # its first window in b's own order
        out[Flip(v)].append(FlippedAlignment(a, b, (kb0 - st) * s, st * s, kb0 * s, (n - 1) * s + _capi.DCT_SIZE, n, ds / n, pa[a], pb[b], Flip(v)))
    return out


def gen_hashes(frames: np.ndarray, src_paths: Sequence, durations: Sequence[int],
               cropdetect: Cropdetect = Cropdetect.LETTERBOX, engine: Optional[Engine] = None, zero_plane: bool = False) -> List[VideoHash]:
    """The part of `gen_hash` after decode (video_hash_builder.rs:214-223) for a batch of clips:
    crop_video_frames(cropdetect) -- default Letterbox, like CreationOptions::default (:55-63) -- then
    VideoHash::from_frames.  frames [n_clips, n_frames >= 16, H, W] u8, or a LIST of [n_frames >= 16, H, W] stacks of different frame
    sizes (Engine.hash_clips_letterbox; with Cropdetect.NONE hash_frame_stacks).  Detection (frames 0 and 8,
    video_frames_gray.rs:201-210) and the cropped resize both run on the GPU; no cropped copies are made.
    zero_plane: the hashes also carry their zero plane (see hash_frame_stacks); with LETTERBOX the boxes are detected by the letterbox
    call and the planes call then hashes the clips on those boxes, so a flip is the flip of the CROPPED clip."""
    if cropdetect == Cropdetect.NONE:
        return hash_frame_stacks(frames, src_paths, durations, engine, zero_plane)
    if cropdetect != Cropdetect.LETTERBOX:
        raise VidProc("Cropdetect::Motion is not supported by the accelerated path")
    if zero_plane:
        eng = engine or default_engine()
        stacks = list(frames)

        def both():
            _words, crops = eng.hash_clips_letterbox(stacks) if isinstance(frames, (list, tuple)) else eng.hash_frames_letterbox(frames)
            return eng.hash_clips_planes(stacks, crops=crops)
        words, zero = _with_planes(both)
        return [VideoHash(words[i], src_paths[i], durations[i], zero[i]) for i in range(len(words))]
    try:
        eng = engine or default_engine()
        words, _crops = eng.hash_clips_letterbox(frames) if isinstance(frames, (list, tuple)) else eng.hash_frames_letterbox(frames)
    except VdfError as e:
        if e.code == _capi.VDF_E_NOT_ENOUGH_FRAMES:
            raise NotEnoughFrames() from e
        if e.code == _capi.VDF_E_BAD_DIMS:
            raise VidProc(str(e)) from e
        raise
    return [VideoHash(words[i], src_paths[i], durations[i]) for i in range(len(words))]


def cropdetect_letterbox(frames: np.ndarray, engine: Optional[Engine] = None) -> List[Crop]:
    """cropdetect_letterbox (vid_dup_finder_common/src/video_frames_gray.rs:201-210) for a batch of clips on the GPU: frames
    [n_clips, n_frames >= 16, H, W] u8 (or a list of [n_frames >= 16, H, W] stacks of different frame sizes) -> the union (crop.rs:53-68) of the letterbox crops of frames 0 and 8 of each clip."""
    mixed = isinstance(frames, (list, tuple))
    try:
        eng = engine or default_engine()
        _words, crops = eng.hash_clips_letterbox(frames) if mixed else eng.hash_frames_letterbox(frames)
    except VdfError as e:
        if e.code == _capi.VDF_E_NOT_ENOUGH_FRAMES:
            raise NotEnoughFrames() from e
        if e.code == _capi.VDF_E_BAD_DIMS:
            raise VidProc(str(e)) from e
        raise
    crops = np.asarray(crops).reshape(-1, 4)
    if mixed:
        return [Crop.from_abi((int(np.shape(s)[2]), int(np.shape(s)[1])), c) for s, c in zip(frames, crops)]
    h, w = int(frames.shape[2]), int(frames.shape[3])
    return [Crop.from_abi((w, h), c) for c in crops]
