"""vid_dup_finder_lib_amd: MI355X-native VideoHash construction + Hamming search behind the
vid_dup_finder_lib API (VideoHash / search / search_with_references / MatchGroup).

The compute path is hand-written HIP for gfx950 in csrc/, reached through the C ABI of
include/vdf.h (libvdf_hip.so).  There is no CPU fallback.
"""
from ._capi import (DEFAULT_SEARCH_TOLERANCE, HASH_BITS, HASH_WORDS, TOLERANCE_SCALING_FACTOR, VdfError)
from .api import (Alignment, AlignmentStretch, FlippedAlignment, RetimedAlignment, align, align_all, align_flipped, align_rates, align_rates_all, align_retimed, best_rates, best_rates_all, RetimedAlignmentStretch, candidate_pairs, candidate_pairs_flipped, candidate_pairs_rates, static_windows, Crop, Cropdetect, Flip, search_flipped, cropdetect_letterbox, Error, MatchGroup, gen_hashes, NotEnoughFrames, NotVideo, TooFewEntries, VideoHash, VidProc, default_engine,
                  hash_frame_stacks, hash_frame_windows, locate, rust_path_key, search, search_with_references, sort_order)
from .engine import (ALIGN_DTYPE, ALIGN_STRETCH_DTYPE, ALIGN_VARIANT_DTYPE, Engine, align_windows_host, align_windows_stretches_host, align_windows_variants_host,
                     window_variants_host, VIDEO_PAIR_DTYPE, align_seed_pairs_host, align_windows_pairs_host, align_windows_stretches_pairs_host,
                     VIDEO_PAIR_VARIANT_DTYPE, align_seed_pairs_variants_host, align_windows_variants_pairs_host, window_class_layout_host, hash_windows_first, hash_windows_first_retimed, hash_window_count_retimed,
                     hash_window_count_rates, hash_windows_first_rates, ALIGN_RETIMED_DTYPE, align_windows_retimed_host, align_windows_retimed_pairs_host,
                     VIDEO_PAIR_RATE_DTYPE, align_seed_pairs_rates_host, ALIGN_RATE_DTYPE, align_windows_rates_host, ALIGN_RATE_STRETCH_DTYPE, align_windows_rates_stretches_host)

__all__ = ["Crop", "Cropdetect", "cropdetect_letterbox", "gen_hashes", "VideoHash", "MatchGroup", "Error", "NotEnoughFrames", "NotVideo", "VidProc", "TooFewEntries", "search",
           "search_with_references", "search_flipped", "Flip", "hash_frame_stacks", "hash_frame_windows", "locate", "align", "Alignment", "static_windows", "Engine", "default_engine", "VdfError", "rust_path_key",
           "sort_order", "DEFAULT_SEARCH_TOLERANCE", "TOLERANCE_SCALING_FACTOR", "HASH_BITS", "HASH_WORDS", "ALIGN_DTYPE", "align_windows_host",
           "align_flipped", "FlippedAlignment", "ALIGN_VARIANT_DTYPE", "align_windows_variants_host", "window_variants_host",
           "align_all", "AlignmentStretch", "ALIGN_STRETCH_DTYPE", "align_windows_stretches_host",
           "candidate_pairs", "VIDEO_PAIR_DTYPE", "align_seed_pairs_host", "align_windows_pairs_host", "align_windows_stretches_pairs_host",
           "candidate_pairs_flipped", "VIDEO_PAIR_VARIANT_DTYPE", "align_seed_pairs_variants_host", "align_windows_variants_pairs_host", "window_class_layout_host",
           "hash_windows_first", "hash_windows_first_retimed", "hash_window_count_retimed", "align_retimed", "RetimedAlignment",
           "ALIGN_RETIMED_DTYPE", "align_windows_retimed_host", "align_windows_retimed_pairs_host", "hash_window_count_rates", "hash_windows_first_rates", "align_rates", "best_rates",
           "candidate_pairs_rates", "VIDEO_PAIR_RATE_DTYPE", "align_seed_pairs_rates_host", "ALIGN_RATE_DTYPE", "align_windows_rates_host",
           "align_rates_all", "best_rates_all", "RetimedAlignmentStretch", "ALIGN_RATE_STRETCH_DTYPE", "align_windows_rates_stretches_host"]
