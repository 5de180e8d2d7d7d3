// Internal declarations shared by the HIP translation units and the C-ABI layer.
// Nothing here is part of the public boundary (include/vdf.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vdf.h"
#include "hash_variant.h"
#include "window_variant.h"
#include "resize_dispatch.h"
#include "windows_plan.h"
#include "windows_mixed_plan.h"
#include "windows_retimed_plan.h"
#include "windows_mixed_retimed_plan.h"
#include "windows_rates_plan.h"
#include "windows_mixed_rates_plan.h"
#include "align_plan.h"
#include "align_retimed_plan.h"
#include "align_rates_plan.h"
#include "align_rates_stretch_plan.h"

namespace vdf {

// ---- Hamming search tiling -------------------------------------------------------------------
// One workgroup = 4 waves; every lane keeps ROWS_PER_LANE target hashes in VGPRs and streams the
// candidate hashes through SGPRs (scalar loads), so a workgroup covers TILE_ROWS targets.
constexpr int kDefaultRowsPerLane = 2;                       // tile = 256 * rows-per-lane targets
constexpr uint32_t kDefaultChunkCols = 2048;                // candidates per workgroup

struct SearchLaunch {
    // rows (targets / references)
    const uint32_t *row_hashes;  // [n_rows][32] dwords
    const uint32_t *row_perm;    // nullable: row position -> index into row_hashes / reported row
    uint32_t n_rows;
    uint32_t row_index_base;     // added to the reported row
    // columns (candidates)
    const uint32_t *col_hashes;  // [n_cols][32]
    uint32_t n_cols;
    // fp4-expanded copies for the MFMA backend ([n_pad][512 B], zero padded); null for the VALU backend
    const void *row_exp, *col_exp;
    // popcounts of rows / columns as floats: [pop | popk | popkT] x n_pad
    const float *row_pop3 = nullptr, *col_pop3 = nullptr;
    uint32_t row_pad = 0, col_pad = 0;
    void *cand = nullptr;                 // suspect queue of the MFMA kernel (16-byte entries, pre-filled with 0xFF)
    uint32_t cand_capacity = 0;
    unsigned long long *cand_head = nullptr;  // next free slot (advanced in per-wave chunks; keeps counting past a full queue)
    // windows + tiles (device scratch, filled by launch_windows_tiles)
    uint32_t *row_lo, *row_hi;   // [n_row_tiles * tile_rows]
    uint32_t *tile_lo, *tile_hi, *tile_first, *tile_count, *tile_offset;  // [n_row_tiles (+1)]
    uint32_t *group_cmin, *group_offset, *group_blocks;  // [n_groups (+1)]: chunk-major grouped order (MFMA backend), else null
    int prune_step = 16;                  // MFMA backend: k-step after which a block that cannot contain a hit stops (16 = never)
    uint32_t shard_index = 0, shard_count = 1;  // row tiles t with t % shard_count == shard_index are this launch's
    uint32_t n_groups, group_size;        // n_groups = 0 for the VALU backend (compact tile list)
    uint32_t n_row_tiles;
    uint32_t tile_rows;          // 256 * rows-per-lane (256, 512 or 1024)
    uint32_t chunk_cols;
    uint32_t tol;
    const uint32_t *matched;     // nullable bitmap over column indices (self mode: rows too)
    int self_mode;
    // output
    vdf_hit *hits;
    unsigned long long capacity;
    unsigned long long *counters;  // [0] hits produced, [1] pairs computed, [2] pairs admitted
    uint32_t *overflow_row;
};

// mode 0: self-search windows [i+1, rhs(i));  mode 1: reference windows [lhs(r), rhs(r)).
hipError_t launch_windows_tiles(int mode, const uint32_t *col_dur, uint32_t n_cols, const uint32_t *row_dur,
                                const uint32_t *row_perm, uint32_t n_rows, uint32_t row_begin, uint32_t row_end,
                                uint32_t shard_index, uint32_t shard_count, const SearchLaunch &L,
                                hipStream_t stream);
hipError_t launch_hamming_tiles(const SearchLaunch &L, uint32_t total_tiles, hipStream_t stream);
// MFMA backend: {0, 1} fp4 encoding, exact.  Rows are padded to a multiple of the tile, columns by a further 128.
constexpr uint32_t kMfmaRowPad = 512, kMfmaColPad = 128;  // kMfmaRowPad = rows of the largest MFMA workgroup tile (8 waves x 64 rows)
// {0, 1} nibbles + popcount arrays pop3 = [pop | popk | popkT] of n_pad floats each
hipError_t launch_expand_fp4(const uint32_t *packed, uint32_t n, uint32_t n_pad, void *expanded, uint32_t k_steps,
                             float *pop3, hipStream_t stream);
hipError_t launch_hamming_tiles_mfma2(const SearchLaunch &L, uint32_t total_tiles, hipStream_t stream);  // branch-free stream; tile_rows 512 or 256
hipError_t launch_resolve_candidates(const SearchLaunch &L, hipStream_t stream);  // its second pass: suspects evaluated exactly
// drops the hits of rows that can never become targets of the greedy replay (hamming.hip); needs the COMPLETE hit set: a sharded
// launch ORs has_in (after step 1) and covered (after step 2) over its shards.  bitmaps = has_in | covered, ceil(n_entries / 32) words each
hipError_t launch_filter_mark_incoming(const vdf_hit *hits, unsigned long long n_hits, uint32_t n_entries, uint32_t *bitmaps, hipStream_t stream);
hipError_t launch_filter_mark_covered(const vdf_hit *hits, unsigned long long n_hits, uint32_t n_entries, uint32_t *bitmaps, hipStream_t stream);
hipError_t launch_filter_compact(const vdf_hit *hits, unsigned long long n_hits, uint32_t n_entries, const uint32_t *bitmaps, vdf_hit *out,
                                 unsigned long long *counter, hipStream_t stream);
hipError_t launch_bitmap_or(uint32_t *dst, const uint32_t *srcs, size_t n_words, uint32_t n_srcs, hipStream_t stream);  // dst |= OR of n_srcs bitmaps
hipError_t launch_group_max_distance(const uint32_t *hashes, const unsigned long long *offsets,
                                     const unsigned long long *members, const uint32_t *ref_hashes,
                                     const long long *ref_index, uint32_t n_groups, uint32_t *out, hipStream_t stream);

// ---- hash construction -----------------------------------------------------------------------
struct ResizeAxisTable {  // device pointers, one axis
    const int32_t *start;  // [16]
    const int32_t *size;   // [16]
    const int16_t *w;      // [16][window]
    int32_t window;
    int32_t precision;
};

hipError_t launch_resize_generic(const uint8_t *frames, size_t n_clips, uint32_t w, uint32_t h, size_t frame_stride,
                                 size_t clip_stride, ResizeAxisTable th, ResizeAxisTable tv, int need_h, int need_v,
                                 int32_t y_first, int32_t tmp_rows, uint8_t *small, hipStream_t stream);
struct MfmaResizeArgs {  // device pointers to the MFMA-layout tables (resize_tables.h: MfmaAxisTable)
    const void *bh, *av;
    const int32_t *bias_h, *bias_v;
    int32_t prec_h, prec_v, n_kt, n_rg;
    const int32_t *band_meta = nullptr;  // bh in band form (resize_tables.h): kt_lo[16], nt[16] on the device
    int32_t band_stride = 0;
    int32_t persistent_wgs_per_cu = 3; // resident workgroups per CU for the persistent kernel
};
// The launchers take the route and its values from the plan (resize_dispatch.h: plan_hash) and only guard their kernels' preconditions.
// plan.route = kPersistentOneTile, kTiled or kPerClipFused
hipError_t launch_resize_dct_fused(const uint8_t *frames, size_t n_clips, uint32_t w, uint32_t h, size_t frame_stride,
                                   size_t clip_stride, const uint8_t *buf_end, const MfmaResizeArgs &a, const HashPlan &plan,
                                   const double *cos_table, uint64_t *out_hashes, uint32_t *out_dontcare,
                                   hipStream_t stream, uint64_t *out_zero = nullptr);
// the whole-line kernel (a.av in kMfmaLayoutVerticalWide order)
hipError_t launch_resize_mfma_frames(const uint8_t *frames, size_t n_clips, uint32_t w, uint32_t h,
                                     size_t frame_stride, size_t clip_stride, const uint8_t *buf_end,
                                     const MfmaResizeArgs &a, uint8_t *small, hipStream_t stream);
// linear-stream form for tightly packed frames whose width is a multiple of 16 but not of the 128-byte line
// (a.av in kMfmaLayoutVertical order); plan.route = kChunkStream (a.bh plain, plan.nb blocks per chunk) or kWaveStream (a.bh in band form,
// plan.waves waves per workgroup)
// clips / tables (both or neither): per-clip row ranges - clip c contributes rows y0 .. y0 + h of its frames (full-width crop
// boxes: top / bottom letterbox bars), resized with vertical table entry v_table; a.av / a.bias_v / a.prec_v / a.n_rg are then unused
struct CropStreamClip;
struct CropStreamTable;
hipError_t launch_resize_mfma_frames_stream(const uint8_t *frames, size_t n_clips, uint32_t w, uint32_t h,
                                            size_t frame_stride, size_t clip_stride, const MfmaResizeArgs &a, const HashPlan &plan,
                                            uint8_t *small, hipStream_t stream, const CropStreamClip *clips = nullptr,
                                            const CropStreamTable *tables = nullptr);
// K-split form for wide frames (1024..4096 columns, a multiple of 16): horizontal table in registers, a.bh in plain
// kMfmaLayoutHorizontal form, a.av in kMfmaLayoutVertical order; plan.route = kKsplit, plan.nb blocks per chunk
hipError_t launch_resize_mfma_frames_ksplit(const uint8_t *frames, size_t n_clips, uint32_t w, uint32_t h,
                                            size_t frame_stride, size_t clip_stride, const MfmaResizeArgs &a, const HashPlan &plan,
                                            uint8_t *small, hipStream_t stream, const CropStreamClip *clips = nullptr,
                                            const CropStreamTable *tables = nullptr);
// ---- letterbox crop detection + cropped resize -------------------------------------------
struct CropClipDesc {  // per clip: crop box inside the W x H frame and the table entries for its size
    uint32_t x0, y0, w, h;
    uint32_t h_table, v_table;
    uint32_t src_clip, pad;  // which clip of the caller's batch (a launch may cover a subset: see CropStreamClip::src_clip)
};
struct CropTableEntry {  // one MFMA-layout axis table (device pointers)
    const void *operand;
    const int32_t *bias;
    int32_t n_tiles, precision;
};
// The same for the linear-stream form (resize_mfma_cropped_stream_kernel): LDS row pitch, the chunk geometry and the
// reciprocal the DMA lanes divide by are fixed per clip on the host; the horizontal table is in band form
struct CropStreamClip {
    uint32_t x0, y0, w, h;
    uint32_t wp, nb, n_chunks, src_clip;  // LDS pitch (odd multiple of 16 >= w + 3, or the frame pitch for a full-width box), 16-row blocks per chunk, chunks per frame;
                                          // src_clip: which clip of the caller's batch this entry is (a launch may cover a subset of the batch: frames are
                                          // read from, and the 16 x 16 results written to, clip src_clip's place)
    uint32_t h_table, v_table, step_rows, step_x;  // 4096 = step_rows * wp + step_x: what one DMA instruction advances a lane by
};
struct CropStreamTable {
    const void *operand;
    const int32_t *bias;
    const int32_t *meta;  // band form: kt_lo[16], nt[16] (horizontal tables only)
    int32_t n_tiles, precision, band_stride, pad;
};
hipError_t launch_resize_mfma_cropped_stream(const uint8_t *frames, size_t n_clips, uint32_t pitch, uint32_t frame_rows,
                                             size_t frame_stride, size_t clip_stride, const CropStreamClip *clips,
                                             const CropStreamTable *tables, int cls, bool shift, uint8_t *small,
                                             hipStream_t stream);  // shift: some row of some box starts off a dword boundary
// crop boxes that share their column range (x0, box_w; e.g. the 4 : 3 picture of every pillarboxed clip in a 16 : 9 batch): the per-wave
// stream kernel gathers the box's bytes of each row; a = the band table of box_w; waves = the group's (CropBoxGroup); per-clip rows as in the ROWCROP launches
hipError_t launch_resize_mfma_box_wavestream(const uint8_t *frames, size_t n_clips, uint32_t w, uint32_t h, size_t frame_stride,
                                             size_t clip_stride, const MfmaResizeArgs &a, uint32_t x0, uint32_t box_w, int waves,
                                             const CropStreamClip *clips, const CropStreamTable *tables, uint8_t *small, hipStream_t stream);
// work: scratch of letterbox_work_bytes(n_clips, frames_per_clip) bytes (the list of frames whose side bars a second pass walks)
size_t letterbox_work_bytes(size_t n_clips, uint32_t frames_per_clip);
// side_strips: 0 = by frame height (32 column strips per pass from 512 rows, 16 from 256, else 8), 16 = at most 16 (VDF_LB_NC16: A/B runs)
hipError_t launch_letterbox(const uint8_t *frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h,
                            size_t frame_stride, size_t clip_stride, uint32_t *crops, uint32_t *work, hipStream_t stream, int side_strips = 0);
// small frames (at most 128 rows, 256 columns): one workgroup per clip, resize + DCT + hash; vertical tables in kMfmaLayoutVertical order
hipError_t launch_resize_dct_cropped_small(const uint8_t *frames, size_t n_clips, uint32_t pitch, size_t frame_stride,
                                           size_t clip_stride, const uint8_t *buf_end, const CropClipDesc *desc,
                                           const CropTableEntry *tables, const double *cos_table, uint64_t *out_hashes,
                                           uint32_t *out_dontcare, hipStream_t stream, uint64_t *out_zero = nullptr);
// the same kernel fed from the device (round 6): boxes = the detect's output [n_clips][4] {left, right, top, bottom} in device memory, tables = the
// (w, h) set of ALL box sizes - horizontal table of box width bw at [bw], vertical table of box height bh at [w + 1 + bh] (api.cpp: box_table_set)
hipError_t launch_resize_dct_cropped_small_boxes(const uint8_t *frames, size_t n_clips, uint32_t w, uint32_t h, size_t frame_stride,
                                                 size_t clip_stride, const uint8_t *buf_end, const uint32_t *boxes,
                                                 const CropTableEntry *tables, const double *cos_table, uint64_t *out_hashes,
                                                 uint32_t *out_dontcare, hipStream_t stream);
// The same two passes on clips of different frame sizes (resize_dispatch.h: plan_letterbox_mixed gives descriptors, launches and the size of `work`).
// d_desc: DEVICE descriptors, every probed frame inside the buffer (check_mixed); crops: DEVICE [n_clips][4], every slot of the plan written.
hipError_t launch_letterbox_mixed(const uint8_t *buf, const LetterboxProbeDesc *d_desc, const LetterboxMixedLaunch *launches, size_t n_launches, size_t n_clips,
                                  uint32_t *crops, uint32_t *work, hipStream_t stream);
// frames of at most 64 x 64: detect + crop + resize + DCT + hash in one persistent kernel (dct_hash.hip: letterbox_resize_dct_hash_small_kernel).
// Every clip's 16-byte loads must stay inside the caller's buffer: the caller keeps the clips within 64 bytes of its end out of this launch.
// box_tables: the set's tables at kSmallBoxTableStride bytes each, in the order above: operand hi | lo (2 x 1024 B), bias[16], precision.
// out_crops: DEVICE [n_clips][4], always written.  wgs_per_cu: 0 = what fits.
constexpr uint32_t kSmallBoxTableStride = 2176;
hipError_t launch_letterbox_hash_small(const uint8_t *frames, size_t n_clips, uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride,
                                       const void *box_tables, const double *cos_table, uint64_t *out_hashes, uint32_t *out_dontcare,
                                       uint32_t *out_crops, int wgs_per_cu, hipStream_t stream);
hipError_t launch_resize_mfma_cropped(const uint8_t *frames, size_t n_clips, uint32_t pitch, size_t frame_stride,
                                      size_t clip_stride, const uint8_t *buf_end, const CropClipDesc *desc,
                                      const CropTableEntry *tables, uint8_t *small, bool wide, hipStream_t stream);
// ---- clips of different frame sizes in one call (vdf_hash_clips_u8[_device]) --------------------------------------------------------------
// desc: DEVICE MixedClipDesc (resize_dispatch.h, where the host-only planner fills them and asserts the layout the kernels read), this launch's
// first; h_table / v_table index `tables`.  buf_end = buf + buf_bytes of the ONE buffer every clip's offset is relative to.  At most
// kMaxClipsPerLaunch clips per launch.
hipError_t launch_mixed_small(const uint8_t *buf, const uint8_t *buf_end, const MixedClipDesc *desc, size_t n_clips, const CropTableEntry *tables,
                              const double *cos_table, uint64_t *out_hashes, uint32_t *out_dontcare, hipStream_t stream, uint64_t *out_zero = nullptr);
// small: this launch's first 4 KB slot; wide: whole-line loads, vertical tables in kMfmaLayoutVerticalWide order
hipError_t launch_mixed_frames(const uint8_t *buf, const uint8_t *buf_end, const MixedClipDesc *desc, size_t n_clips, const CropTableEntry *tables,
                               bool wide, uint8_t *small, hipStream_t stream);
// slot i of small -> the hash of clip desc[i].out_index
hipError_t launch_dct_hash_indexed(const uint8_t *small, const MixedClipDesc *desc, size_t n_clips, const double *cos_table, uint64_t *out_hashes,
                                   uint32_t *out_dontcare, hipStream_t stream, uint64_t *out_zero = nullptr);
// ---- Search::sort on the device (sort_order.hip) ----------------------------------------------------------------
// perm_out = the stable order by (duration, path rank); rank nullable (all paths equal).  scratch from sort_order_scratch_bytes.
size_t sort_order_scratch_bytes(uint32_t n, bool with_rank);
hipError_t launch_sort_order(const uint32_t *dur, const uint32_t *rank, uint32_t n, uint32_t *perm_out, void *scratch,
                             size_t scratch_bytes, hipStream_t stream);
// Search::sort's order of cache entries computed from their PATHS on the device (sort_order.hip): facts first (are the paths plain, how
// long, what do they share: 16 bytes {not_plain, max_len, shared, pad} at d_facts16), then the stable order by (duration, path).
hipError_t launch_path_facts(const char *d_blob, const unsigned long long *d_off, const uint32_t *d_sel, uint32_t n, void *d_facts16, hipStream_t stream);
size_t path_order_scratch_bytes(uint32_t n);
hipError_t launch_path_duration_order(const char *d_blob, const unsigned long long *d_off, const uint32_t *d_sel, const uint32_t *d_dur, uint32_t n,
                                      uint32_t first_word, uint32_t n_words, uint32_t *order_out, void *scratch, size_t scratch_bytes,
                                      hipStream_t stream);
// hashes_out[k] = hashes[perm[k]], dur_out[k] = dur[perm[k]] (dur / dur_out nullable)
// hit list into (row, col) order, in place on the device; rows < 2^row_bits
size_t sort_hits_scratch_bytes(size_t n);
hipError_t launch_sort_hits(vdf_hit *hits, size_t n, unsigned row_bits, void *scratch, size_t scratch_bytes, hipStream_t stream,
                            unsigned col_bits = 32);  // columns < 2^col_bits
hipError_t launch_gather_hashes(const uint64_t *hashes, const uint32_t *dur, const uint32_t *perm, uint32_t n, uint64_t *hashes_out,
                                uint32_t *dur_out, hipStream_t stream);
hipError_t launch_dct_hash(const uint8_t *small, size_t small_clip_stride, size_t small_frame_stride, size_t n_clips,
                           const double *cos_table, uint64_t *out_hashes, uint32_t *out_dontcare, hipStream_t stream, uint64_t *out_zero = nullptr);
// ---- the zero plane and the hashes of the flipped clips -------------------------------------------------------------------
// out_zero (above; nullable): the launch runs its kernels' PLANES instantiations and writes 16 words per clip - bit i set iff coefficient i
// of the clip is 0.0 - beside the hashes.  Null: the plain instantiations, as before.
// out[j][c][16] = the hash of clip c flipped by variants[j] (0 ... 7; at most 8 entries, n <= 2^32 - 1)
hipError_t launch_hash_variants(const uint64_t *hashes, const uint64_t *zero, size_t n, const uint32_t *variants, uint32_t n_variants, uint64_t *out,
                                hipStream_t stream);
// ---- every 16-frame window of a clip (windows_plan.h) -------------------------------------------------------------------------
// Where the 16 x 16 frames of the clips are: frame f of clip c at base + c clip_stride + (f / 16) chunk_stride + (f % 16) frame_stride for
// f < main_frames, else at tail + c tail_clip_stride + 256 (f - tail_first).  dwords: every frame starts on a 4-byte boundary.
struct WindowsFrames {
    const uint8_t *base, *tail;
    size_t clip_stride, chunk_stride, frame_stride, tail_clip_stride;
    uint32_t main_frames, tail_first;
    bool dwords;
};
// out_hashes[16 (c n_win + k)] = the hash of frames [k stride, k stride + 16) of clip c; out_dontcare (nullable) at c n_win + k
// out_zero (nullable): the kernel's PLANES form, the windows' zero planes at out_zero + 16 (c n_win + k); null: the plain form, as before
hipError_t launch_dct_hash_windows(const WindowsFrames &f, size_t n_clips, const WindowsPlan &plan, const double *cos_table, uint64_t *out_hashes,
                                   uint32_t *out_dontcare, hipStream_t stream, uint64_t *out_zero = nullptr);
// ---- window hashes of videos of different sizes and lengths (windows_mixed_plan.h) ---------------------------------------------
// small: the 16 x 16 frames of every pseudo-clip of the plan, slot s at small + 4096 s; videos / seg_first: DEVICE copies of the plan's records and
// of its segment table (n_videos + 1 entries); n_groups = seg_first[n_videos].  Window k of video i to row first[i] + k of the outputs.
hipError_t launch_dct_hash_windows_mixed(const uint8_t *small, const WindowsVideoRecord *videos, const uint32_t *seg_first, uint32_t n_videos,
                                         uint32_t n_groups, uint32_t stride, uint32_t per_seg, const double *cos_table, uint64_t *out_hashes,
                                         uint32_t *out_dontcare, hipStream_t stream, uint64_t *out_zero = nullptr);
// ---- retimed window hashes (windows_retimed_plan.h) ---------------------------------------------------------------------------
// out_hashes[16 (c n_win + k)] = the hash of the 16 frames k stride + tap(i) of clip c; out_dontcare (nullable) at c n_win + k
hipError_t launch_dct_hash_windows_retimed(const WindowsFrames &f, size_t n_clips, const WindowsRetimedPlan &plan, const double *cos_table,
                                           uint64_t *out_hashes, uint32_t *out_dontcare, hipStream_t stream);
// ---- retimed window hashes of videos of different sizes and lengths (windows_mixed_retimed_plan.h) -----------------------------
// small, videos, seg_first, n_groups as launch_dct_hash_windows_mixed (n_win, first and seg_first of the records: the retimed ones); rate: stride,
// span, taps and per_seg of the call.  Grids are cut at kMaxWindowGroupsPerLaunch.
hipError_t launch_dct_hash_windows_mixed_retimed(const uint8_t *small, const WindowsVideoRecord *videos, const uint32_t *seg_first, uint32_t n_videos,
                                                 uint32_t n_groups, const WindowsRetimedPlan &rate, const double *cos_table, uint64_t *out_hashes,
                                                 uint32_t *out_dontcare, hipStream_t stream);
// ---- retimed window hashes at several rates from one read of the frames (windows_rates_plan.h) -----------------------------------
// window k of clip c at rate r to row plan.a.out_first[r] + c n_win_r + k of out_hashes (16 words a row) and of out_dontcare (nullable)
hipError_t launch_dct_hash_windows_rates(const WindowsFrames &f, size_t n_clips, const WindowsRatesPlan &plan, const double *cos_table,
                                         uint64_t *out_hashes, uint32_t *out_dontcare, hipStream_t stream);
// ---- retimed window hashes of a mixed library at several rates (windows_mixed_rates_plan.h) --------------------------------------
// small, videos, seg_first, n_groups as launch_dct_hash_windows_mixed (the records' n_win and seg_first: of the rate with the most windows); row0:
// DEVICE copy of the plan's [n_rates][n_videos] table.  Window k of video i at rate r to row row0[r n_videos + i] + k.  Grids are cut at
// kMaxWindowGroupsPerLaunch.
hipError_t launch_dct_hash_windows_mixed_rates(const uint8_t *small, const WindowsVideoRecord *videos, const uint32_t *seg_first, const uint32_t *row0,
                                               uint32_t n_videos, uint32_t n_groups, uint32_t stride, uint32_t per_seg, const WindowsMixedRatesArgs &rates,
                                               const double *cos_table, uint64_t *out_hashes, uint32_t *out_dontcare, hipStream_t stream);
// ---- the variant of a set of window hashes (window_variant.h) ------------------------------------------------------------------
// rows [row0, row0 + n_rows) = [first[0], first[n_videos]) of out (and of out_skip, if skip is given) from hashes / zero / skip; variant 0 ... 7
hipError_t launch_window_variants(const uint64_t *hashes, const uint64_t *zero, const uint32_t *first, uint32_t n_videos, const uint8_t *skip,
                                  uint32_t variant, uint32_t row0, uint32_t n_rows, uint64_t *out, uint8_t *out_skip, hipStream_t stream);
// ---- alignment of videos on their window hashes (align_plan.h, align.hip) ---------------------------------------------------
// One chunk of pairs (align_plan.h: align_next_chunk): band kernel, per-pair reduction, dense list in (a, b) order.  All pointers are device
// pointers; scratch holds align_scratch_bytes(n_pairs, n_units).  *dense_out / *total_out: where in scratch the records and their number are
// once the stream has run.
struct AlignLaunch {
    const uint32_t *a_hashes, *a_first;  // [windows][32] dwords, [videos + 1]
    const uint8_t *a_skip;               // nullable, per window
    const uint32_t *b_hashes, *b_first;
    const uint8_t *b_skip;
    const AlignPair *pairs;
    const uint32_t *unit_offset;         // [n_pairs + 1]
    uint32_t n_pairs, n_units;
    uint32_t tol, min_run;
    void *scratch;
    vdf_alignment **dense_out;
    uint32_t **total_out;
    const AlignRect *rects;              // n_rects != 0: the masked kernel, rects[pair * n_rects + i]; 0: the plain kernel
    uint32_t n_rects;                    // 0 ... kAlignMaxStretches - 1
};
size_t align_scratch_bytes(size_t n_pairs, size_t n_units);
hipError_t launch_align_chunk(const AlignLaunch &L, hipStream_t stream);
// One chunk of a retimed call (align_retimed_plan.h: align_retimed_next_chunk): L as above with the chunk's (pair, phase, band)
// units, no rectangles, and L.dense_out unused; num / den in lowest terms.  The same scratch; *dense_out: the records, in (a, b) order.
hipError_t launch_align_retimed_chunk(const AlignLaunch &L, uint32_t num, uint32_t den, vdf_alignment_retimed **dense_out, hipStream_t stream);
// The seed pass of a call (align_plan.h: AlignSeedPlan): every unit's seeds against its rows of B into `bitmap` (n_a x n_b
// bits, cleared by the caller on the stream), then the count and scan of its set bits.  *total_out: where in scratch the number of pairs is
// once the stream has run; launch_align_seed_scatter then writes the first `limit` of them, in (a, b) order.  All pointers are device pointers;
// scratch holds align_seed_scratch_bytes(n_words).
struct AlignSeedLaunch {
    const uint32_t *a_hashes;
    const uint8_t *a_skip;               // nullable, per window
    const uint32_t *seed_window, *seed_video;
    uint32_t n_seeds;
    const uint32_t *b_hashes;
    const uint8_t *b_skip;
    const uint32_t *row_video;           // [n_rows]
    uint32_t row_base, n_rows;
    const unsigned long long *unit_offset;  // [n_chunks + 1]
    const uint32_t *tile_first;          // [n_chunks]
    uint32_t n_chunks;
    uint64_t n_units;
    uint32_t tol;
    int self_mode;
    uint32_t n_b;
    uint32_t *bitmap;
    uint32_t n_words;
    void *scratch;
    uint32_t **total_out;
};
size_t align_seed_scratch_bytes(size_t n_words);
hipError_t launch_align_seed(const AlignSeedLaunch &L, hipStream_t stream);
hipError_t launch_align_seed_scatter(const AlignSeedLaunch &L, vdf_video_pair *out, uint32_t limit, hipStream_t stream);
// The seed pass against the variants.  launch_align_class_layout: n seeds of A (zero == null; row r = window seed_window[r]) or
// n rows of B from window row_base on, into the class-major rows of window_class_layout.h (36 / 72 dwords each).  launch_align_seed_variants:
// every unit's seeds against its tile of 256 rows into `bitmap` - popcount(variant_mask) slots of n_a x n_b bits, the requested variants in
// ascending order, cleared by the caller on the stream - then the count and scan of its set bits; the scatter writes the first `limit`
// triples in (variant, a, b) order.  scratch holds align_seed_scratch_bytes(n_words).
struct AlignSeedVariantsLaunch {
    const uint32_t *seeds;               // [n_seeds][36]
    uint32_t n_seeds;
    const uint32_t *rows;                // [n_rows][72], 16-byte aligned
    const uint32_t *row_video;           // [n_rows]
    uint32_t n_rows;
    const unsigned long long *unit_offset;  // [n_chunks + 1]; the plan is align_seed_plan's at tile_rows = kSeedVariantsTileRows
    const uint32_t *tile_first;          // [n_chunks]
    uint32_t n_chunks;
    uint64_t n_units;
    uint32_t tol;
    int self_mode;
    uint32_t variant_mask;               // bits 1 ... 7
    uint32_t n_a, n_b;
    uint32_t *bitmap;
    uint32_t n_words;
    void *scratch;
    uint32_t **total_out;
};
hipError_t launch_align_class_layout(const uint32_t *hashes, const uint32_t *zero, const uint8_t *skip, const uint32_t *seed_window,
                                     const uint32_t *seed_video, uint32_t row_base, uint32_t n, uint32_t *out, hipStream_t stream);
hipError_t launch_align_seed_variants(const AlignSeedVariantsLaunch &L, hipStream_t stream);
hipError_t launch_align_seed_variants_scatter(const AlignSeedVariantsLaunch &L, vdf_video_pair_variant *out, uint32_t limit, hipStream_t stream);
// The seed pass of the retimed alignment (align_seed_rates_plan.h: AlignSeedRatesPlan): every unit's seeds - of every phase of
// every listed rate - against its tile of gathered rows of B into `bitmap` (n_slots x n_a x n_b bits, cleared by the caller on the stream), then
// the count and scan of its set bits; the scatter writes the first `limit` triples in (rate, a, b) order.  All pointers are device pointers;
// scratch holds align_seed_scratch_bytes(n_words).
struct AlignSeedRatesLaunch {
    const uint32_t *a_hashes;
    const uint8_t *a_skip;               // nullable, per window
    const uint32_t *seed_window, *seed_video, *seed_slot;
    const uint32_t *chunk_first;         // [n_chunks + 1]
    const uint32_t *b_hashes;
    const uint8_t *b_skip;
    const uint32_t *row_window, *row_video;  // [tiles x kSeedTileRows]
    const unsigned long long *unit_offset;  // [n_chunks + 1]
    const uint32_t *tile_first;          // [n_chunks]
    uint32_t n_chunks;
    uint64_t n_units;
    uint32_t tol;
    int exclude_same;
    uint32_t n_slots, n_a, n_b;
    uint32_t *bitmap;
    uint32_t n_words;
    void *scratch;
    uint32_t **total_out;
};
hipError_t launch_align_seed_rates(const AlignSeedRatesLaunch &L, hipStream_t stream);
hipError_t launch_align_seed_rates_scatter(const AlignSeedRatesLaunch &L, vdf_video_pair_rate *out, uint32_t limit, hipStream_t stream);
// One chunk of a call over (rate, a, b) triples (align_rates_plan.h: AlignRatesChunk): the band walk of every (triple, phase,
// band) unit, the two-level reduction per triple, the dense list in (rate, a, b) order.  plan: the chunk's one upload (table | triples |
// unit_offset, align_rates_plan_bytes); a_first: n_rates x (n_a + 1); scratch holds align_rates_scratch_bytes(n_triples, n_units).  *dense_out /
// *total_out: where in scratch the records and their number are once the stream has run.
struct AlignRatesLaunch {
    const uint32_t *a_hashes, *a_first;
    const uint8_t *a_skip;               // nullable, per window
    const uint32_t *b_hashes, *b_first;
    const uint8_t *b_skip;
    const void *plan;
    uint32_t n_triples, n_units;
    uint32_t tol, min_run;
    void *scratch;
    vdf_alignment_rate **dense_out;
    uint32_t **total_out;
};
hipError_t launch_align_rates_chunk(const AlignRatesLaunch &L, hipStream_t stream);
// A masked round of such a chunk (align_rates_stretch_plan.h: AlignRatesRound): L as above on the round's triples, L.plan the round's
// upload with n_rects rectangles per triple behind unit_offset (align_rates_round_plan_bytes), n_rects in 1 ... kAlignMaxStretches - 1.  The same
// scratch and the same 32-byte records: the rank is the round's number.
hipError_t launch_align_rates_masked_chunk(const AlignRatesLaunch &L, uint32_t n_rects, hipStream_t stream);

}  // namespace vdf
