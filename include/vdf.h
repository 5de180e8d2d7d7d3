/*
 * vdf.h -- C ABI of the MI355X-native VideoHash construction + Hamming search engine.
 *
 * This is the drop-in boundary for the hot path of Farmadupe/vid_dup_finder_lib.  The
 * reference has no FFI layer of its own (it is one Rust crate); the entry points below are
 * what a `vdf-sys` binding would declare to replace the loops named next to each function.
 * The Rust-side stub is shown in INTEGRATION.md.  Citations are relative to the reference
 * repository root.
 *
 * Conventions
 *   - Plain pointers and sizes only.  No Rust, C++ or torch type crosses this boundary.
 *   - Return value: VDF_OK (0) or a negative vdf_status.  A human-readable message for the
 *     last failure on a context is available from vdf_last_error().
 *   - A hash is 16 x uint64_t = 1024 bits: bit i of the hash is bit (i & 63) of word (i >> 6)
 *     (bitvec Lsb0 over [usize;16], vid_dup_finder_lib/src/video_hashing/video_hash.rs:29,64-68).
 *   - "sorted order" means the order Search::sort leaves the entries in
 *     (src/video_hashing/search_algorithm.rs:55-61: stable by (duration, src_path)).  Sorting
 *     needs paths and stays on the caller's side; every index this library returns is an index
 *     into the arrays the caller passed.
 *   - Functions with the suffix _device take DEVICE pointers (HIP allocations on the
 *     context's GPU) and a hipStream_t passed as void* (NULL = the context's own non-blocking
 *     stream, NOT the legacy default stream) and need a single-device context; everything else
 *     takes host pointers (or, *_shards, one device pointer per GPU of a multi-GPU context).
 *     Stream order is all the ordering there is: work the caller queued on ANOTHER stream - a fill of the output buffer, the
 *     decoder's writes of the frames - is not waited for.  Pass the stream that work is on, or finish it first.
 *     Calls that only queue work share the context's scratch (the resized frames between the resize and the DCT stage, the work lists and
 *     counters of the letterbox and search kernels), and nothing orders two such calls on DIFFERENT streams of one context against each
 *     other: queue a context's _device calls on one stream, or finish one call before starting the next on another stream.
 *   - The search calls need their (candidate) arrays in sorted order and return VDF_E_INVAL when the
 *     durations are not ascending.
 *   - vdf_ctx_create() binds a context to one GPU.  vdf_ctx_create_multi() makes ONE context over several GPUs of
 *     the node (one host thread and one stream per device inside the library): the host-array calls
 *     (vdf_search_self, vdf_search_refs, vdf_hash_frames_u8[_letterbox]) then fan out by themselves, and the
 *     *_shards calls take data that is already resident on the devices.  See DESIGN.md "Multi-GPU".
 *   - Thread safety: a context serialises its own calls with an internal mutex, so
 *     vdf_hash_frames_u8 may be called from many threads (the app hashes from rayon workers,
 *     vid_dup_finder_app/src/video_hash_filesystem_cache/video_hash_filesystem_cache.rs:246).
 */
#ifndef VDF_H
#define VDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDF_DCT_SIZE 16    /* src/definitions.rs:34 */
#define VDF_HASH_SIZE 10   /* src/definitions.rs:36 */
#define VDF_HASH_BITS 1000 /* src/definitions.rs:42 */
#define VDF_HASH_WORDS 16  /* src/definitions.rs:43 */
#define VDF_DEFAULT_SEARCH_TOLERANCE 0.35 /* src/definitions.rs:5 */

typedef enum vdf_status {
    VDF_OK = 0,
    VDF_E_NOT_ENOUGH_FRAMES = -1, /* Error::NotEnoughFrames, src/video_hashing/mod.rs:27 */
    VDF_E_BAD_DIMS = -2,          /* the size asserts of dct_3d.rs:31-38 / Error::VidProc */
    VDF_E_HIP = -3,               /* HIP runtime failure or no usable GPU */
    VDF_E_OOM = -4,
    VDF_E_INVAL = -5,
    VDF_E_OVERFLOW = -6,          /* a caller-provided hit buffer was too small */
    VDF_E_RCCL = -7               /* librccl could not be loaded, or a collective failed (multi-GPU contexts only) */
} vdf_status;

typedef struct vdf_ctx vdf_ctx;

/* One thresholded pair.  Self-search: row = target index i, col = candidate index j > i.
 * Reference search: row = reference index (caller's order), col = candidate index. */
typedef struct vdf_hit {
    uint32_t row;
    uint32_t col;
} vdf_hit;

/* CSR result, the C form of Vec<MatchGroup> (src/video_hashing/matches/match_group.rs:10-13).
 * members[offsets[g] .. offsets[g+1]) are the duplicates of group g, already in the
 * reference's order.  ref_index[g] is the reference's position for search_with_references
 * and -1 for search().  Payload is library-allocated; release with vdf_groups_free(). */
typedef struct vdf_groups {
    uint64_t n_groups;
    uint64_t *offsets;  /* n_groups + 1 */
    uint64_t *members;  /* offsets[n_groups] */
    int64_t *ref_index; /* n_groups */
} vdf_groups;

/* Statistics of the last search on a context (for benchmarks and profiles). */
typedef struct vdf_search_stats {
    uint64_t pairs;         /* comparisons the reference's duration windows admit */
    uint64_t pairs_computed;/* pairs the tiles actually evaluated (>= pairs) */
    uint64_t n_hits;        /* thresholded pairs produced by the device */
    uint64_t n_tiles;       /* workgroups launched for the distance kernel */
    uint32_t n_launches;    /* distance-kernel launches (1 unless the hit buffer overflowed) */
    float kernel_ms;        /* HIP-event time of the distance kernel(s), on their stream */
    uint64_t pairs_early_exit; /* of pairs_computed: comparisons that stopped before the last bit because the partial distance
                                  of their whole block already exceeded the tolerance (exact; both backends) */
    uint32_t early_exit_bits;  /* bit positions counted before that test (0 = test disabled) */
    uint32_t reserved;
} vdf_search_stats;

/* Where the time of the last search call on a context went (benchmarks; accumulated over the launches of the call).
 * Device figures are HIP-event times on the kernels' own stream, host figures wall time. */
typedef struct vdf_search_timing {
    float prep_ms;      /* host wall: operand expansion + window / tile kernels, up to the launch of the distance kernel */
    float stream_ms;    /* device: the distance kernel proper */
    float resolve_ms;   /* device: exact evaluation of the queued suspect pairs (matrix-core backend; else 0) */
    float download_ms;  /* host wall: hit list into (row, col) order and into the caller's buffer */
    float replay_ms;    /* host wall: greedy replay / group assembly (host-level calls only) */
    float total_ms;     /* host wall of the whole call (host-level calls only) */
    uint64_t suspects;          /* suspect-queue entries written (matrix-core backend) */
    uint64_t suspect_capacity;  /* size of that queue in the last launch */
    uint64_t hits_filtered;     /* thresholded pairs dropped on the device because their row can never become a target of the
                                   greedy replay (host-level search() and the *_replay device call, sharded or not; they are counted in
                                   vdf_search_stats.n_hits) */
} vdf_search_timing;

/* ---- context ------------------------------------------------------------------------------ */
int vdf_ctx_create(int device_id, vdf_ctx **out);
/* One context over n_devices GPUs of this node: the single search() / search_with_references() call of the crate
 * (src/video_hashing/video_dup_finder.rs:7-13,19-46, called once per run from vid_dup_finder_app/src/app/app_fns.rs:
 * 478-482) then uses all of them.  Inside: one host thread + stream per device; the sorted database is replicated on every
 * device (from the caller's host arrays directly, or - *_shards calls - by an RCCL all-gather over xGMI), row tiles of the
 * triangle are dealt round-robin, the host merges the hits and replays the greedy grouping once, so the MatchGroups are
 * identical for every device count.  A device may be listed more than once (testing on one GPU): its slots then share
 * the GPU and the collective is replaced by device-to-device copies. */
int vdf_ctx_create_multi(const int *device_ids, int n_devices, vdf_ctx **out);
int vdf_ctx_device_count(const vdf_ctx *ctx);        /* 1 for vdf_ctx_create */
int vdf_ctx_device_at(const vdf_ctx *ctx, int slot); /* HIP device id of a slot, -1 if out of range */
/* Per-device statistics of the last search on a multi-GPU context (vdf_ctx_last_search_stats gives the sums, with
 * kernel_ms = the slowest device's). */
int vdf_ctx_device_search_stats(const vdf_ctx *ctx, int slot, vdf_search_stats *out);
int vdf_ctx_device_search_timing(const vdf_ctx *ctx, int slot, vdf_search_timing *out); /* that slot's phases and hits_filtered */
/* RCCL communicators (= ranks, one per GPU) the context has initialised so far: 0 until a *_shards call replicated through librccl
 * (a device list that repeats a GPU, or a single-device context, never does: plain device copies). */
int vdf_ctx_rccl_ranks(const vdf_ctx *ctx);
void vdf_ctx_destroy(vdf_ctx *ctx);
const char *vdf_last_error(const vdf_ctx *ctx); /* ctx may be NULL: last ctx_create failure */
const char *vdf_version(void);
int vdf_ctx_device(const vdf_ctx *ctx);
/* Hit-buffer capacity (entries) used by the host-level search calls; default 1<<24: 128 MB of DEVICE memory per GPU of the context
 * (8 bytes per entry).  The page-locked host staging the lists come down through is sized by what the searches actually produce
 * (512 KB to begin with), not by this capacity. */
int vdf_ctx_set_hit_capacity(vdf_ctx *ctx, uint64_t capacity);
int vdf_ctx_last_search_stats(const vdf_ctx *ctx, vdf_search_stats *out);
int vdf_ctx_last_search_timing(const vdf_ctx *ctx, vdf_search_timing *out); /* multi-GPU context: host figures + the slowest device's */
/* Diagnostics: bytes of device memory held by the library's growable buffers over all contexts of the process (tables, staging, hit
 * lists, crop descriptors ...).  Back to its earlier value after vdf_ctx_destroy, or a buffer was forgotten. */
long long vdf_live_device_bytes(void);
long long vdf_live_pinned_bytes(void); /* the same for page-locked host staging */

/* ---- host helpers (no GPU needed) ------------------------------------------------------------ */
/* VideoHash::hamming_distance, video_hash.rs:190-192,311-317: all 16 words, padding included. */
uint32_t vdf_hamming_u1024(const uint64_t *a, const uint64_t *b);
/* `(tolerance * TOLERANCE_SCALING_FACTOR) as u32`, search_algorithm.rs:64,82. */
uint32_t vdf_tolerance_int(double tolerance);
/* Sum over targets of the candidates inside the one-sided x1.1 window (search_algorithm.rs:99). */
uint64_t vdf_count_pairs_self(const uint32_t *sorted_durations, size_t n);
/* Sum over references of the +-5% window sizes (search_algorithm.rs:173-185). */
uint64_t vdf_count_pairs_refs(const uint32_t *sorted_cand_durations, size_t n_cand, const uint32_t *ref_durations,
                              size_t n_ref);
void vdf_groups_free(vdf_groups *g);

/* ---- hash construction: replaces VideoHash::from_frames, video_hash.rs:45-73 ----------------
 * (crop_resize_buf per frame, vid_dup_finder_common/src/resize_gray.rs:11-54; Dct3d::from_images
 * + dct_3d, dct_3d.rs:15-53 and raw_dct_ops.rs:107-142; hash_bits, dct_3d.rs:55-66; Lsb0 pack).
 * frames: n_clips clips of frames_per_clip gray u8 frames of w x h (row-major, tightly packed rows);
 * frame f of clip c starts at frames + c*clip_stride + f*frame_stride (bytes).  Only the first 16
 * frames of a clip are read.  frames_per_clip < 16 (or 0) -> VDF_E_NOT_ENOUGH_FRAMES.
 * out_hashes: n_clips x 16 words.  out_dontcare (nullable): per clip, the number of the 1000
 * coefficients with |coef| < 1e-6 (their sign is rounding noise; DESIGN.md "Parity rule"). */
int vdf_hash_frames_u8(vdf_ctx *ctx, const uint8_t *frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w,
                       uint32_t h, size_t frame_stride, size_t clip_stride, uint64_t *out_hashes,
                       uint32_t *out_dontcare);
int vdf_hash_frames_u8_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                              uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride, uint64_t *d_out_hashes,
                              uint32_t *d_out_dontcare, void *stream);

/* ---- letterbox crop detection + cropped hashing (the step right before from_frames) -------------
 * Replaces crop_video_frames with Cropdetect::Letterbox, the builder's default
 * (src/video_hashing/video_hash_builder.rs:188-212,59): cropdetect_letterbox
 * (vid_dup_finder_common/src/video_frames_gray.rs:201-210: frames 0 and 8, letterbox_crop with
 * AnyColour(16), :38-128, crops united by per-edge minimum, crop.rs:53-68), then every frame is
 * cropped and handed to from_frames.  Here the crop box is read in place: no cropped copies.
 * Crops are 4 x uint32 per clip: left, right, top, bottom edge offsets (crop.rs:3-10). */
int vdf_cropdetect_letterbox_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                                    uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride,
                                    uint32_t *d_crops /* DEVICE [n_clips][4] */, void *stream);
/* crops: HOST [n_clips][4] (NULL or all zero = no crop).  l + r >= w or t + b >= h -> VDF_E_INVAL. */
int vdf_hash_frames_u8_cropped_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                                      uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride,
                                      const uint32_t *crops, uint64_t *d_out_hashes, uint32_t *d_out_dontcare,
                                      void *stream);
/* detect + crop + hash in one call; out_crops (HOST, nullable) receives the detected boxes: they are there when the call returns (the
 * call then ends with a wait for its own work; pass NULL, or use the _async form below, to only queue). */
int vdf_hash_frames_u8_letterbox_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                                        uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride,
                                        uint64_t *d_out_hashes, uint32_t *d_out_dontcare, uint32_t *out_crops,
                                        void *stream);
/* The same with the boxes left on the DEVICE (d_out_crops: [n_clips][4], nullable), ordered on `stream` like the hashes.  For frames of
 * at most 256 columns and 128 rows the call only queues work: no copy to the host and no wait anywhere between detect and hash (frames of at
 * most 64 x 64: one kernel does both) - the reference's builder likewise detects, crops and hashes a clip in one pass
 * (video_hash_builder.rs:188-204).  Larger frames: the kernel per box shape is chosen on the host, so the call waits for the detect. */
int vdf_hash_frames_u8_letterbox_device_async(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                                              uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride,
                                              uint64_t *d_out_hashes, uint32_t *d_out_dontcare, uint32_t *d_out_crops,
                                              void *stream);
int vdf_hash_frames_u8_letterbox(vdf_ctx *ctx, const uint8_t *frames, size_t n_clips, uint32_t frames_per_clip,
                                 uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride, uint64_t *out_hashes,
                                 uint32_t *out_crops, uint32_t *out_dontcare);

/* ---- every 16-frame window of a clip: duplicates that are shifted in time ---------------------------
 * A copy with the intro trimmed, a clip cut out of a longer video, a re-upload that starts a few seconds later: the
 * hash of frames 0..15 does not see them.  These calls hash EVERY window of a clip - window k = frames
 * [k * window_stride, k * window_stride + 16), n_win = (frames_per_clip - 16) / window_stride + 1 of them
 * (vdf_hash_window_count) - and read, resize and spatially transform every frame ONCE: the 3-D DCT runs along y,
 * x, then t, and the y and x passes of a frame are the same in every window that holds it.
 * Word for word what vdf_hash_frames_u8_device gives on the same buffer with clip_stride = window_stride *
 * frame_stride, don't-care counts included.  ALL frames_per_clip frames of a clip are used; frame f of clip c at
 * frames + c*clip_stride + f*frame_stride, no byte outside [frames, end of the last clip's last frame) is read.
 * out_hashes: n_clips x n_win x 16 words, window k of clip c at 16 (c n_win + k); out_dontcare (nullable) at c n_win + k.
 * Errors, in this order: frames_per_clip < 16 -> VDF_E_NOT_ENOUGH_FRAMES; a zero dimension -> VDF_E_BAD_DIMS;
 * frame_stride < w*h -> VDF_E_INVAL; window_stride == 0 -> VDF_E_INVAL; n_clips * n_win >= 2^32 -> VDF_E_INVAL;
 * (n_clips == 0: VDF_OK, nothing is launched;) a null pointer -> VDF_E_INVAL; a multi-GPU context -> VDF_E_INVAL.
 * The host form uploads the frames in one piece and calls the device form (no pipelining over the link).
 * The _planes forms are these calls plus out_zero (required; n_clips x n_win x 16 words, window k of clip c at 16 (c n_win + k)): the ZERO PLANE
 * of every window, as the planes calls below define it - bit i set iff coefficient i == 0.0, bits 1000 ... 1023 are 0, H & Z == 0.  Same
 * checks in the same order (a null out_zero is among the null pointers), then an axis size whose resize table is not its own mirror image ->
 * VDF_E_BAD_DIMS, and a multi-GPU context last -> VDF_E_INVAL.  Same resize runs and routes; out_hashes and out_dontcare are bit-identical to
 * the plain calls'.  With the planes, vdf_window_variants_* and vdf_align_windows_variants* see flipped and reversed stretches.
 * Not here: zero planes of window hashes from the two plain calls (the _planes forms write them).  Videos of different frame sizes and
 * lengths, with crop boxes if they have any, in one call: vdf_hash_windows_clips_u8* below. */
size_t vdf_hash_window_count(uint32_t frames_per_clip, uint32_t window_stride); /* 0 if frames_per_clip < 16 or window_stride == 0 */
int vdf_hash_windows_u8(vdf_ctx *ctx, const uint8_t *frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w,
                        uint32_t h, size_t frame_stride, size_t clip_stride, uint32_t window_stride, uint64_t *out_hashes,
                        uint32_t *out_dontcare);
int vdf_hash_windows_u8_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                               uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride, uint32_t window_stride,
                               uint64_t *d_out_hashes, uint32_t *d_out_dontcare, void *stream);
int vdf_hash_windows_u8_planes(vdf_ctx *ctx, const uint8_t *frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w,
                               uint32_t h, size_t frame_stride, size_t clip_stride, uint32_t window_stride, uint64_t *out_hashes,
                               uint32_t *out_dontcare, uint64_t *out_zero);
int vdf_hash_windows_u8_planes_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                                      uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride, uint32_t window_stride,
                                      uint64_t *d_out_hashes, uint32_t *d_out_dontcare, uint64_t *d_out_zero, void *stream);

/* ---- retimed window hashes: a copy at another frame rate or speed ----------------------------------------------
 * The window calls above assume that two files hold the same frames, one for one.  A copy re-encoded from 30 to 25 fps keeps
 * 5 of every 6 frames, a 1.5x re-upload 2 of 3: its window k holds the frames of NO window of the original.  These calls hash
 * windows of the original that do hold them.  A rate is rate_num / rate_den with
 * 1 <= rate_den <= rate_num <= 2 rate_den and rate_num <= 65535, and
 *   tap(i) = floor(i * rate_num / rate_den), i = 0 ... 15;      span = tap(15) + 1 (16 ... 31);
 *   retimed window k = the hash of the 16 frames k * window_stride + tap(i) - exactly what vdf_hash_frames_u8 gives on those
 *   16 frames gathered into a stack, don't-care count included;
 *   n_win = (frames_per_clip - span) / window_stride + 1 (vdf_hash_window_count_retimed; 0 if frames_per_clip < span, if
 *   window_stride == 0 or if the rate is outside the range).
 * If B[j] = A[c + floor(j num / den)], the retimed window c + num m of A at num / den equals the plain window den m of B.
 * Always retime the side with MORE frames per second; rates below 1 would repeat frames and are not offered.
 * Arguments, layout of the outputs and the resize stage as vdf_hash_windows_u8[_device]; every frame is read, resized and
 * spatially transformed once.  Errors: that call's, in its order (frames_per_clip < 16 -> VDF_E_NOT_ENOUGH_FRAMES first), then
 * a rate outside the range or rate_den == 0 -> VDF_E_INVAL, then frames_per_clip < span -> VDF_E_NOT_ENOUGH_FRAMES.
 * At rate_num == rate_den, and at every rate whose taps are 0 ... 15 (25/24, say), the call IS the plain call: its route, its words.
 * The host form uploads in one piece and calls the device form's work.  A multi-GPU context -> VDF_E_INVAL.
 * Not here: zero planes of retimed windows, the batching queue.  A library of videos of different sizes and lengths in one call:
 * vdf_hash_windows_clips_u8_retimed[_device] below. */
size_t vdf_hash_window_count_retimed(uint32_t frames_per_clip, uint32_t window_stride, uint32_t rate_num, uint32_t rate_den);
int vdf_hash_windows_u8_retimed(vdf_ctx *ctx, const uint8_t *frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w,
                                uint32_t h, size_t frame_stride, size_t clip_stride, uint32_t window_stride, uint32_t rate_num,
                                uint32_t rate_den, uint64_t *out_hashes, uint32_t *out_dontcare);
int vdf_hash_windows_u8_retimed_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                                       uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride, uint32_t window_stride,
                                       uint32_t rate_num, uint32_t rate_den, uint64_t *d_out_hashes, uint32_t *d_out_dontcare,
                                       void *stream);

/* ---- retimed window hashes at several rates from one read of the frames ---------------------------------------------
 * Whoever looks for retimed copies does not know the rate: they try the usual ones - 1/1, 6/5, 5/4, 3/2, 2/1.  One
 * vdf_hash_windows_u8_retimed* call per rate reads, resizes and spatially transforms every frame once PER RATE, and only the pass along t
 * depends on the rate.  These calls take up to VDF_WINDOWS_MAX_RATES rates and do the rest once.  The job:
 *   frames ... window_stride   as vdf_hash_windows_u8[_device]'s arguments of those names; frames is a host pointer in
 *                              vdf_hash_windows_u8_rates and a device pointer in vdf_hash_windows_u8_rates_device;
 *   n_rates, rate_num, rate_den   1 ... 8 rates, each as vdf_hash_windows_u8_retimed takes it; HOST arrays in both forms.  Duplicate and
 *                              unreduced rates are legal, each listed rate gets its block.  1/1 gives the plain windows (the B side of
 *                              vdf_align_windows_retimed*) from the same pass;
 *   out_hashes, out_dontcare   RATE-MAJOR: with n_win_r = vdf_hash_window_count_retimed(frames_per_clip, window_stride, rate_num[r], rate_den[r])
 *                              and rate_first[r] = n_clips * (n_win_0 + ... + n_win_{r-1}), window k of clip c at rate r is row
 *                              rate_first[r] + c n_win_r + k: 16 words of out_hashes, one entry of out_dontcare (nullable).  Host pointers in
 *                              the host form, device pointers in the device form;
 *   stream                     device form only: the call is ordered on it, NULL = the context's stream.  (It travels in the job: the
 *                              job is the call's whole argument list.)
 * Block r is, word for word and count for count, what vdf_hash_windows_u8_retimed[_device] writes for rate r on the same frames.
 * vdf_hash_window_count_rates: host only; the total number of rows, rate_first (nullable, n_rates + 1 entries, the last one the total) filled
 * in; 0 rows if n_rates is outside 1 ... 8, a rate array is null, or any rate has no window (vdf_hash_window_count_retimed == 0).
 * Errors, in this order: a null ctx or job -> VDF_E_INVAL; those of vdf_hash_windows_u8 in its order; n_rates == 0, n_rates >
 * VDF_WINDOWS_MAX_RATES or a null rate array -> VDF_E_INVAL; the first rate outside the range -> VDF_E_INVAL; the first rate with
 * frames_per_clip < span -> VDF_E_NOT_ENOUGH_FRAMES (the message names the rate's index); 2^32 rows or more in all -> VDF_E_INVAL; a multi-GPU
 * context -> VDF_E_INVAL; n_clips == 0 -> VDF_OK, nothing is launched.
 * The host form uploads the frames ONCE, downloads all blocks and waits.  The device form only queues work; the rate arrays have left the
 * host when it returns.
 * Not here: zero planes, the batching queue, multi-GPU contexts.  Videos of different sizes and lengths at several rates in one call:
 * vdf_hash_windows_clips_u8_rates[_device] below. */
#define VDF_WINDOWS_MAX_RATES 8
typedef struct vdf_windows_rates_job {
    const uint8_t *frames;
    size_t n_clips;
    uint32_t frames_per_clip;
    uint32_t w;
    uint32_t h;
    size_t frame_stride;
    size_t clip_stride;
    uint32_t window_stride;
    uint32_t n_rates;
    const uint32_t *rate_num;
    const uint32_t *rate_den;
    uint64_t *out_hashes;
    uint32_t *out_dontcare;
    void *stream;
} vdf_windows_rates_job;
size_t vdf_hash_window_count_rates(size_t n_clips, uint32_t frames_per_clip, uint32_t window_stride, uint32_t n_rates,
                                   const uint32_t *rate_num, const uint32_t *rate_den, size_t *rate_first);
int vdf_hash_windows_u8_rates(vdf_ctx *ctx, const vdf_windows_rates_job *job);
int vdf_hash_windows_u8_rates_device(vdf_ctx *ctx, const vdf_windows_rates_job *job);

/* ---- align videos on their window hashes: the longest shared stretch of every pair of videos -------------
 * Which videos share a stretch, at what offset, and for how long.  Two sets of videos, A and B, each the
 * window hashes of its videos one after the other (what vdf_hash_windows_* writes): hashes[n_windows_total][16] and
 * first[n_videos + 1], video v owning the windows first[v] ... first[v + 1].  Videos may differ in window count; a video of
 * 0 windows is legal and pairs with nothing.  For videos a, b with Na, Nb windows:
 *   - a CELL (ka, kb) matches iff neither window is skipped and vdf_hamming_u1024(A[a][ka], B[b][kb]) <= tol
 *     (tol = min(tol_int, 1024), as the searches clamp it);
 *   - a RUN is a maximal stretch of consecutive matching cells on one diagonal offset = kb - ka: (offset, start_a,
 *     n_windows, dist_sum); only runs of n_windows >= min_run compete;
 *   - the best run of the pair maximises score = n_windows * (tol + 1) - dist_sum: every matching cell adds at least 1, so a
 *     maximal run beats its sub-runs, and a true copy at distance ~0 beats the same stretch seen one diagonal off at a
 *     larger distance, even where that one is a window longer.  Ties: the smaller signed offset, then the smaller start_a;
 *   - a pair without a competing run produces nothing: at most ONE record per pair, however dense the matches are.
 * b_hashes == NULL is SELF mode: B = A (b_first, n_b, b_skip are ignored) and only the pairs a < b are evaluated; a video is
 * never aligned with itself.  skip (nullable, one byte per window, non-zero = this window abstains) lets static stretches
 * stay out: their windows are all alike and match everything static.
 * out: HOST buffer of `capacity` records, filled in (a, b) order.  *n_out = the number of records found; if it exceeds
 * capacity the first `capacity` entries of out are valid (the first in (a, b) order) and the caller calls again with a larger
 * buffer - VDF_OK, like the hit buffers.
 * Errors, in this order, all VDF_E_INVAL: a null required pointer (out may be NULL when capacity is 0); min_run == 0; a
 * video of more than 2^20 windows (keeps the score below 2^31); a first array that is not non-decreasing (the device
 * form reads the first arrays back to plan the launch and checks them too; that they fit the hash arrays is the caller's
 * contract); more than 2^24 pairs of videos in one call (the mirrors split); a multi-GPU context.
 * n_a == 0, n_b == 0 or self mode with one video: VDF_OK, *n_out = 0, nothing is launched.
 * vdf_align_windows_device: the array pointers are DEVICE pointers (hashes 16-byte aligned), out is on the host; the call
 * waits for its own work.  vdf_align_windows: host arrays; uploads them and calls the device form.
 * vdf_align_windows_host: no context, no GPU - the definition above in plain C++ (every diagonal walked, XOR + popcount):
 * the CPU-tested statement of the semantics, for tiny inputs and tests.
 * ONE stretch per pair here - a video that holds two separate excerpts of another reports the better one; every shared stretch of a
 * pair: vdf_align_windows_stretches* below.
 * Flipped and reversed stretches: vdf_align_windows_variants* below.  Not here: multi-GPU contexts. */
typedef struct vdf_alignment { /* 24 bytes */
    uint32_t a;                /* video index in A */
    uint32_t b;                /* video index in B (self mode: in A, a < b) */
    int32_t offset;            /* kb - ka, in windows */
    uint32_t start_a;          /* ka of the run's first window */
    uint32_t n_windows;
    uint32_t dist_sum;         /* sum of the run's distances */
} vdf_alignment;
int vdf_align_windows_host(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                           const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                           uint32_t tol_int, uint32_t min_run, vdf_alignment *out, size_t capacity, size_t *n_out);
int vdf_align_windows(vdf_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                      const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                      uint32_t tol_int, uint32_t min_run, vdf_alignment *out, size_t capacity, size_t *n_out);
int vdf_align_windows_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a,
                             const uint8_t *d_a_skip, const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b,
                             const uint8_t *d_b_skip, uint32_t tol_int, uint32_t min_run, vdf_alignment *out,
                             size_t capacity, size_t *n_out, void *stream);

/* ---- EVERY shared stretch of a pair, not only the best one -------------------------------------------------
 * An ad break cut out of a re-upload leaves two stretches at two offsets; a compilation that uses a source twice, or a loop, repeats one.
 * The definition is vdf_align_windows' word for word - cell rule, run, score, ties, min_run, skip bytes, the tol clamp, self mode, 2^20
 * windows per video, 2^24 pairs per call - and then, for one pair (a, b) of Na x Nb windows:
 *   - RANK 0 is the record vdf_align_windows reports;
 *   - after a stretch (offset, start_a, n) is reported, with start_b = start_a + offset, its RECTANGLE
 *       [max(0, start_a - guard), min(Na, start_a + n + guard)) x [max(0, start_b - guard), min(Nb, start_b + n + guard))
 *     (bounds in 64-bit arithmetic: nothing wraps) becomes misses for all later ranks.  A cell is masked only if ka lies in the A range AND
 *     kb in the B range of the SAME rectangle: the same rows of A matched against another part of B stay visible, so a source used twice in
 *     a compilation gives two records;
 *   - a masked cell ends a run exactly as a non-matching cell does: a diagonal that crosses a rectangle yields separate runs before and
 *     after it, each of which competes only if it has min_run windows of its own;
 *   - RANK r is the best run of the matrix masked by the rectangles of ranks 0 ... r - 1;
 *   - a pair stops at the first rank without a competing run, or after max_stretches ranks.
 * max_stretches: 1 ... 8.  guard: 0 ... 2^20 windows; it widens the rectangles so that the neighbouring diagonals of slowly changing content
 * - windows one frame apart share 15 of their 16 frames - are not reported as stretches of their own.
 * out: HOST buffer of `capacity` records ordered by (a, b, rank).  *n_out = the number found; if it exceeds capacity the first `capacity`
 * records in that order are valid - VDF_OK, as the align calls.  With max_stretches == 1 the records are vdf_align_windows' field for
 * field, with rank 0.
 * Errors: those of vdf_align_windows in their order; then max_stretches outside 1 ... 8; then guard above 2^20; then a multi-GPU context -
 * all VDF_E_INVAL.
 * vdf_align_windows_stretches_host: no context, no GPU - the definition above in plain C++, the CPU-tested statement of the semantics.
 * vdf_align_windows_stretches: host arrays, uploaded as vdf_align_windows uploads them.  vdf_align_windows_stretches_device: DEVICE
 * pointers, out on the host; the call waits for its own work.
 * Not offered: more than one stretch per pair against the flipped variants (vdf_align_windows_variants* stays one per pair). */
typedef struct vdf_alignment_stretch { /* 28 bytes */
    uint32_t a;                /* the six fields of vdf_alignment */
    uint32_t b;
    int32_t offset;
    uint32_t start_a;
    uint32_t n_windows;
    uint32_t dist_sum;
    uint32_t rank;             /* 0 ... max_stretches - 1: 0 is the pair's best stretch */
} vdf_alignment_stretch;
int vdf_align_windows_stretches_host(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                     const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                                     uint32_t tol_int, uint32_t min_run, uint32_t max_stretches, uint32_t guard,
                                     vdf_alignment_stretch *out, size_t capacity, size_t *n_out);
int vdf_align_windows_stretches(vdf_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                                uint32_t tol_int, uint32_t min_run, uint32_t max_stretches, uint32_t guard,
                                vdf_alignment_stretch *out, size_t capacity, size_t *n_out);
int vdf_align_windows_stretches_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a,
                                       const uint8_t *d_a_skip, const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b,
                                       const uint8_t *d_b_skip, uint32_t tol_int, uint32_t min_run, uint32_t max_stretches,
                                       uint32_t guard, vdf_alignment_stretch *out, size_t capacity, size_t *n_out, void *stream);

/* ---- a library is not walked pair by pair: seed the candidate pairs, align only those ------------------------
 * The align calls above walk every cell of every pair of videos, also where no pair shares anything.  An exact filter: a run that competes
 * has at least min_run consecutive matching cells on one diagonal, and any min_run consecutive values of ka contain a multiple of min_run.
 * So a pair (a, b) can have a record only if some cell (ka, kb) matches with ka % min_run == 0.
 * Inputs: those of vdf_align_windows - hashes, first arrays, nullable skip bytes, tol = min(tol_int, 1024), min_run >= 1, self mode when
 * b_hashes == NULL.
 *   - a SEED is window ka of video a with ka % min_run == 0; ka counts from the video's own first window, not from the array's;
 *   - pair (a, b) is a CANDIDATE iff some seed of a and some window kb of b form a matching cell under the align rule: neither window is
 *     skipped and the distance over all 16 words is <= tol.  In self mode the pair must also have a < b.
 * The candidates are a set, exact and deterministic.  It holds every pair for which vdf_align_windows has a record; it may hold pairs that
 * have none (an isolated matching cell).  With min_run == 1 every window is a seed.
 * vdf_align_seed_pairs*: out is a HOST buffer of `capacity` pairs, filled in (a, b) order, under the capacity protocol of the align calls
 * (*n_out = the number found; the first `capacity` are valid).  Errors: those of vdf_align_windows, in their order - the limit of 2^24 pairs
 * of videos included (it sizes the bitmap the pairs are marked in) and a multi-GPU context last.
 * vdf_align_windows_pairs*: vdf_align_windows restricted to a caller-given HOST list of n_pairs pairs (also in the device form): the records
 * are those the all-pairs call reports for the listed pairs, field for field, in (a, b) order.  The list must be strictly increasing in
 * (a, b), with a < n_a and b < n_b, and a < b in self mode (b < n_a there).  Errors, in this order, all VDF_E_INVAL: a null list with
 * n_pairs > 0; those of vdf_align_windows up to the first arrays; n_a or n_b above 2^32 - 1 (a video index does not fit 32 bits: n_a x n_b
 * may be anything below that); more than 2^24 LISTED pairs; a list that is not strictly increasing; a pair that names a video that does not exist; a pair with a >= b in self mode;
 * a multi-GPU context.  (The device form reads the first arrays back and checks them after the list, as vdf_align_windows_device does
 * after its own checks.)
 * vdf_align_windows_stretches_pairs*: the same restriction for vdf_align_windows_stretches; max_stretches and guard are checked behind the
 * align checks, as there, and before the list.
 * Each in the usual three forms: _host (plain C++, no context: the CPU-tested statement of the semantics), host arrays through a context,
 * _device (DEVICE arrays and a stream; the call waits for its own work).
 * A skip byte is read with the aligned 32-bit word that holds it (the seed kernel reads a seed's byte by a scalar load, as the band kernels of
 * vdf_align_windows read a row's): for a skip array that does not begin or end on a 4-byte boundary up to 3 bytes beside it are read - inside
 * the same word, so inside the same page and, with any device allocator, the same allocation - and their values are ignored.
 * The variants on a list and seeded: vdf_align_windows_variants_pairs* and vdf_align_seed_pairs_variants* below. */
typedef struct vdf_video_pair { /* 8 bytes */
    uint32_t a;                /* video index in A */
    uint32_t b;                /* video index in B (self mode: in A, a < b) */
} vdf_video_pair;
int vdf_align_seed_pairs_host(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                              const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                              uint32_t tol_int, uint32_t min_run, vdf_video_pair *out, size_t capacity, size_t *n_out);
int vdf_align_seed_pairs(vdf_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                         const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                         uint32_t tol_int, uint32_t min_run, vdf_video_pair *out, size_t capacity, size_t *n_out);
int vdf_align_seed_pairs_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a,
                                const uint8_t *d_a_skip, const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b,
                                const uint8_t *d_b_skip, uint32_t tol_int, uint32_t min_run, vdf_video_pair *out,
                                size_t capacity, size_t *n_out, void *stream);
int vdf_align_windows_pairs_host(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                 const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                                 const vdf_video_pair *pairs, size_t n_pairs, uint32_t tol_int, uint32_t min_run,
                                 vdf_alignment *out, size_t capacity, size_t *n_out);
int vdf_align_windows_pairs(vdf_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                            const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                            const vdf_video_pair *pairs, size_t n_pairs, uint32_t tol_int, uint32_t min_run,
                            vdf_alignment *out, size_t capacity, size_t *n_out);
int vdf_align_windows_pairs_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a,
                                   const uint8_t *d_a_skip, const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b,
                                   const uint8_t *d_b_skip, const vdf_video_pair *pairs, size_t n_pairs, uint32_t tol_int,
                                   uint32_t min_run, vdf_alignment *out, size_t capacity, size_t *n_out, void *stream);
int vdf_align_windows_stretches_pairs_host(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                           const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                                           const vdf_video_pair *pairs, size_t n_pairs, uint32_t tol_int, uint32_t min_run,
                                           uint32_t max_stretches, uint32_t guard, vdf_alignment_stretch *out, size_t capacity,
                                           size_t *n_out);
int vdf_align_windows_stretches_pairs(vdf_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a,
                                      const uint8_t *a_skip, const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b,
                                      const uint8_t *b_skip, const vdf_video_pair *pairs, size_t n_pairs, uint32_t tol_int,
                                      uint32_t min_run, uint32_t max_stretches, uint32_t guard, vdf_alignment_stretch *out,
                                      size_t capacity, size_t *n_out);
int vdf_align_windows_stretches_pairs_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a,
                                             const uint8_t *d_a_skip, const uint64_t *d_b_hashes, const uint32_t *d_b_first,
                                             size_t n_b, const uint8_t *d_b_skip, const vdf_video_pair *pairs, size_t n_pairs,
                                             uint32_t tol_int, uint32_t min_run, uint32_t max_stretches, uint32_t guard,
                                             vdf_alignment_stretch *out, size_t capacity, size_t *n_out, void *stream);

/* ---- align RETIMED windows: a copy at another frame rate or speed, every phase in one call ---------------------
 * Which of these videos is a 30 -> 25 fps or 1.5 x copy of which, and where.  A holds RETIMED windows at stride 1 (what
 * vdf_hash_windows_u8_retimed* writes at rate_num / rate_den), B plain windows at stride 1; arrays as vdf_align_windows takes them: hashes,
 * first[n + 1], nullable skip bytes.  The rate is rate_num / rate_den with 1 <= rate_den <= rate_num <= 2 rate_den; the call reduces it by its
 * gcd to num / den, and num <= VDF_ALIGN_RETIMED_MAX_NUM after that (above it the sub-matrices below degenerate).  If B[j] = A[c + (j num) / den],
 * retimed window c + num m of A equals plain window den m of B: the matching cells lie on a line of slope num / den, which
 * vdf_align_windows does not follow.  So for a pair (a, b) of Na x Nb windows and every PHASE p = 0 ... num - 1:
 *   - the SUB-MATRIX of phase p has the cells (i, j) = (row p + num i of a, row den j of b) for i < ceil((Na - p) / num) - none if p >= Na -
 *     and j < ceil(Nb / den);
 *   - a cell matches iff both skip bytes - read at those same rows - are 0 and the distance is <= tol = min(tol_int, 1024);
 *   - runs, min_run, score and ties INSIDE a phase are vdf_align_windows' rule on the sub-matrix, word for word: a run is a maximal stretch
 *     of matching cells on one diagonal offset = j - i, min_run counts sub-sampled windows, score = n (tol + 1) - dist_sum, ties go to the
 *     smaller offset, then the smaller i0: the PHASE-BEST;
 *   - ACROSS the phases the pair keeps the phase-best with the largest score; on a tie the smaller first_a = p + num i0, then the smaller
 *     first_b = den (i0 + offset).  Two levels, each with its own tie rule: one comparator over all runs of all phases gives other records.
 * At most ONE record per pair, in (a, b) order, under the capacity protocol of vdf_align_windows (*n_out is always the number found, the
 * first `capacity` records are valid).  There is NO self mode: A and B are different hash sets even for one library (b_hashes == NULL with
 * n_b > 0 is a null pointer); a library against itself is the _pairs form with the list a != b.  At rate 1 / 1 the records are
 * vdf_align_windows' with first_a = start_a, first_b = start_a + offset.
 * Errors, all VDF_E_INVAL: those of vdf_align_windows in their order (2^20 windows per video and 2^24 pairs per call included); then a rate
 * outside 1 <= den <= num <= 2 den; then a reduced num above VDF_ALIGN_RETIMED_MAX_NUM; then a multi-GPU context.  The _pairs forms: a
 * caller-given HOST list as vdf_align_windows_pairs* takes it (strictly increasing in (a, b), a < n_a, b < n_b), checked as there, the rate
 * behind the align checks and before the list.  Each in the usual three forms: _host (plain C++, no context, no GPU: the CPU-tested
 * statement of the semantics), host arrays through a context (uploaded as vdf_align_windows uploads them), _device (DEVICE arrays, out
 * on the host; the call waits for its own work).  Skip bytes are read as the other align calls read them (the aligned 32-bit word).
 * Not offered: window starts of B that are not multiples of den; flips; rates above 2.  Several stretches per pair:
 * vdf_align_windows_rates_stretches* below (a one-rate list is this call's pair). */
#define VDF_ALIGN_RETIMED_MAX_NUM 32
typedef struct vdf_alignment_retimed { /* 24 bytes */
    uint32_t a;                /* video index in A */
    uint32_t b;                /* video index in B */
    uint32_t first_a;          /* the run's first (retimed) window of a: p + num i0 */
    uint32_t first_b;          /* the run's first window of b: den (i0 + offset); the run's m-th cell is (first_a + num m, first_b + den m) */
    uint32_t n_windows;        /* sub-sampled windows in the run */
    uint32_t dist_sum;         /* sum of the run's distances */
} vdf_alignment_retimed;
int vdf_align_windows_retimed_host(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                   const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                                   uint32_t tol_int, uint32_t min_run, uint32_t rate_num, uint32_t rate_den,
                                   vdf_alignment_retimed *out, size_t capacity, size_t *n_out);
int vdf_align_windows_retimed(vdf_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                              const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                              uint32_t tol_int, uint32_t min_run, uint32_t rate_num, uint32_t rate_den,
                              vdf_alignment_retimed *out, size_t capacity, size_t *n_out);
int vdf_align_windows_retimed_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a,
                                     const uint8_t *d_a_skip, const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b,
                                     const uint8_t *d_b_skip, uint32_t tol_int, uint32_t min_run, uint32_t rate_num,
                                     uint32_t rate_den, vdf_alignment_retimed *out, size_t capacity, size_t *n_out, void *stream);
int vdf_align_windows_retimed_pairs_host(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                         const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                                         const vdf_video_pair *pairs, size_t n_pairs, uint32_t tol_int, uint32_t min_run,
                                         uint32_t rate_num, uint32_t rate_den, vdf_alignment_retimed *out, size_t capacity,
                                         size_t *n_out);
int vdf_align_windows_retimed_pairs(vdf_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                    const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                                    const vdf_video_pair *pairs, size_t n_pairs, uint32_t tol_int, uint32_t min_run,
                                    uint32_t rate_num, uint32_t rate_den, vdf_alignment_retimed *out, size_t capacity,
                                    size_t *n_out);
int vdf_align_windows_retimed_pairs_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a,
                                           const uint8_t *d_a_skip, const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b,
                                           const uint8_t *d_b_skip, const vdf_video_pair *pairs, size_t n_pairs, uint32_t tol_int,
                                           uint32_t min_run, uint32_t rate_num, uint32_t rate_den, vdf_alignment_retimed *out,
                                           size_t capacity, size_t *n_out, void *stream);

/* ---- the retimed alignment, seeded: the candidates of every phase of up to VDF_WINDOWS_MAX_RATES rates from one pass ----
 * Which pairs (a, b) can have a record of vdf_align_windows_retimed* at which rate of a list?  A is what vdf_hash_windows_clips_u8_rates*
 * writes - one block of retimed windows per listed rate, rate-major - B holds plain windows at stride 1 (the 1/1 block of such a call).
 * Rate r of the list is reduced by its gcd to num / den.  Counted inside their videos,
 *   - a SEED under r is window ka of video a of block r with (ka / num) % min_run == 0 (integer division): sub-sampled index i = ka / num of
 *     phase p = ka % num, with i a multiple of min_run;
 *   - a ROW under r is window kb of video b with kb % den == 0;
 *   - pair (a, b) is a CANDIDATE UNDER r iff some seed and some row have both skip bytes 0 and a distance over all 16 words <= tol =
 *     min(tol_int, 1024); with exclude_same != 0 (requires n_a == n_b: a library against itself) a pair with a == b is never a candidate.
 * A run of >= min_run cells on a diagonal of a phase's sub-matrix holds an i that is a multiple of min_run, so the set holds every pair with a
 * record of vdf_align_windows_retimed* at r; it is the union over p < num of vdf_align_seed_pairs' set on (windows p, p + num, ... of A's videos;
 * windows 0, den, ... of B's).  At 1/1 it is vdf_align_seed_pairs' set between the two sets.  There is no self mode (b_hashes == NULL with
 * n_b > 0 is a null pointer).  Duplicate and unreduced rates are legal, each listed rate gets its slot.
 * The job - the call's whole argument list, as vdf_windows_clips_rates_job is:
 *   a_hashes, a_skip (nullable)   the rows of A; a_first: n_rates x (n_a + 1) entries, row r at a_first + r (n_a + 1); a_rate_first: HOST array of
 *                              n_rates + 1 size_t (only the first n_rates are read), nullable = zeros - what vdf_hash_windows_clips_first_rates
 *                              fills.  Window k of video i at rate r is row a_rate_first[r] + a_first[r][i] + k of a_hashes and a_skip: a hash
 *                              call's outputs go in unchanged.  Fewer than 2^32 rows in all;
 *   b_hashes, b_first, b_skip, n_b   as vdf_align_seed_pairs takes them;
 *   n_rates, rate_num, rate_den   1 ... VDF_WINDOWS_MAX_RATES rates, HOST arrays in all forms;
 *   tol_int, min_run, exclude_same;
 *   out, capacity, n_out       HOST buffer of `capacity` vdf_video_pair_rate triples in (rate, a, b) order - rate is the index into the job's
 *                              list; *n_out = the number found over all rates, the first `capacity` are valid if it exceeds capacity - VDF_OK;
 *   stream                     device form only: the call is ordered on it, NULL = the context's stream.
 * Errors, all VDF_E_INVAL, in this order: a null job or ctx; the checks of vdf_align_seed_pairs in its order of KINDS - null pointers (n_out; out
 * with capacity > 0; hashes or first array of a side that has videos), min_run == 0, a video above 2^20 windows, a first array that decreases,
 * 2^32 rows of A or more, more than 2^24 pairs of videos - each kind on B first and then on the blocks of A in list order (the blocks of the first
 * min(n_rates, VDF_WINDOWS_MAX_RATES) rates); n_rates outside 1 ... VDF_WINDOWS_MAX_RATES or a null rate array; the first rate outside
 * 1 <= den <= num <= 2 den; the first rate with a reduced num above VDF_ALIGN_RETIMED_MAX_NUM; exclude_same with n_a != n_b; a multi-GPU context.
 * n_a == 0 or n_b == 0: VDF_OK with *n_out = 0.  The device form makes every check that needs no first array, in that order, reads the first
 * arrays back, and checks them.
 * _host: plain C++, no context, no GPU - the CPU-tested statement of the semantics.  vdf_align_seed_pairs_rates: host arrays, uploaded once.
 * _device: DEVICE arrays (hashes, first arrays, skip bytes); the rate arrays, a_rate_first and out stay on the host; the call waits for its own
 * work.  The context forms make ONE pass: rates that share a den share their gathered rows of B, and the seeds of every phase of every rate
 * stream past them in one launch.  Skip bytes of A are read as the other seed calls read them (the aligned 32-bit word).
 * Not offered: zero planes; multi-GPU contexts.  The align call over the triples is vdf_align_windows_rates*, below. */
typedef struct vdf_video_pair_rate { /* 12 bytes */
    uint32_t a;                /* video index in A */
    uint32_t b;                /* video index in B */
    uint32_t rate;             /* index into the job's rate list */
} vdf_video_pair_rate;
typedef struct vdf_align_seed_rates_job {
    const uint64_t *a_hashes;
    const uint32_t *a_first;
    const size_t *a_rate_first;
    const uint8_t *a_skip;
    size_t n_a;
    const uint64_t *b_hashes;
    const uint32_t *b_first;
    const uint8_t *b_skip;
    size_t n_b;
    uint32_t n_rates;
    const uint32_t *rate_num;
    const uint32_t *rate_den;
    uint32_t tol_int;
    uint32_t min_run;
    uint32_t exclude_same;
    vdf_video_pair_rate *out;
    size_t capacity;
    size_t *n_out;
    void *stream;
} vdf_align_seed_rates_job;
int vdf_align_seed_pairs_rates_host(const vdf_align_seed_rates_job *job);
int vdf_align_seed_pairs_rates(vdf_ctx *ctx, const vdf_align_seed_rates_job *job);
int vdf_align_seed_pairs_rates_device(vdf_ctx *ctx, const vdf_align_seed_rates_job *job);

/* ---- align retimed windows at up to VDF_WINDOWS_MAX_RATES rates in ONE call: (rate, a, b) triples ----------------------------
 * The third step of the retimed pipeline - hash (vdf_hash_windows_clips_u8_rates*), seed (vdf_align_seed_pairs_rates*), align - with the rate list
 * in one call, as the first two take it.  A and B are what the seed call takes, unchanged: A rate-major with a_first (n_rates x (n_a + 1)) and the
 * HOST array a_rate_first (nullable = zeros), window k of video i at rate r in row a_rate_first[r] + a_first[r][i] + k; B plain windows.
 * The record of a triple (r, a, b) is, field for field, the record vdf_align_windows_retimed_pairs* gives for the pair (a, b) on block r at
 * rate_num[r] / rate_den[r] - the sub-matrices, the two-level reduction and its tie rules are that call's - with rate = r and
 * n_frames_b = (n_windows - 1) den + 16 (den in lowest terms) added; where that call gives no record, this one gives none.  Records come in
 * (rate, a, b) order under the capacity protocol of the align calls (*n_out is always the number found, the first `capacity` are valid).
 * Duplicate and unreduced rates are legal, each listed rate gets its slot; tol = min(tol_int, 1024).  Which triples are walked:
 *   triples != NULL            exactly the listed ones: a HOST array in all forms, strictly increasing in (rate, a, b), rate < n_rates, a < n_a,
 *                              b < n_b; seed and exclude_same must be 0.  What vdf_align_seed_pairs_rates* wrote goes in unchanged;
 *   triples == NULL, seed == 0 every (r, a, b); with exclude_same != 0 (requires n_a == n_b) without those with a == b;
 *   triples == NULL, seed != 0 the candidate set of vdf_align_seed_pairs_rates* on the same arguments, found inside the call.  That set holds
 *                              every pair that has a record, so the output equals the seed == 0 output, record for record.
 * Limits: n_a x n_b <= 2^24, n_triples <= 2^27, 2^20 windows per video, fewer than 2^32 rows of A.
 * Errors, all VDF_E_INVAL, in this order: a null job or ctx; the checks of vdf_align_seed_pairs_rates in its order, up to and including the rate
 * list, each kind on B first and then on the blocks of A; exclude_same with n_a != n_b; a list together with seed or exclude_same; the list
 * (more than 2^27 entries, then the first bad entry: not strictly increasing, a rate outside the list, a video that does not exist); a
 * multi-GPU context.  n_a == 0, n_b == 0 or an empty list: VDF_OK with *n_out = 0.
 * _host: plain C++, no context, no GPU - vdf_align_windows_retimed_pairs_host's definition triple by triple, behind
 * vdf_align_seed_pairs_rates_host where seed != 0.  vdf_align_windows_rates: host arrays, uploaded ONCE for both the seed pass and the walk.
 * _device: DEVICE hashes, first arrays and skip bytes; the rate arrays, a_rate_first, triples and out stay on the host; the first arrays are read
 * back as the seed call reads them; the call is ordered on `stream` (NULL = the context's) and waits for its own work.  In the context forms a
 * chunk of units may span rates: the triples of all rates are one launch set.
 * Not offered: the candidates handed to the band kernels on the device (the triples visit the host for planning); flips per triple; a C
 * best_rates; multi-GPU contexts.  Several stretches per triple: vdf_align_windows_rates_stretches*, below. */
typedef struct vdf_alignment_rate { /* 32 bytes */
    uint32_t a;                /* video index in A */
    uint32_t b;                /* video index in B */
    uint32_t rate;             /* index into the job's rate list */
    uint32_t first_a;          /* p + num i0, counted inside video a of block `rate` */
    uint32_t first_b;          /* den (i0 + offset) */
    uint32_t n_windows;        /* sub-sampled windows in the run */
    uint32_t dist_sum;         /* sum of the run's distances */
    uint32_t n_frames_b;       /* (n_windows - 1) den + 16: the frames of b the run covers, comparable across rates */
} vdf_alignment_rate;
typedef struct vdf_align_rates_job {
    const uint64_t *a_hashes;
    const uint32_t *a_first;
    const size_t *a_rate_first;
    const uint8_t *a_skip;
    size_t n_a;
    const uint64_t *b_hashes;
    const uint32_t *b_first;
    const uint8_t *b_skip;
    size_t n_b;
    uint32_t n_rates;
    const uint32_t *rate_num;
    const uint32_t *rate_den;
    uint32_t tol_int;
    uint32_t min_run;
    const vdf_video_pair_rate *triples;
    size_t n_triples;
    uint32_t seed;
    uint32_t exclude_same;
    vdf_alignment_rate *out;
    size_t capacity;
    size_t *n_out;
    void *stream;
} vdf_align_rates_job;
int vdf_align_windows_rates_host(const vdf_align_rates_job *job);
int vdf_align_windows_rates(vdf_ctx *ctx, const vdf_align_rates_job *job);
int vdf_align_windows_rates_device(vdf_ctx *ctx, const vdf_align_rates_job *job);

/* ---- EVERY stretch of a retimed pair, ranked, at up to VDF_WINDOWS_MAX_RATES rates in one call ---------------------------------
 * A re-upload that was converted to another frame rate or sped up is usually edited as well: an ad break cut out (two stretches at two lines
 * first_b - first_a den / num), a scene replaced (two runs on one line), a source used twice.  vdf_align_windows_rates* reports one record per
 * triple; these calls report up to max_stretches, ranked - vdf_align_windows_stretches* for (rate, a, b) triples.  The inputs are exactly those of
 * vdf_align_windows_rates*: A rate-major with a_first (n_rates x (n_a + 1)) and the HOST array a_rate_first, B plain windows at stride 1, the rate
 * list, tol_int, min_run, and the three triple modes (a HOST list; every triple, with or without exclude_same; seed != 0).
 * For one triple (r, a, b), rate r reduced to num / den, Na rows of a in block r, Nb rows of b:
 *   - RANK 0 is the record vdf_align_windows_rates* reports for the triple, field for field;
 *   - after a stretch (first_a, first_b, n) is reported, its RECTANGLE counts as non-matching for all later ranks of this triple.  It is kept in
 *     the ROWS OF THE TWO VIDEOS, not in a phase's sub-matrix: rows [max(0, first_a - ga), min(Na, first_a + num (n - 1) + 1 + ga)) of a with
 *     ga = ceil(guard num / den), rows [max(0, first_b - guard), min(Nb, first_b + den (n - 1) + 1 + guard)) of b; bounds in 64-bit arithmetic;
 *   - cell (i, j) of the sub-matrix of ANY phase p is masked iff row p + num i lies in the rows of a AND row den j in the rows of b of the same
 *     rectangle.  The rectangle masks all phases: otherwise rank 1 would be the same stretch seen from the neighbouring phase.  The same rows
 *     of a against another part of b stay visible;
 *   - a masked cell ends a run exactly as a non-matching cell does;
 *   - RANK k is vdf_align_windows_retimed*'s record on the matrix masked by the rectangles of ranks 0 ... k - 1: the phase-bests by the align
 *     rule, then the two-level reduction with its tie rules;
 *   - a triple stops at the first rank without a record, or after max_stretches ranks.
 * max_stretches: 1 ... 8.  guard: 0 ... 2^20, counted in rows of B - B holds plain windows at stride 1, so frames of b.
 * At rate 1/1 the rectangle is vdf_align_windows_stretches'; a one-rate list at 1/1 gives vdf_align_windows_stretches_pairs*' records with
 * first_a = start_a, first_b = start_a + offset.  seed != 0 seeds ONCE, in front of rank 0: a triple without a rank-0 record has no later rank,
 * so the candidate set is still exact and the output equals the seed == 0 output record for record.
 * The job: the fields of vdf_align_rates_job with their meaning, max_stretches and guard, and out of the record type below.  Records come in
 * (rate, a, b, rank) order under the capacity protocol of the align calls (*n_out is always the number found, the first `capacity` are valid).
 * With max_stretches == 1 the records are vdf_align_windows_rates*', with rank 0.
 * Errors, all VDF_E_INVAL, in this order: those of vdf_align_windows_rates* in their order, up to and including the list; max_stretches outside
 * 1 ... 8; guard above 2^20; a multi-GPU context.  n_a == 0, n_b == 0 or an empty list: VDF_OK with *n_out = 0.
 * _host: plain C++, no context, no GPU - the definition above triple by triple, the CPU-tested statement of the semantics.
 * vdf_align_windows_rates_stretches: host arrays - hashes, first arrays and skip bytes go up ONCE, for the seed pass and all rounds.
 * _device: DEVICE hashes, first arrays and skip bytes; the rate arrays, a_rate_first, triples and out stay on the host; the call is ordered on
 * `stream` (NULL = the context's) and waits for its own work.  In the context forms round 0 of a chunk is vdf_align_windows_rates*' launch;
 * round k >= 1 walks only the triples that had a record in round k - 1, so a call whose triples have no record launches nothing more.
 * Not offered: a round loop on the device (the records of a round visit the host, which appends the rectangles); flips; a C best_rates;
 * multi-GPU contexts; rates outside [1, 2]. */
typedef struct vdf_alignment_rate_stretch { /* 36 bytes */
    uint32_t a;                /* the eight fields of vdf_alignment_rate */
    uint32_t b;
    uint32_t rate;
    uint32_t first_a;
    uint32_t first_b;
    uint32_t n_windows;
    uint32_t dist_sum;
    uint32_t n_frames_b;
    uint32_t rank;             /* 0 ... max_stretches - 1: 0 is the triple's best stretch */
} vdf_alignment_rate_stretch;
typedef struct vdf_align_rates_stretches_job {
    const uint64_t *a_hashes;
    const uint32_t *a_first;
    const size_t *a_rate_first;
    const uint8_t *a_skip;
    size_t n_a;
    const uint64_t *b_hashes;
    const uint32_t *b_first;
    const uint8_t *b_skip;
    size_t n_b;
    uint32_t n_rates;
    const uint32_t *rate_num;
    const uint32_t *rate_den;
    uint32_t tol_int;
    uint32_t min_run;
    const vdf_video_pair_rate *triples;
    size_t n_triples;
    uint32_t seed;
    uint32_t exclude_same;
    uint32_t max_stretches;
    uint32_t guard;
    vdf_alignment_rate_stretch *out;
    size_t capacity;
    size_t *n_out;
    void *stream;
} vdf_align_rates_stretches_job;
int vdf_align_windows_rates_stretches_host(const vdf_align_rates_stretches_job *job);
int vdf_align_windows_rates_stretches(vdf_ctx *ctx, const vdf_align_rates_stretches_job *job);
int vdf_align_windows_rates_stretches_device(vdf_ctx *ctx, const vdf_align_rates_stretches_job *job);

/* ---- mirrored, flipped and reversed STRETCHES: window hashes with their zero planes -----------------------
 * A mirrored re-upload with its intro trimmed: the variant search sees only frames 0 ... 15 of a file, the align calls only unflipped
 * stretches.  With the zero plane of every window (vdf_hash_windows_u8_planes*) the window hashes of the flipped video follow from the
 * video's own, by the rule of the planes calls below (H_v = (H ^ M_v) & ~Z; variant bit 0 = mirror along W, bit 1 = flip along H, bit 2 =
 * reverse the frames).
 *
 * vdf_window_variants_*: the variant of a SET of window hashes.  hashes / zero: [windows][16], first[n_videos + 1], video v owning the rows
 * first[v] ... first[v + 1] (N of them; 0 is legal); rows outside [first[0], first[n_videos]) are neither read nor written.  Output row
 * first[v] + j = (H[i] ^ M_variant) & ~Z[i] with i = first[v] + j without bit 2 and i = first[v] + N - 1 - j with it; the skip byte
 * (skip nullable; out_skip is null iff skip is) is carried along the same way.  Without bit 2 the rows are the window hashes of the flipped
 * video, word for word.  With bit 2 they are the window hashes of the REVERSED video: exactly so when (F - 16) % window_stride == 0 for its F
 * frames, otherwise those of the reversed video with its first (F - 16) % window_stride frames dropped - still a reversed stretch, on the
 * window grid of the original.
 * Errors, in this order, all VDF_E_INVAL: variant outside 1 ... 7; (n_videos == 0: VDF_OK;) a null required pointer, or exactly one of skip /
 * out_skip; an output that is one of the inputs; a first array that decreases; (device form) a multi-GPU context.  The device form reads the
 * first array back to check it and size its launch; the rows are ordered on `stream`.  The host form takes no context. */
int vdf_window_variants_host(const uint64_t *hashes, const uint64_t *zero, const uint32_t *first, size_t n_videos, const uint8_t *skip,
                             uint32_t variant, uint64_t *out_hashes, uint8_t *out_skip);
int vdf_window_variants_device(vdf_ctx *ctx, const uint64_t *d_hashes, const uint64_t *d_zero, const uint32_t *d_first, size_t n_videos,
                               const uint8_t *d_skip, uint32_t variant, uint64_t *d_out_hashes, uint8_t *d_out_skip, void *stream);
/* vdf_align_windows against the variants of B: for every variant v whose bit is set in variant_mask (bits 1 ... 7), in ascending order, the
 * variant-v set of B is derived (vdf_window_variants_*) and A is aligned against it - the semantics of vdf_align_windows word for word (cell
 * rule, run, score, ties, min_run, skip, the tol clamp, 2^20 windows per video, 2^24 pairs per call), with B's rows replaced by the derived
 * rows.  So offset and start_a + offset index the DERIVED order of b: with bit 2 of v set, derived window j is original window
 * kb = Nb - 1 - j, and the stretch runs backwards through b.
 * A: hashes, first, skip.  B: hashes, ZERO (b_zero, required), first, skip.  b_hashes == NULL is SELF mode: B = A with a_zero as its zero
 * plane (required then, ignored otherwise); only the pairs a < b are evaluated, so a video is never aligned with its own mirror, as
 * vdf_search_variants drops (r, r).
 * out: HOST buffer of `capacity` records ordered by (variant, a, b), at most one per (variant, pair).  *n_out = the number found over all
 * variants; if it exceeds capacity the first `capacity` records in that order are valid - VDF_OK, as the align calls.
 * Errors: those of vdf_align_windows in their order; then variant_mask with bit 0 or a bit above 7; then a missing zero plane; then a
 * multi-GPU context - all VDF_E_INVAL.
 * Where coefficients are exactly zero d(a, v(b)) and d(v(a), b) can differ: the zero plane of b clears bits of v(b) that a may have set.  So
 * near the tolerance a stretch may be found with B flipped and not with the sides swapped (the asymmetry of vdf_search_variants). */
typedef struct vdf_alignment_variant { /* 28 bytes */
    uint32_t a;                /* the six fields of vdf_alignment; offset and start_a + offset count in the DERIVED order of b */
    uint32_t b;
    int32_t offset;
    uint32_t start_a;
    uint32_t n_windows;
    uint32_t dist_sum;
    uint32_t variant;          /* 1 ... 7 */
} vdf_alignment_variant;
int vdf_align_windows_variants_host(const uint64_t *a_hashes, const uint64_t *a_zero, const uint32_t *a_first, size_t n_a,
                                    const uint8_t *a_skip, const uint64_t *b_hashes, const uint64_t *b_zero, const uint32_t *b_first,
                                    size_t n_b, const uint8_t *b_skip, uint32_t tol_int, uint32_t min_run, uint32_t variant_mask,
                                    vdf_alignment_variant *out, size_t capacity, size_t *n_out);
int vdf_align_windows_variants(vdf_ctx *ctx, const uint64_t *a_hashes, const uint64_t *a_zero, const uint32_t *a_first, size_t n_a,
                               const uint8_t *a_skip, const uint64_t *b_hashes, const uint64_t *b_zero, const uint32_t *b_first,
                               size_t n_b, const uint8_t *b_skip, uint32_t tol_int, uint32_t min_run, uint32_t variant_mask,
                               vdf_alignment_variant *out, size_t capacity, size_t *n_out);
int vdf_align_windows_variants_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint64_t *d_a_zero, const uint32_t *d_a_first,
                                      size_t n_a, const uint8_t *d_a_skip, const uint64_t *d_b_hashes, const uint64_t *d_b_zero,
                                      const uint32_t *d_b_first, size_t n_b, const uint8_t *d_b_skip, uint32_t tol_int,
                                      uint32_t min_run, uint32_t variant_mask, vdf_alignment_variant *out, size_t capacity,
                                      size_t *n_out, void *stream);

/* ---- the flipped alignment, seeded: the candidates under every requested variant from one pass over the seeds ----
 * For variant v in 1 ... 7: the variant-v set of B is vdf_window_variants_*'s output, and pair (a, b) is a CANDIDATE UNDER v iff it is a
 * candidate of vdf_align_seed_pairs* on (A, variant-v set of B): seeds are the windows ka % min_run == 0 counted inside video a; neither row
 * skipped; distance over all 16 words <= min(tol_int, 1024); a < b in self mode.  Self mode is B = A with a_zero as its plane, as
 * vdf_align_windows_variants defines it.  A candidate needs only some seed and some row of b, and bit 2 of v only reorders b's rows and
 * carries their skip bytes along: the candidate set under v does not depend on the reversal, only on M_v and Z.  It holds every pair with a
 * record of vdf_align_windows_variants* under v.
 * vdf_align_seed_pairs_variants*: the arguments of vdf_align_windows_variants* up to variant_mask; out is a HOST buffer of `capacity`
 * triples ordered by (variant, a, b); *n_out = the total over the requested variants, the first `capacity` entries are valid if it exceeds
 * capacity - VDF_OK.  Errors: those of vdf_align_seed_pairs* in their order; then variant_mask with bit 0 or a bit above 7; then a missing
 * zero plane; then a multi-GPU context - all VDF_E_INVAL.  The context forms make one pass over the seeds for all requested variants (the
 * seven masks split the 1000 bits into eight classes of 125 on which every M_v is constant, so eight partial sums give every distance).
 * vdf_align_windows_variants_pairs*: vdf_align_windows_variants* restricted to a HOST list (also in the device form) of n_triples
 * (variant, a, b) triples; the list names the variants, there is no mask.  Per variant present in the list, ascending, the set is derived and
 * the align core runs on that variant's sublist.  The records are vdf_alignment_variant, equal field for field to the all-pairs variants
 * call's for the listed triples, in (variant, a, b) order, under the same capacity protocol.  Errors, in this order, all VDF_E_INVAL: a null
 * list with n_triples > 0; those of vdf_align_windows up to the first arrays; n_a or n_b above 2^32 - 1; more than 2^24 listed triples; a
 * list that is not strictly increasing in (variant, a, b); a variant outside 1 ... 7; a triple that names a video that does not exist; a
 * triple with a >= b in self mode (the list failures name the entry's index); a missing zero plane; a multi-GPU context.
 * Each in the three forms: _host (plain C++, no context: vdf_window_variants_host, then the plain host forms - the reference), host arrays
 * through a context, _device (DEVICE arrays and a stream; the call waits for its own work).  A _device form on a multi-GPU context has no
 * device to read the first arrays back from: it makes every check that needs no first array, in the order above, and then refuses the
 * context - a decreasing first array or a video above 2^20 windows is not reported there (as vdf_align_windows_variants_device).
 * Not offered: more than one stretch per pair under a variant; multi-GPU contexts. */
typedef struct vdf_video_pair_variant { /* 12 bytes */
    uint32_t a;                /* video index in A */
    uint32_t b;                /* video index in B (self mode: in A, a < b) */
    uint32_t variant;          /* 1 ... 7 */
} vdf_video_pair_variant;
int vdf_align_seed_pairs_variants_host(const uint64_t *a_hashes, const uint64_t *a_zero, const uint32_t *a_first, size_t n_a,
                                       const uint8_t *a_skip, const uint64_t *b_hashes, const uint64_t *b_zero, const uint32_t *b_first,
                                       size_t n_b, const uint8_t *b_skip, uint32_t tol_int, uint32_t min_run, uint32_t variant_mask,
                                       vdf_video_pair_variant *out, size_t capacity, size_t *n_out);
int vdf_align_seed_pairs_variants(vdf_ctx *ctx, const uint64_t *a_hashes, const uint64_t *a_zero, const uint32_t *a_first, size_t n_a,
                                  const uint8_t *a_skip, const uint64_t *b_hashes, const uint64_t *b_zero, const uint32_t *b_first,
                                  size_t n_b, const uint8_t *b_skip, uint32_t tol_int, uint32_t min_run, uint32_t variant_mask,
                                  vdf_video_pair_variant *out, size_t capacity, size_t *n_out);
int vdf_align_seed_pairs_variants_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint64_t *d_a_zero, const uint32_t *d_a_first,
                                         size_t n_a, const uint8_t *d_a_skip, const uint64_t *d_b_hashes, const uint64_t *d_b_zero,
                                         const uint32_t *d_b_first, size_t n_b, const uint8_t *d_b_skip, uint32_t tol_int,
                                         uint32_t min_run, uint32_t variant_mask, vdf_video_pair_variant *out, size_t capacity,
                                         size_t *n_out, void *stream);
int vdf_align_windows_variants_pairs_host(const uint64_t *a_hashes, const uint64_t *a_zero, const uint32_t *a_first, size_t n_a,
                                          const uint8_t *a_skip, const uint64_t *b_hashes, const uint64_t *b_zero, const uint32_t *b_first,
                                          size_t n_b, const uint8_t *b_skip, const vdf_video_pair_variant *triples, size_t n_triples,
                                          uint32_t tol_int, uint32_t min_run, vdf_alignment_variant *out, size_t capacity, size_t *n_out);
int vdf_align_windows_variants_pairs(vdf_ctx *ctx, const uint64_t *a_hashes, const uint64_t *a_zero, const uint32_t *a_first, size_t n_a,
                                     const uint8_t *a_skip, const uint64_t *b_hashes, const uint64_t *b_zero, const uint32_t *b_first,
                                     size_t n_b, const uint8_t *b_skip, const vdf_video_pair_variant *triples, size_t n_triples,
                                     uint32_t tol_int, uint32_t min_run, vdf_alignment_variant *out, size_t capacity, size_t *n_out);
int vdf_align_windows_variants_pairs_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint64_t *d_a_zero, const uint32_t *d_a_first,
                                            size_t n_a, const uint8_t *d_a_skip, const uint64_t *d_b_hashes, const uint64_t *d_b_zero,
                                            const uint32_t *d_b_first, size_t n_b, const uint8_t *d_b_skip,
                                            const vdf_video_pair_variant *triples, size_t n_triples, uint32_t tol_int, uint32_t min_run,
                                            vdf_alignment_variant *out, size_t capacity, size_t *n_out, void *stream);

/* The class-major rows the seed pass against the variants reads (csrc/window_class_layout.h states the permutation): made
 * callable so that the layout kernel can be held against its host twin word for word, and for callers who want to see what a window looks like
 * to that pass.  hashes / first / skip as vdf_window_variants_*.
 *   zero == NULL: the SEEDS of the set - window first[v] + k min_run of every video v, in order - 36 dwords each: [0, 33) the hash's bits
 *     class-major, 33 the popcount of all 1024 bits, 34 the skip byte as 0 / 1, 35 the video index.
 *   zero != NULL: the ROWS first[0] ... first[n_videos] - 1, 72 dwords each: [0, 33) H & ~Z class-major, 33 / 34 the counts of live (non-Z)
 *     bits of classes 1 ... 4 / 5 ... 7, one byte each from the low byte up, 35 the skip byte as 0 / 1, [36, 69) ~Z class-major, 69 ... 71 zero.
 * out holds capacity_rows rows of that size; *n_rows = the number the layout has.  Errors, in this order, all VDF_E_INVAL: a null required pointer;
 * min_run == 0; more than 2^32 - 1 videos; (device form) a multi-GPU context; a first array that decreases; fewer rows of room than the layout has
 * (*n_rows is set).  _host: plain C++, no context.  _device: DEVICE pointers, out included (16-byte aligned); the first array is read back; the
 * call waits for its own work. */
int vdf_window_class_layout_host(const uint64_t *hashes, const uint64_t *zero, const uint32_t *first, size_t n_videos, const uint8_t *skip,
                                 uint32_t min_run, uint32_t *out, size_t capacity_rows, size_t *n_rows);
int vdf_window_class_layout_device(vdf_ctx *ctx, const uint64_t *d_hashes, const uint64_t *d_zero, const uint32_t *d_first, size_t n_videos,
                                   const uint8_t *d_skip, uint32_t min_run, uint32_t *d_out, size_t capacity_rows, size_t *n_rows,
                                   void *stream);

/* ---- clips of DIFFERENT frame sizes in one call ----------------------------------------------------
 * A library holds dozens of resolutions and its files arrive in any order.  All clips of a call live in ONE
 * buffer of buf_bytes bytes and name their place by offset: every address is checked against that buffer on
 * the host, over all clips, before anything is queued (a rejected call launches nothing).  Clip i's hash lands
 * at out_hashes + 16 i (out_dontcare[i]), whatever order the kernels take the clips in.  Rows are tightly
 * packed (w bytes apart); the crop box is read in place, as in vdf_hash_frames_u8_cropped_device.
 * Errors, in this order, each message naming the first offending clip: frames_per_clip < 16 ->
 * VDF_E_NOT_ENOUGH_FRAMES; a zero dimension -> VDF_E_BAD_DIMS; frame_stride < w*h -> VDF_E_INVAL; a box that
 * leaves no pixels -> VDF_E_INVAL; offset + 15*frame_stride + w*h > buf_bytes -> VDF_E_INVAL; a box size whose
 * coefficients do not fit the i8 split -> VDF_E_BAD_DIMS.
 * Clips that all share (w, h, frame_stride) at offsets one positive step apart take exactly the kernels of
 * vdf_hash_frames_u8[_cropped]_device.  A multi-GPU context refuses both calls with VDF_E_INVAL. */
typedef struct vdf_clip {      /* 40 bytes */
    uint64_t offset;           /* first byte of frame 0, relative to the buffer */
    uint64_t frame_stride;     /* bytes between frames, >= w*h */
    uint32_t w;
    uint32_t h;
    uint32_t crop_left;        /* the four edge offsets of the crop box (crop.rs:3-10), in the order of the `crops` arrays above; */
    uint32_t crop_right;       /* all zero = whole frame */
    uint32_t crop_top;
    uint32_t crop_bottom;
} vdf_clip;
int vdf_hash_clips_u8(vdf_ctx *ctx, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips,
                      uint32_t frames_per_clip, uint64_t *out_hashes, uint32_t *out_dontcare);
/* clips: HOST array.  The call returns once the descriptors have left the host; the hashes are ordered on `stream`. */
int vdf_hash_clips_u8_device(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips,
                             uint32_t frames_per_clip, uint64_t *d_out_hashes, uint32_t *d_out_dontcare, void *stream);
/* Cropdetect::Letterbox on clips of different frame sizes: detection on per-clip descriptors (frames 0 and 8 of every clip, the rules of
 * vdf_cropdetect_letterbox_device), then the mixed hash on the detected boxes.  The letterbox calls take the whole frame, as the reference does:
 * after the errors above, in their order, a clip whose four crop fields are not all zero -> VDF_E_INVAL ("caller-supplied crop box in a
 * letterbox call", naming the first such clip).  Every check runs before anything is queued.  Clips that share (w, h, frame_stride) at
 * offsets one positive step apart take exactly the route of vdf_cropdetect_letterbox_device / vdf_hash_frames_u8_letterbox_device.
 * The hash calls WAIT for their detect (the kernel per box shape is chosen on the host, as for large frames above); a detected box size
 * whose coefficients do not fit the i8 split -> VDF_E_BAD_DIMS, reported after the detect, and no hash is written.  A multi-GPU context
 * refuses all three with VDF_E_INVAL. */
/* boxes only: d_crops DEVICE [n_clips][4] l, r, t, b, ordered on stream; queues its kernels and waits for nothing but the upload of its
 * descriptors (which, in stream order, waits for what the caller queued in front of it) */
int vdf_cropdetect_letterbox_clips_device(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips,
                                          uint32_t frames_per_clip, uint32_t *d_crops, void *stream);
/* detect + crop + hash; out_crops HOST [n_clips][4], nullable; the call waits for its detect, the hashes are ordered on stream */
int vdf_hash_clips_u8_letterbox_device(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips,
                                       uint32_t frames_per_clip, uint64_t *d_out_hashes, uint32_t *d_out_dontcare,
                                       uint32_t *out_crops, void *stream);
int vdf_hash_clips_u8_letterbox(vdf_ctx *ctx, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips,
                                uint32_t frames_per_clip, uint64_t *out_hashes, uint32_t *out_crops, uint32_t *out_dontcare);

/* ---- every 16-frame window of videos of DIFFERENT frame sizes and lengths in one call ----------------
 * The producer of what the align calls read.  n_videos videos in ONE buffer, each with its own vdf_clip descriptor (size,
 * frame stride, optional crop box, read in place) and its own frame count n_frames[i] (HOST array).  Window k of video i is frames
 * [k * window_stride, k * window_stride + 16) of that video inside its box; with first[] = the prefix sums of
 * vdf_hash_window_count(n_frames[i], window_stride) (vdf_hash_windows_clips_first) its hash goes to out_hashes + 16 (first[i] + k), its
 * don't-care count to out_dontcare[first[i] + k] (nullable) and, in the _planes forms, its zero plane to out_zero + 16 (first[i] + k)
 * (required there) - whatever order the kernels take the videos in.  The words are the words vdf_hash_windows_u8* gives for each video alone
 * (on a contiguous cropped copy, if it has a box).
 * vdf_hash_windows_clips_first: host only, no context; first has n_videos + 1 entries, the caller sizes its buffers by first[n_videos].
 * A null pointer, window_stride == 0 or 2^32 windows or more -> VDF_E_INVAL; an n_frames below 16 -> VDF_E_NOT_ENOUGH_FRAMES.
 * Errors of the hash calls, checked over all videos on the host before anything is queued (a rejected call launches nothing), in this order,
 * each message naming the first offending video: n_frames < 16 -> VDF_E_NOT_ENOUGH_FRAMES; a zero dimension -> VDF_E_BAD_DIMS;
 * frame_stride < w*h -> VDF_E_INVAL; a box that leaves no pixels -> VDF_E_INVAL; offset + (n_frames - 1)*frame_stride + w*h > buf_bytes ->
 * VDF_E_INVAL; window_stride == 0 -> VDF_E_INVAL; an n_frames within 64 of 2^32 -> VDF_E_INVAL; 2^32 windows or more in the call ->
 * VDF_E_INVAL; (n_videos == 0: VDF_OK, nothing is launched;) a null pointer -> VDF_E_INVAL (a null clips or n_frames array with n_videos > 0 is
 * reported before everything else: there is nothing to check the videos by); a box size whose coefficients do not fit the i8 split ->
 * VDF_E_BAD_DIMS; _planes forms: an axis size whose resize table is not its own mirror image -> VDF_E_BAD_DIMS; a multi-GPU context ->
 * VDF_E_INVAL, last.
 * Videos that all share (w, h, frame_stride, n_frames), have no box and sit at offsets one positive step apart take exactly the route of
 * vdf_hash_windows_u8[_planes]_device with clip_stride = that step.  The host forms upload the buffer in one piece.  The device forms are
 * ordered on `stream`; clips and n_frames are HOST arrays, and the call returns once the descriptors have left the host. */
int vdf_hash_windows_clips_first(const uint32_t *n_frames, size_t n_videos, uint32_t window_stride, uint32_t *first);
int vdf_hash_windows_clips_u8(vdf_ctx *ctx, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames,
                              size_t n_videos, uint32_t window_stride, uint64_t *out_hashes, uint32_t *out_dontcare);
int vdf_hash_windows_clips_u8_device(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames,
                                     size_t n_videos, uint32_t window_stride, uint64_t *d_out_hashes, uint32_t *d_out_dontcare, void *stream);
int vdf_hash_windows_clips_u8_planes(vdf_ctx *ctx, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames,
                                     size_t n_videos, uint32_t window_stride, uint64_t *out_hashes, uint32_t *out_dontcare, uint64_t *out_zero);
int vdf_hash_windows_clips_u8_planes_device(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips,
                                            const uint32_t *n_frames, size_t n_videos, uint32_t window_stride, uint64_t *d_out_hashes,
                                            uint32_t *d_out_dontcare, uint64_t *d_out_zero, void *stream);

/* ---- the RETIMED windows of videos of different frame sizes and lengths in one call ----------------
 * vdf_hash_windows_clips_u8[_device] with the windows of vdf_hash_windows_u8_retimed[_device]: the producer of the A side of
 * vdf_align_windows_retimed* for a whole library.  The video arguments are those of vdf_hash_windows_clips_u8*: n_videos videos in ONE buffer,
 * each with its own vdf_clip (offset, frame stride, size, optional crop box, read in place) and its own frame count n_frames[i]; clips and
 * n_frames are HOST arrays.  The rate arguments are those of vdf_hash_windows_u8_retimed*: 1 <= rate_den <= rate_num <= 2 rate_den,
 * rate_num <= 65535, tap(t) = floor(t * rate_num / rate_den), span = tap(15) + 1.  Retimed window k of video i is the hash of its frames
 * k * window_stride + tap(t), t = 0 ... 15, inside its box.  With first[] = the prefix sums of
 * vdf_hash_window_count_retimed(n_frames[i], window_stride, rate_num, rate_den) (vdf_hash_windows_clips_first_retimed) its hash goes to
 * out_hashes + 16 (first[i] + k) and its don't-care count to out_dontcare[first[i] + k] (nullable).  Words and counts are exactly those of
 * vdf_hash_windows_u8_retimed on that video alone (on a contiguous cropped copy, if it has a box).
 * Errors, checked over all videos on the host before anything is queued (a rejected call launches nothing), each message naming the first
 * offending video where one is meant: first those of vdf_hash_windows_clips_u8*, in that call's order (an n_frames below 16 ->
 * VDF_E_NOT_ENOUGH_FRAMES first ... a multi-GPU context -> VDF_E_INVAL); then a rate outside the range or rate_den == 0 -> VDF_E_INVAL; then an
 * n_frames[i] < span -> VDF_E_NOT_ENOUGH_FRAMES (a library call returns no 0-window video).  n_videos == 0: VDF_OK, nothing is launched.
 * vdf_hash_windows_clips_first_retimed: host only, no context; first has n_videos + 1 entries.  A null pointer, window_stride == 0 or 2^32
 * windows or more -> VDF_E_INVAL; an n_frames below 16 -> VDF_E_NOT_ENOUGH_FRAMES; then the two rate rules above.
 * Routes: a rate whose taps are 0 ... 15 (rate_num == rate_den, 25/24) IS vdf_hash_windows_clips_u8[_device]: its route, its words.  Videos
 * that all share (w, h, frame_stride, n_frames), have no box and sit at offsets one positive step apart take exactly the route of
 * vdf_hash_windows_u8_retimed_device with clip_stride = that step.  Everything else is resized once, frame by frame, and hashed by one kernel
 * whose workgroups find their video in a segment table.  The host form uploads the buffer in one piece.  The device form is ordered on `stream`
 * and returns once the descriptors have left the host.
 * Not here: zero planes of retimed windows, the batching queue, multi-GPU contexts.  Several rates from one read of the library:
 * vdf_hash_windows_clips_u8_rates[_device] below. */
int vdf_hash_windows_clips_first_retimed(const uint32_t *n_frames, size_t n_videos, uint32_t window_stride, uint32_t rate_num, uint32_t rate_den,
                                         uint32_t *first);
int vdf_hash_windows_clips_u8_retimed(vdf_ctx *ctx, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames,
                                      size_t n_videos, uint32_t window_stride, uint32_t rate_num, uint32_t rate_den, uint64_t *out_hashes,
                                      uint32_t *out_dontcare);
int vdf_hash_windows_clips_u8_retimed_device(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips,
                                             const uint32_t *n_frames, size_t n_videos, uint32_t window_stride, uint32_t rate_num,
                                             uint32_t rate_den, uint64_t *d_out_hashes, uint32_t *d_out_dontcare, void *stream);

/* ---- the retimed windows of a library of different frame sizes and lengths at SEVERAL rates in one call ----------------
 * vdf_hash_windows_clips_u8_retimed[_device] with the rate list of vdf_hash_windows_u8_rates[_device]: for the owner of a
 * library who does not know the rate.  Every frame is read, resized and spatially transformed ONCE, whatever the number of rates.  The job:
 *   buf, buf_bytes, clips, n_frames, n_videos, window_stride   as vdf_hash_windows_clips_u8*'s arguments of those names; buf is a host pointer
 *                              in vdf_hash_windows_clips_u8_rates and a device pointer in _device; clips and n_frames are HOST arrays;
 *   n_rates, rate_num, rate_den   1 ... VDF_WINDOWS_MAX_RATES rates, each as vdf_hash_windows_u8_retimed takes it; HOST arrays in both forms.
 *                              Duplicate and unreduced rates are legal, each listed rate gets its block;
 *   out_hashes, out_dontcare   RATE-MAJOR, and every block is a library: with first[r][] = the prefix sums of
 *                              vdf_hash_window_count_retimed(n_frames[i], window_stride, rate_num[r], rate_den[r]) - n_videos + 1 entries, exactly
 *                              what vdf_hash_windows_clips_first_retimed gives for rate r - and rate_first[r] = the totals of the blocks before r,
 *                              window k of video i at rate r is row rate_first[r] + first[r][i] + k: 16 words of out_hashes, one entry of
 *                              out_dontcare (nullable).  Host pointers in the host form, device pointers in the device form;
 *   stream                     device form only: the call is ordered on it, NULL = the context's stream.
 * Block r is, word for word and count for count, what vdf_hash_windows_clips_u8_retimed[_device] writes for rate r on the same arguments, also
 * at the plain taps (1/1, 25/24).  (out_hashes + 16 rate_first[r], first[r]) is, unchanged, the A side of vdf_align_windows_retimed*; the 1/1
 * block is a B side.
 * vdf_hash_windows_clips_first_rates: host only, no context; first has n_rates * (n_videos + 1) entries, row r at first + r (n_videos + 1);
 * rate_first (nullable) has n_rates + 1 entries, the last one the total number of rows.  A null first, window_stride == 0, n_rates outside
 * 1 ... 8 or a null rate array -> VDF_E_INVAL; an n_frames below 16 -> VDF_E_NOT_ENOUGH_FRAMES; then the rate rules and the row limit below.
 * Errors of the hash calls, checked on the host before anything is queued (a rejected call launches nothing), in this order: a null ctx or
 * job -> VDF_E_INVAL; those of vdf_hash_windows_clips_u8*, in that call's order, ending with a multi-GPU context -> VDF_E_INVAL; n_rates
 * outside 1 ... 8 or a null rate array -> VDF_E_INVAL; the first rate outside 1 <= den <= num <= 2 den, num <= 65535 -> VDF_E_INVAL; in list
 * order, the first rate for which some n_frames[i] < span -> VDF_E_NOT_ENOUGH_FRAMES (the message names the rate's index and the first such
 * video: a library call returns no 0-window video at any rate); 2^32 rows or more in all -> VDF_E_INVAL; n_videos == 0 -> VDF_OK, nothing
 * is launched.
 * Routes: videos that all share (w, h, frame_stride, n_frames), have no box and sit at offsets one positive step apart take exactly the route
 * of vdf_hash_windows_u8_rates_device with clip_stride = that step (its rows coincide: first[r][c] = c n_win_r).  Everything else - a one-rate
 * list and plain-tap rates included - is resized once and hashed by one kernel whose workgroups find their video in a segment table.
 * The host form uploads the buffer ONCE, downloads all blocks and waits.  The device form only queues work on job->stream and returns once the
 * descriptors and the rate arrays have left the host.
 * Not here: zero planes, the batching queue, multi-GPU contexts (VDF_E_INVAL), rates outside [1, 2]. */
typedef struct vdf_windows_clips_rates_job {
    const uint8_t *buf;
    size_t buf_bytes;
    const vdf_clip *clips;
    const uint32_t *n_frames;
    size_t n_videos;
    uint32_t window_stride;
    uint32_t n_rates;
    const uint32_t *rate_num;
    const uint32_t *rate_den;
    uint64_t *out_hashes;
    uint32_t *out_dontcare;
    void *stream;
} vdf_windows_clips_rates_job;
int vdf_hash_windows_clips_first_rates(const uint32_t *n_frames, size_t n_videos, uint32_t window_stride, uint32_t n_rates,
                                       const uint32_t *rate_num, const uint32_t *rate_den, uint32_t *first, size_t *rate_first);
int vdf_hash_windows_clips_u8_rates(vdf_ctx *ctx, const vdf_windows_clips_rates_job *job);
int vdf_hash_windows_clips_u8_rates_device(vdf_ctx *ctx, const vdf_windows_clips_rates_job *job);

/* ---- mirrored, flipped and reversed duplicates from ONE hash pass -------------------------------------
 * The reference cannot see through a horizontal mirror or a flip (vid_dup_finder_lib/src/lib.rs:102-111).  Here the hash of the
 * flipped clip follows from the clip's own hash: the quantised resize tables are mirror-symmetric and the DCT's first step is
 * x[i] +- x[15 - i], so flipping the clip along W, along H or in time multiplies coefficient (kt, kx, ky) by (-1)^kx, (-1)^ky or
 * (-1)^kt - bit for bit, up to the sign of zero.  The hash keeps coef > 0.0, so all that is missing is where the
 * coefficients are exactly zero - the ZERO PLANE Z: 16 words per clip, bit i set iff coefficient i == 0.0 (bits 1000 ... 1023 are 0,
 * and H & Z == 0).  Then, with variant v: bit 0 = mirror along W, bit 1 = flip along H, bit 2 = reverse the 16 frames used, and
 *     M_v[i] = 1 iff i < 1000 and ((v & 1) kx + ((v >> 1) & 1) ky + ((v >> 2) & 1) kt) is odd,   i = 100 kt + 10 kx + ky,
 *     H_v = (H ^ M_v) & ~Z
 * is exactly the hash the plain call gives for the flipped frames.  Exact zeros are not rare (a static clip has 900).
 *
 * The planes calls are the plain calls plus out_zero (n_clips x 16 words, required): same checks in the same order, same kernel
 * route for the same input, out_hashes bit-identical to the plain call's.  An axis size whose resize table is not its own mirror
 * image would be refused with VDF_E_BAD_DIMS (none is, for 1 ... 4200; the call asks per size).  The clips calls take crop boxes in
 * their descriptors, so they are also the letterboxed form - detect with the calls above, pass the boxes in - and a variant of a
 * cropped clip is the flip of the CROPPED clip.  A multi-GPU context refuses all four with VDF_E_INVAL.
 * The app's hash cache has no room for the plane: hashes loaded from a cache cannot be flipped. */
int vdf_hash_frames_u8_planes(vdf_ctx *ctx, const uint8_t *frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w,
                              uint32_t h, size_t frame_stride, size_t clip_stride, uint64_t *out_hashes,
                              uint32_t *out_dontcare, uint64_t *out_zero);
int vdf_hash_frames_u8_planes_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                                     uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride, uint64_t *d_out_hashes,
                                     uint32_t *d_out_dontcare, uint64_t *d_out_zero, void *stream);
int vdf_hash_clips_u8_planes(vdf_ctx *ctx, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips,
                             uint32_t frames_per_clip, uint64_t *out_hashes, uint32_t *out_dontcare, uint64_t *out_zero);
int vdf_hash_clips_u8_planes_device(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips,
                                    uint32_t frames_per_clip, uint64_t *d_out_hashes, uint32_t *d_out_dontcare,
                                    uint64_t *d_out_zero, void *stream);
/* H_v of one hash (host only, no context): hash, zero, out = 16 words each (out may alias hash).  variant > 7 or a null pointer ->
 * VDF_E_INVAL; variant 0 is the identity on a hash of the planes calls. */
int vdf_hash_variant(const uint64_t *hash, const uint64_t *zero, uint32_t variant, uint64_t *out);
/* The same for n resident hashes: d_out (n x 16 words, not d_hashes or d_zero) ordered on stream.  Single-device contexts. */
int vdf_hash_variants_device(vdf_ctx *ctx, const uint64_t *d_hashes, const uint64_t *d_zero, size_t n, uint32_t variant,
                             uint64_t *d_out, void *stream);
/* Which entries look like the MIRROR of which: for every variant v whose bit is set in variant_mask (bits 1 ... 7; bit 0 or a bit
 * above 7 -> VDF_E_INVAL) the library derives V_v = the variant-v hashes on the device and runs the reference search
 * (vdf_search_refs: search_one's +-5% windows, search_algorithm.rs:63-77,173-185) with V_v as the references and the plain hashes
 * as the candidates, both carrying the same durations.  hashes / zero / durations: n entries in sorted order.  The pair (r, r) - a
 * clip against its own mirror (a static or symmetric clip is its own mirror) - is dropped, and so are references left without a
 * match.  out: the caller's array of 8 vdf_groups, indexed by v; out[v] of a requested v is in the reference-search shape
 * (ref_index = r, members ascending): "the variant v of r looks like these".  The others are zeroed.  Release each with
 * vdf_groups_free().  A pair may be reported from both sides (r in a's group and a in r's); and where coefficients are exactly zero
 * d(v(a), b) and d(a, v(b)) can differ (the zero plane of a clears bits of v(a) that b may have set), so near the tolerance it
 * may be reported from one side only.  Single-device contexts. */
int vdf_search_variants(vdf_ctx *ctx, const uint64_t *hashes, const uint64_t *zero, const uint32_t *durations, size_t n,
                        uint32_t tol_int, uint32_t variant_mask, vdf_groups *out /* [8] */);
int vdf_search_variants_device(vdf_ctx *ctx, const uint64_t *d_hashes, const uint64_t *d_zero, const uint32_t *d_durations,
                               size_t n, uint32_t tol_int, uint32_t variant_mask, vdf_groups *out /* [8] */, void *stream);

/* ---- search(): replaces Search::search_self, search_algorithm.rs:81-171 (hot loop :150-156) --
 * hashes: n x 16 words, durations: n, both in sorted order.  tol_int from vdf_tolerance_int().
 * Groups come back exactly as search() builds them (video_dup_finder.rs:7-13): members = hits in
 * sorted order then the target; groups in descending target order; every group has >= 2 members. */
int vdf_search_self(vdf_ctx *ctx, const uint64_t *hashes, const uint32_t *durations, size_t n, uint32_t tol_int,
                    vdf_groups *out);

/* ---- search_with_references(): replaces Search::search_one + duration_slice,
 * search_algorithm.rs:63-77,173-185, driven as video_dup_finder.rs:19-46 does (one reference at a
 * time, consume = false).  Candidates in sorted order; references in the caller's order.
 * Groups: one per reference with >= 1 hit, in reference input order; members ascending. */
int vdf_search_refs(vdf_ctx *ctx, const uint64_t *cand_hashes, const uint32_t *cand_durations, size_t n_cand,
                    const uint64_t *ref_hashes, const uint32_t *ref_durations, size_t n_ref, uint32_t tol_int,
                    vdf_groups *out);

/* ---- device-resident pieces (what the host-level calls above are built from) -----------------
 * These let a caller keep the hash database in HBM, shard the work over several processes
 * (one GPU each) and merge on the host.  All produce the thresholded adjacency; the greedy,
 * order-dependent part of search_self is replayed on the host by vdf_replay_self().
 *
 * vdf_search_self_device: emits every pair (i, j), i < j < rhs(i), hamming <= tol_int, where
 *   rhs(i) = first index with duration > (f64(duration[i]) * 1.1) as u32   (search_algorithm.rs:99).
 *   Row tiles (vdf_row_tile_size() consecutive targets) are dealt round-robin: this call handles
 *   tiles t with t % shard_count == shard_index.  Only rows in [row_begin, row_end) are searched.
 *   d_matched (nullable): bitmap, 1 bit per entry, bit set = entry already consumed; such
 *   entries are skipped both as targets and as candidates (exactly the `matched` flag).
 *   hits (HOST buffer, capacity entries) receives the pairs sorted by (row, col); *n_hits is the
 *   number produced by the device (may exceed capacity); *overflow_row is the smallest row that
 *   lost a hit (or, on the matrix-core backend, a suspect pair that could not be queued for the exact
 *   second pass: only possible with very dense near-duplicates), or UINT32_MAX.  Rows below
 *   *overflow_row are complete.
 *   Returns VDF_OK also when a buffer overflowed: check *overflow_row. */
int vdf_search_self_device(vdf_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_durations, size_t n,
                           uint32_t tol_int, uint32_t shard_index, uint32_t shard_count, uint32_t row_begin,
                           uint32_t row_end, const uint32_t *d_matched, vdf_hit *hits, uint64_t capacity,
                           uint64_t *n_hits, uint32_t *overflow_row, void *stream);

/* The replay-only form of vdf_search_self_device for a caller that shards search() over PROCESSES (one GPU each) and feeds the
 * merged lists to vdf_replay_self and nothing else: hits of rows that can never become targets of the greedy loop
 * (search_algorithm.rs:131-170: a row with an incoming hit from a root - a row nobody hits - is consumed before its turn) are
 * dropped on the device before the sort and the download; a cluster of s mutual duplicates sends down s - 1 pairs, not
 * s (s - 1) / 2.  Whether a row is such a row is a property of the COMPLETE hit set, which a sharded launch has spread over
 * its shards, so the shards meet three times through the caller's callbacks (every shard of the launch must make the call,
 * also one whose tiles produce no hits; xchg = NULL with shard_count = 1 is the unsharded case, and with shard_count > 1
 * disables the filter):
 *   agree:     in/out *all_complete (this shard saw no buffer overflow -> AND over the shards), *total_hits (-> sum);
 *              the filter runs only if all are complete (and the total is worth it) - the same decision on every shard;
 *   or_bitmap: d_bitmap[0 .. n_words) (DEVICE, 1 bit per entry) |= every other shard's, in place; the library's kernels that
 *              wrote it were queued on `stream` and the ones that read it will be - order the exchange on it or finish it
 *              before returning (all-gather + vdf_bitmap_or_device, or an all-reduce(MAX) of a byte map: RCCL has no OR).
 *              Called twice per filtered launch (has-incoming, covered).
 * Callbacks return 0 or a negative vdf_status, which the call hands back.  *n_hits = the pairs kept; everything else as
 * vdf_search_self_device (after an overflow nothing is dropped and the overflow protocol applies unchanged). */
typedef struct vdf_shard_exchange {
    void *user;
    int (*agree)(void *user, int *all_complete, uint64_t *total_hits);
    int (*or_bitmap)(void *user, uint32_t *d_bitmap, size_t n_words, void *stream);
} vdf_shard_exchange;
int vdf_search_self_device_replay(vdf_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_durations, size_t n,
                                  uint32_t tol_int, uint32_t shard_index, uint32_t shard_count, uint32_t row_begin,
                                  uint32_t row_end, const uint32_t *d_matched, vdf_hit *hits, uint64_t capacity,
                                  uint64_t *n_hits, uint32_t *overflow_row, const vdf_shard_exchange *xchg, void *stream);
/* d_dst[w] |= d_srcs[0 * n_words + w] | ... | d_srcs[(n_srcs - 1) * n_words + w] on the device (the local half of an OR over
 * shards after an all-gather; with n_srcs = 1 and a zeroed destination: a copy).  Single-device contexts.  Takes no lock:
 * callable from inside an or_bitmap callback. */
int vdf_bitmap_or_device(vdf_ctx *ctx, uint32_t *d_dst, const uint32_t *d_srcs, size_t n_words, uint32_t n_srcs, void *stream);

/* vdf_search_refs_device: emits every pair (r, j) with j inside reference r's +-5% window
 * (search_algorithm.rs:173-185) and hamming <= tol_int; row = r + ref_index_base, hits (HOST
 * buffer) sorted by (row, col).  Every hit is part of the output here (consume = false), so an
 * undersized buffer is simply an error: VDF_E_OVERFLOW with *n_hits = the size required. */
int vdf_search_refs_device(vdf_ctx *ctx, const uint64_t *d_cand_hashes, const uint32_t *d_cand_durations,
                           size_t n_cand, const uint64_t *d_ref_hashes, const uint32_t *d_ref_durations,
                           size_t n_ref, uint32_t tol_int, uint32_t ref_index_base, vdf_hit *hits,
                           uint64_t capacity, uint64_t *n_hits, void *stream);

/* Search::sort on the device (search_algorithm.rs:55-61: stable sort_by_key on (duration, src_path)) for a database that is
 * already resident in HBM - hashes just produced on the GPU need not visit the host between hashing and searching.
 * d_perm_out[k] = input index of the entry at sorted position k.  Paths stay with the caller: d_path_rank (DEVICE, nullable)
 * gives each entry the rank of its src_path among the caller's paths in PathBuf's (component-wise) order, equal paths sharing
 * a rank; NULL = all paths equal.  Entries with equal (duration, rank) keep their input order, as the stable sort does. */
int vdf_sort_order_device(vdf_ctx *ctx, const uint32_t *d_durations, const uint32_t *d_path_rank, size_t n,
                          uint32_t *d_perm_out, void *stream);
/* d_hashes_out[k] = d_hashes[d_perm[k]] (and the durations likewise; both duration pointers may be NULL).  Not in place. */
int vdf_apply_order_device(vdf_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_durations, const uint32_t *d_perm, size_t n,
                           uint64_t *d_hashes_out, uint32_t *d_durations_out, void *stream);

/* A promise that lets searches against ONE resident database skip work: until the next call of this function the n x 16 words at
 * d_hashes will not change.  Searches whose candidate database is exactly (d_hashes, n) then reuse the operand expansion the
 * matrix-core backend makes of it (0.15 ms per million hashes - a sixth of a reference search at the BASELINE configs[4] shape:
 * the app searches its one cache database with reference set after reference set, app_fns.rs:428-482).  d_hashes = NULL withdraws the
 * promise.  Single-device contexts. */
int vdf_ctx_pin_database(vdf_ctx *ctx, const uint64_t *d_hashes, size_t n);

uint32_t vdf_row_tile_size(void); /* rows per tile of the default backend (informational: any shard_count works) */

/* Host replay of search_self's consumption order (search_algorithm.rs:131-170) over hits sorted
 * by (row, col).  matched (nullable, n bytes, in/out) carries consumption state between partial
 * replays; rows in [row_begin, row_end) are replayed.  Appends groups in ASCENDING target order
 * to *out (which must be zero-initialised before the first call); call vdf_groups_finish_self()
 * once at the end to apply ret.reverse() (search_algorithm.rs:167). */
int vdf_replay_self(size_t n, const vdf_hit *hits, uint64_t n_hits, uint32_t row_begin, uint32_t row_end,
                    uint8_t *matched, vdf_groups *out);
int vdf_groups_finish_self(vdf_groups *g);
/* Hits into (row, col) order, in place (host; what the replay and the grouping expect: merging the lists of several
 * processes, one GPU each, is concatenate + this). */
int vdf_sort_hits(vdf_hit *hits, uint64_t n_hits);
/* Groups for search_with_references from hits sorted by (row, col). */
int vdf_groups_from_ref_hits(const vdf_hit *hits, uint64_t n_hits, vdf_groups *out);

/* ---- multi-GPU contexts: data already resident on the devices -------------------------------------------------
 * Array arguments have one entry per slot of the context (vdf_ctx_device_count()); pointer k is a DEVICE pointer on
 * the GPU of slot k.  The caller's work that produced the buffers must be complete (the library runs on its own
 * streams).  Results are identical to the single-device calls on the concatenated arrays.
 *
 * vdf_search_self_shards: the sorted database (Search::sort order, search_algorithm.rs:55-61) cut into consecutive
 *   shards, shard k on device k (sizes may differ, may be 0).  One all-gather of the hashes ((n / G) x 16 x u64 per
 *   device) and one of the durations replicate it - ncclAllGather over xGMI when the shards are equal, the same
 *   exchange as grouped ncclBroadcasts otherwise - then as vdf_search_self.  RCCL failures -> VDF_E_RCCL.
 * vdf_search_refs_shards: candidates sharded and gathered the same way; the references are the concatenation of the
 *   per-device reference shards (group ref_index = position in that concatenation); device k searches its own.
 * vdf_hash_frames_u8_shards: every device hashes its own clips (independent: no communication);
 *   d_out_dontcare may be NULL (or hold NULLs). */
int vdf_search_self_shards(vdf_ctx *ctx, const uint64_t *const *d_hash_shards, const uint32_t *const *d_dur_shards,
                           const size_t *shard_n, uint32_t tol_int, vdf_groups *out);
int vdf_search_refs_shards(vdf_ctx *ctx, const uint64_t *const *d_cand_hash_shards, const uint32_t *const *d_cand_dur_shards,
                           const size_t *cand_shard_n, const uint64_t *const *d_ref_hash_shards,
                           const uint32_t *const *d_ref_dur_shards, const size_t *ref_shard_n, uint32_t tol_int,
                           vdf_groups *out);
int vdf_hash_frames_u8_shards(vdf_ctx *ctx, const uint8_t *const *d_frames, const size_t *n_clips, uint32_t frames_per_clip,
                              uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride, uint64_t *const *d_out_hashes,
                              uint32_t *const *d_out_dontcare);

/* ---- batching queue for concurrent per-file callers ------------------------------------------------
 * The app hashes one file per rayon worker (vid_dup_finder_app/src/video_hash_filesystem_cache/
 * video_hash_filesystem_cache.rs:237-257 -> VideoHashBuilder::hash, video_hash_builder.rs:80-82,214-223).
 * vdf_hash_queue_submit may be called from any number of threads: the clips of concurrent callers are
 * hashed by batched launches (the first caller of a batch waits up to max_wait_us for others or until
 * max_batch clips joined).  The queue keeps two batch slots per GPU of the context, each with pinned staging and a
 * private context: while one batch is on the GPU the next one is already collecting (and may launch).
 * frames = 16 gray frames of w x h, tightly packed; blocks until the hash is
 * there.  letterbox != 0 applies Cropdetect::Letterbox first (out_crop, nullable, gets the box). */
typedef struct vdf_hash_queue vdf_hash_queue;
int vdf_hash_queue_create(vdf_ctx *ctx, uint32_t w, uint32_t h, uint32_t max_batch, uint32_t max_wait_us, int letterbox,
                          vdf_hash_queue **out);
int vdf_hash_queue_submit(vdf_hash_queue *q, const uint8_t *frames, uint64_t *out_hash, uint32_t *out_crop);
int vdf_hash_queue_stats(vdf_hash_queue *q, uint64_t *n_batches, uint64_t *n_clips);
/* The largest number of batches that were on the GPU(s) at the same time since the queue was created (>= 2 shows that a
 * second batch was collected and launched while the first was still running). */
int vdf_hash_queue_in_flight_max(vdf_hash_queue *q, uint32_t *out);
void vdf_hash_queue_destroy(vdf_hash_queue *q);

/* The same queue for clips of ANY frame size: one queue serves a whole library, whatever resolutions its files have.
 * A batch closes when max_batch clips joined, when the next clip would not fit the slot's staging_bytes of pinned
 * memory, or when its first caller has waited max_wait_us; the batch is hashed by one vdf_hash_clips_u8 call.
 * slots_per_gpu: batches in the making per GPU, 0 = 2, at most 16.  frames = 16 gray frames of w x h, tightly packed;
 * blocks until the hash is there.  A clip of more than staging_bytes (16 * w * h) -> VDF_E_INVAL. */
typedef struct vdf_hash_queue_mixed vdf_hash_queue_mixed;
int vdf_hash_queue_create_mixed(vdf_ctx *ctx, size_t staging_bytes, uint32_t max_batch, uint32_t max_wait_us,
                                uint32_t slots_per_gpu, vdf_hash_queue_mixed **out);
/* The same queue with Cropdetect::Letterbox: a batch is hashed by one vdf_hash_clips_u8_letterbox call. */
int vdf_hash_queue_create_mixed_letterbox(vdf_ctx *ctx, size_t staging_bytes, uint32_t max_batch, uint32_t max_wait_us,
                                          uint32_t slots_per_gpu, vdf_hash_queue_mixed **out);
int vdf_hash_queue_mixed_submit(vdf_hash_queue_mixed *q, const uint8_t *frames, uint32_t w, uint32_t h, uint64_t *out_hash);
/* either kind of mixed queue; out_crop (nullable): the clip's box l, r, t, b - a plain queue writes zeros.  vdf_hash_queue_mixed_submit on a
 * letterbox queue hashes with letterbox and drops the box. */
int vdf_hash_queue_mixed_submit_crop(vdf_hash_queue_mixed *q, const uint8_t *frames, uint32_t w, uint32_t h,
                                     uint64_t *out_hash, uint32_t *out_crop);
int vdf_hash_queue_mixed_stats(vdf_hash_queue_mixed *q, uint64_t *n_batches, uint64_t *n_clips);
int vdf_hash_queue_mixed_in_flight_max(vdf_hash_queue_mixed *q, uint32_t *out);
void vdf_hash_queue_mixed_destroy(vdf_hash_queue_mixed *q);

/* ---- the app's Sorting::Distance key (vid_dup_finder_app/src/app/search_output.rs:43-60) ----------
 * out_max[g] = max hamming distance over all pairs of group g's contained paths: its members (indices
 * into hashes, n x 16, host) and, when ref_hashes and groups->ref_index are given and ref_index[g] >= 0,
 * the group's reference ref_hashes[ref_index[g]].  Every group has >= 2 contained paths in the reference. */
int vdf_groups_max_distance(vdf_ctx *ctx, const uint64_t *hashes, size_t n, const uint64_t *ref_hashes, size_t n_ref,
                            const vdf_groups *groups, uint32_t *out_max);

/* ---- the app's on-disk hash cache <-> SoA (host only) ---------------------------------------------
 * Format: bincode 2 `config::standard()` (little endian, varint) of
 * HashMap<PathBuf, MtimeCacheEntry { cache_mtime: SystemTime, value: Result<VideoHash, Error> }>
 * (vid_dup_finder_app/src/video_hash_filesystem_cache/generic_filesystem_cache/base_fs_cache.rs:26,
 * 106-118,192-204; processing_fs_cache.rs:23-27; generic_cache_if.rs:23; video_hash.rs:26-32).
 * Decoding yields the arrays the search ABI takes; entries whose value is Err(..) are counted, not
 * returned.  Entry order is the file's (a HashMap's: arbitrary); sort before searching. */
typedef struct vdf_cache_soa {
    uint64_t n_entries;      /* map length */
    uint64_t n_ok;           /* entries with Ok(VideoHash): length of the arrays below */
    uint64_t n_err;          /* entries with Err(..) */
    uint64_t n_key_differs;  /* Ok entries whose map key != VideoHash.src_path (0 for caches the app wrote) */
    uint64_t *hashes;        /* n_ok x 16 */
    uint32_t *durations;     /* n_ok */
    uint64_t *path_offsets;  /* n_ok + 1 byte offsets into paths (VideoHash.src_path, UTF-8, not NUL terminated) */
    char *paths;
    uint64_t *mtime_secs;    /* n_ok: cache_mtime.secs_since_epoch */
    uint32_t *mtime_nanos;   /* n_ok */
} vdf_cache_soa;
int vdf_cache_decode(const uint8_t *data, size_t len, vdf_cache_soa *out); /* malformed input -> VDF_E_INVAL */
/* The same on n_threads host threads (0 = one per 8 MB of file, at most 32 and at most the machine's; what vdf_cache_decode does).
 * bincode has no entry index, so the file is cut where the byte pattern of an Ok entry's hash words resynchronises, every range
 * is parsed by its own thread, and the ranges must meet exactly: if they do not, the file is decoded front to back instead - the
 * result never depends on the speculation.  Measured (profiles/r05_cache_ingest.txt, the GPU box: 256 hardware threads under a 16-CPU cgroup quota): 10 M entries
 * (2.69 GB) in 35 ms with the automatic thread count, 0.42 s on one thread.  The output arrays ask for transparent huge pages. */
int vdf_cache_decode_mt(const uint8_t *data, size_t len, int n_threads, vdf_cache_soa *out);
unsigned long long vdf_cache_decode_fallbacks(void); /* diagnostics: how often this process fell back to the front-to-back decode */
void vdf_cache_free(vdf_cache_soa *c);
/* Writes a cache the app can load: every entry Ok(VideoHash), key = src_path.  mtime arrays may be NULL (0).
 * *out_data is library-allocated; release with vdf_buffer_free(). */
int vdf_cache_encode(uint64_t n, const uint64_t *hashes, const uint32_t *durations, const uint64_t *path_offsets,
                     const char *paths, const uint64_t *mtime_secs, const uint32_t *mtime_nanos, uint8_t **out_data,
                     size_t *out_len);
void vdf_buffer_free(void *p);

/* ---- the cache's metadata sidecar (host only) ---------------------------------------------------------
 * Next to its cache file <dir>/<stem>.<ext> the app keeps <dir>/<stem>.metadata.txt holding
 * "{operating_system:?},{decode_backend:?},{crop:?},{skip_forward_amount},{cache_version}"
 * (vid_dup_finder_app/src/video_hash_filesystem_cache/cache_metadata.rs:45-51,80-89; video_hash_filesystem_cache.rs:76-139).
 * A cache file WITHOUT its sidecar makes the app exit (video_hash_filesystem_cache.rs:113-117), and a sidecar whose fields differ
 * from the run's options refuses the cache (:127-137) - the crop field is what keeps Cropdetect::None hashes and Letterbox hashes
 * of the same files apart.  Writers of a cache for the app: vdf_cache_encode + vdf_cache_metadata_new / _format / _path.
 * Readers of an app-written cache: vdf_cache_metadata_parse + _validate before the entries are mixed with this engine's hashes. */
enum { VDF_CACHE_OS_WINDOWS = 0, VDF_CACHE_OS_UNIX = 1 };               /* cache_metadata.rs:6-10 */
enum { VDF_CACHE_BACKEND_FFMPEG = 0, VDF_CACHE_BACKEND_GSTREAMER = 1 }; /* cache_metadata.rs:25-29 */
enum { VDF_CROPDETECT_NONE = 0, VDF_CROPDETECT_LETTERBOX = 1, VDF_CROPDETECT_MOTION = 2 }; /* vid_dup_finder_lib/src/definitions.rs:46-54 */
typedef struct vdf_cache_metadata {
    int32_t operating_system;
    int32_t decode_backend;
    int32_t crop;
    int32_t reserved;
    double skip_forward_amount;
    uint64_t cache_version;
} vdf_cache_metadata;
/* VdfCacheMetadata::new (cache_metadata.rs:54-78) as this library's target sees it: Unix, FfmpegBackend (the app's default
 * features), cache_version 1. */
int vdf_cache_metadata_new(int32_t crop, double skip_forward_amount, vdf_cache_metadata *out);
/* to_disk_fmt (:80-89).  *out_len = the text's length (no NUL counted; one is appended when it fits); cap too small -> VDF_E_OVERFLOW. */
int vdf_cache_metadata_format(const vdf_cache_metadata *m, char *buf, size_t cap, size_t *out_len);
/* try_parse (:91-125): exactly five comma-separated fields; operating system and backend are trimmed and lower-cased, crop is the
 * exact variant name, the numbers are Rust's str::parse (no white space).  VDF_E_INVAL with the app's message in err (nullable). */
int vdf_cache_metadata_parse(const char *text, size_t len, vdf_cache_metadata *out, char *err, size_t err_cap);
/* validate (:127-168) against new(exp_crop, exp_skip_forward_amount): VDF_OK, or VDF_E_INVAL with the first mismatch in err. */
int vdf_cache_metadata_validate(const vdf_cache_metadata *act, int32_t exp_crop, double exp_skip_forward_amount, char *err, size_t err_cap);
/* The sidecar's path for a cache path: file_stem() + ".metadata.txt" in the same directory (video_hash_filesystem_cache.rs:93-104).
 * A path without a file name ("..", "/") -> VDF_E_INVAL (the app reports EINVAL there). */
int vdf_cache_metadata_path(const char *cache_path, size_t len, char *buf, size_t cap, size_t *out_len);

/* ---- Search::sort's path order for a whole cache (host only) ------------------------------------------
 * Search::sort keys on (duration, src_path) and PathBuf orders by COMPONENTS (search_algorithm.rs:55-61; std::path::Path::cmp):
 * [RootDir | CurDir], then one Normal component per non-empty piece between '/', inner "." skipped, ".." = ParentDir;
 * RootDir < CurDir < ParentDir < Normal(bytes), a component-wise prefix sorts first.  "a/b" < "a.b", "a//b" == "a/b".
 * vdf_path_compare: -1 / 0 / +1.  vdf_path_ranks: out_rank[i] = number of distinct paths that sort before path i (equal paths
 * share a rank) for the n paths paths[path_offsets[i] .. path_offsets[i + 1]) - the layout of vdf_cache_soa - on n_threads host
 * threads (0 = all); what vdf_sort_order_device takes as d_path_rank.  No per-entry allocation. */
int vdf_path_compare(const char *a, size_t len_a, const char *b, size_t len_b);
int vdf_path_ranks(const char *paths, const uint64_t *path_offsets, size_t n, uint32_t *out_rank, int n_threads);

/* Search::sort's order itself (search_algorithm.rs:55-61) for n entries given as HOST arrays: out_order[k] = index of the entry at
 * position k of the stable order by (duration, PathBuf order of the path).  For plain paths (no empty, "." or ".." component, no NUL:
 * what a directory walk produces) of at most 1024 bytes the path half runs on the device - an LSD radix sort over 8-byte words of the
 * paths - otherwise through vdf_path_ranks on the host; *used_device (nullable) says which.  Same order either way. */
int vdf_sort_order_paths(vdf_ctx *ctx, const uint32_t *durations, const uint64_t *path_offsets, const char *paths, size_t n,
                         uint32_t *out_order, int *used_device);

/* ---- from the entries of a decoded cache to MatchGroups in one call -----------------------------------
 * What the app does between loading its cache and printing groups (vid_dup_finder_app/src/app/app_fns.rs:428-482: fetch the
 * hashes of the --files paths and of the --with-refs paths, then search() or search_with_references()), on the SoA arrays of
 * vdf_cache_decode, with no per-entry host object: upload -> Search::sort on the device (paths included when they are plain:
 * vdf_sort_order_paths; else PathBuf ranks from vdf_path_ranks + vdf_sort_order_device) -> gather -> search.
 * cand_idx (nullable = all n entries, n_cand ignored) and ref_idx select entries of the arrays; n_ref == 0 -> search(), else
 * search_with_references() with the references in ref_idx order.  Group members (and ref_index) are indices into the caller's
 * arrays (NOT into cand_idx / ref_idx), in the reference's order.  timing (nullable) receives the phases. */
typedef struct vdf_cache_search_timing {
    float rank_ms;    /* durations, path blob and offsets to the device + the plain-path check (host route: + vdf_path_ranks) */
    float upload_ms;  /* host wall: hashes, durations, ranks to the device(s) */
    float sort_ms;    /* device + host wall: Search::sort order, gather, order download */
    float search_ms;  /* the search call proper (vdf_ctx_last_search_timing has its phases) */
    float map_ms;     /* host: group members back to the caller's indices */
    float total_ms;
} vdf_cache_search_timing;
int vdf_search_cache_entries(vdf_ctx *ctx, const uint64_t *hashes, const uint32_t *durations, const uint64_t *path_offsets,
                             const char *paths, size_t n, const uint64_t *cand_idx, size_t n_cand, const uint64_t *ref_idx,
                             size_t n_ref, uint32_t tol_int, vdf_groups *out, vdf_cache_search_timing *timing);

#ifdef __cplusplus
}
#endif
#endif /* VDF_H */
