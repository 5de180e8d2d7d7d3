// Which linear-stream resize kernel a frame size gets and with what geometry (LDS row pitch, 16-row blocks per chunk).
// Host-only arithmetic (no HIP), shared by the launchers in dct_hash.hip and by api.cpp; tests/cpp/resize_dispatch_main.cpp
// checks the LDS budgets and the pitch rules for every width on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

#include "resize_tables.h"

namespace vdf {

// LDS budgets of the linear-stream kernels.  Chunk form (resize_mfma_frame_stream_kernel, frames up to 512 wide): S = two workgroups
// per CU, 64-row chunks, whole table.  The M sizes (one workgroup per CU, 32 KB of table, two 62 KB chunk buffers; the band form
// of the table for crops wider than 1024: 16 outputs x at most 15 tiles x 128 B + padding) serve the general cropped kernel only -
// uncropped M-class frames take the per-wave form.  The K-split kernel keeps its table in registers: two 75 KB buffers.
// + 128: the operand reads' overrun past the last row.
constexpr int kStreamBufS = 30 * 1024 + 128, kStreamTabS = 8;
constexpr int kStreamBufM = 62 * 1024 + 128, kStreamTabM = 16;
constexpr int kKsplitBuf = 75 * 1024 + 128;
constexpr int kWaveStreamBuf = 16 * 1920 + 128;  // one 16-row block of a frame up to 1920 wide per wave (round 3: resize_mfma_frame_wavestream_kernel)
constexpr int kWaveStreamTabBytes = 16 * (kMfmaBandMaxTiles * 128 + 32) + 128;  // band table + zero slot
// narrower frames: more waves, each with its own (smaller) block buffer, so that the blocks in flight per CU stay near 120 KB.
// A block's DMA instructions fill whole KBs: the buffers are the block rounded up to 1 KB (+ the operand reads' overrun).
constexpr int kWaveStreamBuf5 = 25 * 1024 + 128, kWaveStreamBuf6 = 21 * 1024 + 128, kWaveStreamBuf8 = 15 * 1024 + 128;  // pitches up to 1600, 1344, 960
constexpr int kWaveStreamBuf3 = 37 * 1024 + 128;  // ... and wider frames (pitches up to 2368: 2048 x 1152, 2160 x 3840 portrait) with three waves
constexpr int kWaveStreamTabMid = 16 * (12 * 128 + 32) + 128;    // band tables of at most 12 tiles per output (five waves: frames up to 1600 columns)
constexpr int kWaveStreamTabSmall = 16 * (10 * 128 + 32) + 128;  // at most 10 (six and eight waves: up to 1344 columns)
constexpr int kStreamPartBytes = 3 * 64 * 4 * 4;  // s_part: the vertical partial sums of waves 1..3
constexpr int kLdsPerCu = 160 * 1024;
static_assert(16 * (kMfmaBandMaxTiles * 128 + 32) + 128 <= kStreamTabM * 2048, "band table + zero slot fit the M class");
static_assert(2 * (2 * kStreamBufS + kStreamTabS * 2048 + kStreamPartBytes) <= kLdsPerCu, "two S workgroups per CU");
static_assert(2 * kStreamBufM + kStreamTabM * 2048 + kStreamPartBytes <= kLdsPerCu, "one M workgroup per CU");
static_assert(2 * kKsplitBuf + 2 * 3 * 64 * 16 + kStreamPartBytes <= kLdsPerCu, "one K-split workgroup per CU");
static_assert(4 * kWaveStreamBuf + kWaveStreamTabBytes + 2 * kStreamPartBytes <= kLdsPerCu, "one per-wave-stream workgroup per CU");
static_assert(3 * kWaveStreamBuf3 + kWaveStreamTabBytes + 2 * 2 * 1024 <= kLdsPerCu, "three waves");
static_assert(5 * kWaveStreamBuf5 + kWaveStreamTabMid + 2 * 4 * 1024 <= kLdsPerCu, "five waves");
static_assert(6 * kWaveStreamBuf6 + kWaveStreamTabSmall + 2 * 5 * 1024 <= kLdsPerCu, "six waves");
static_assert(8 * kWaveStreamBuf8 + kWaveStreamTabSmall + 2 * 7 * 1024 <= kLdsPerCu, "eight waves");

// LDS row pitch of the stream kernel: the frame's own for multiples of 16 - unless it is a multiple of 256, where the 16
// rows of a block would share one bank group (16-way conflict on every operand read: re-pitched, 768 / 1024 / 1280 wide
// gain 12 / 10 / 6 %; pitches with 8-way conflicts or fewer - 1920, 640, 480 - are faster left alone: the linear DMA is
// worth more than the conflicts cost); otherwise the next odd multiple of 16 that holds the row and the up to 3 bytes a
// dword-aligned row start puts in front of it.
uint32_t stream_pitch(uint32_t w);
// 16-row blocks per chunk (at most 4) that fit a buffer at that pitch; 0 = not even one
uint32_t stream_blocks_per_chunk(uint32_t wp, int buf_bytes);
// buffer class of a width: 0 none, 1 = S (the chunk kernel), 2 = M, 3 = M with the band table; *nb = 16-row blocks per chunk
int stream_class(uint32_t w, uint32_t *nb);
bool resize_stream_wants_band(uint32_t w, int knob = 0);  // the width's kernel takes a.bh in kMfmaLayoutHorizontalBand form (= the per-wave form)
// One block stream per wave (resize_mfma_frame_wavestream_kernel): every M-class width whose (re-pitched, whole-KB) block fits a wave's
// buffer - 512 .. 2368 columns - with as many waves per workgroup as buffers fit (8 / 6 / 5 / 4 / 3; 0 = the width does not take this form).
// knob (vdf_ctx::wavestream_knob, read once per context): 0 = the measured rule, n > 0 = VDF_WAVESTREAM_NW=n forces n waves where the block
// fits the n-wave buffer, -1 = VDF_NO_WAVESTREAM=1 switches the form off (measurements / tests).
int resize_wavestream_waves(uint32_t w, int knob = 0);
bool resize_wavestream_applies(uint32_t w, int knob = 0);
// a launch over crop boxes that share their column range (x0, box_w) of frames frame_w wide: LDS row pitch and addressing mode (0 linear
// copy of whole rows, 1 gather, 2 gather + the operand shift for rows that start off a dword), and the wave count (0: not this kernel)
uint32_t box_stream_pitch(uint32_t frame_w, uint32_t x0, uint32_t box_w, int *mode);
int resize_wavestream_waves_box(uint32_t frame_w, uint32_t x0, uint32_t box_w, int knob = 0);
constexpr int wavestream_buf_bytes(int nw) { return nw == 3 ? kWaveStreamBuf3 : nw == 4 ? kWaveStreamBuf : nw == 5 ? kWaveStreamBuf5 : nw == 6 ? kWaveStreamBuf6 : nw == 8 ? kWaveStreamBuf8 : 0; }
bool resize_wavestream_table_fits(int nw, int band_stride);  // does a band table of that stride (bytes per output) fit the nw-wave kernel's table array
// Clips whose crop boxes are full-width (top / bottom bars only): do the ROWCROP instantiations of the stream kernels beat the general
// cropped kernels at this frame width?  (measured; the frame must also pass resize_stream_eligible / resize_ksplit_eligible)
bool resize_rowcrop_streams(uint32_t w);
// Does a call take a linear-stream kernel (chunk or per-wave form)?  Frames starting on 16-byte boundaries and ending on one, rows packed
// inside a frame (frames and clips may be padded), 64 .. 1920 columns.
bool resize_stream_eligible(const uint8_t *frames, uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride, int knob = 0);
// frames of at most 128 rows (the fused kernel's range) that measured faster on the stream kernels: wide, short ones
bool resize_short_prefers_stream(uint32_t w, uint32_t h);
// narrow frames of 129 ... 256 rows that measured faster on the tiled persistent kernel (the fused family) than on the stream kernels
bool resize_tall_prefers_tiled(uint32_t w, uint32_t h);

// K-split form (1024..4096 columns, a multiple of 16): LDS pitch (an odd multiple of 16) and blocks per chunk (0: does not fit)
uint32_t ksplit_geometry(uint32_t w, uint32_t *wp);
bool resize_ksplit_eligible(const uint8_t *frames, uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride);

// cropped clips: can frames of this pitch take the stream form and with which buffers (1 = S, 2 = M); per crop box the LDS
// pitch and the blocks per chunk (a full-width box at a pitch without 16-way conflicts keeps the frame's pitch: linear DMA)
bool resize_cropped_stream_class(uint32_t pitch, int *cls);
uint32_t resize_cropped_stream_blocks(uint32_t crop_w, uint32_t x0, uint32_t pitch, int cls, uint32_t *wp);

// ---- The planner: which kernel hashes a call.  Pure host arithmetic over the call and the context's knobs; api.cpp
// fetches the tables a plan names and switches on its route, the launchers of dct_hash.hip switch on its values.  tests/cpp/resize_dispatch_main.cpp
// enumerates it: every route's preconditions hold for every width, and the documented sizes land on the documented kernels.
struct HashKnobs {  // copied from vdf_ctx (vdf_ctx.h says which VDF_* variable sets each)
    int resize_mode = 0, wavestream_knob = 0;
    bool hash_no_persistent = false, no_rowcrop = false, rowcrop_all = false, no_boxstream = false, no_smallcrop = false, lb_host_plan = false,
         no_lb_fused = false;
};
struct HashCall {
    const uint8_t *base;  // for its alignment only
    uint32_t w, h;
    size_t frame_stride, clip_stride, n_clips;
};
// one value per row of DESIGN.md 4.1; kRefused: a forced mode whose tables do not fit the i8 split (VDF_E_BAD_DIMS)
enum class HashRoute { kRefused, kDirect16, kPersistentOneTile, kTiled, kPerClipFused, kChunkStream, kWaveStream, kKsplit, kWholeLine, kScalar };
// What a plan cannot know before the tables are built; the caller plans again with what it found.
enum class TableFit { kAll, kNoBand /* the width's band table does not fit */, kNoPlain /* a plain table does not fit the i8 split */ };
struct HashPlan {
    HashRoute route = HashRoute::kRefused;
    int layout_h = kMfmaLayoutHorizontal, layout_v = kMfmaLayoutVertical;  // the MFMA tables to fetch (none: kDirect16, kScalar, kRefused)
    int n_kt = 0, n_rg = 0;        // 64-column / 64-row tiles of the frame
    int tiled_nrg = 0, waves = 0;  // kTiled: the <NKT = n_kt, NRG, WAVES> instantiation; kWaveStream: waves per workgroup
    uint32_t nb = 0;               // kChunkStream / kKsplit: 16-row blocks per chunk
    bool full_tile = false;        // kPersistentOneTile: exactly 64 x 64 (the <FULL> instantiation)
    bool last_clip_apart = false;  // the persistent kernels: the last clip goes through the per-clip kernel and its careful loader
};
HashPlan plan_hash(const HashCall &c, const HashKnobs &k, TableFit fit = TableFit::kAll);
// The resize stage alone (the windows calls, DESIGN.md 4.9: the DCT is a kernel of its own there): plan_hash's route where that route writes
// the 16 x 16 frames to memory - chunk stream, wave stream, K-split, whole-line, scalar - and, where plan_hash names a kernel with the DCT
// fused in (or the 16 x 16 copy), the whole-line kernel; the scalar kernel where the whole-line tables do not fit the i8 split (kNoPlain).
// Never a fused route, never kDirect16; kRefused only as plan_hash refuses (a forced mode of the caller's whose tables do not fit).
HashPlan plan_resize_only(const HashCall &c, const HashKnobs &k, TableFit fit = TableFit::kAll);

// resize_dct_hash_tiled_kernel<NKT, NRG, WAVES>: WAVES (the second __launch_bounds__ argument) by [NKT - 1][NRG = 1, 2, 4]; measured
// (profiles/r05_short_frames.txt).  0: no such instantiation (one tile is the persistent kernel's).
constexpr int kTiledWaves[4][3] = {{0, 1, 3}, {1, 3, 2}, {3, 3, 3}, {2, 2, 2}};
constexpr int tiled_waves(int nkt, int nrg) { return kTiledWaves[nkt - 1][nrg == 4 ? 2 : nrg - 1]; }

// Cropped calls (crops: HOST array [n_clips][4] = left, right, top, bottom, not all zero).  Small frames take one kernel; otherwise every clip
// goes to exactly one part: full-width boxes on a ROWCROP launch, side-bar boxes that share a column range on per-wave box launches, the rest
// on one general kernel (the gather stream kernel or the whole-line cropped kernel).
struct CropTableFit {  // what building the tables showed; the caller plans again with each fact it finds
    bool rows_table = true;     // the frame width's horizontal table in the ROWCROP launch's layout fits
    bool height_tables = true;  // every box height's vertical table fits (false: the whole call through one general kernel)
    bool gather_tables = true;  // the tables of the rest's boxes fit the gather stream kernel
    std::vector<uint64_t> ranges_without_table;  // crop_range_key of the column ranges whose band table does not fit (the i8 split, or that wave count's array)
};
constexpr uint64_t crop_range_key(uint32_t x0, uint32_t box_w) { return ((uint64_t)x0 << 32) | box_w; }
struct CropBoxGroup { uint32_t x0, box_w; int waves; std::vector<uint32_t> ids; };
constexpr size_t kMaxCropBoxGroups = 16, kMinCropBoxGroupClips = 4;
struct CropPlan {
    enum Kind { kBadBox /* a box leaves no pixels */, kSmall /* resize_dct_hash_cropped_small_kernel */, kParts } kind = kParts;
    HashPlan rows_kernel;              // the ROWCROP launch: kChunkStream, kWaveStream or kKsplit; kRefused = none
    std::vector<uint32_t> rows;        // its clips
    std::vector<CropBoxGroup> groups;  // per-wave box launches, one per column range
    std::vector<uint32_t> rest;        // the general kernel's clips
    bool rest_gather = false;          // resize_mfma_cropped_stream_kernel, else resize_mfma_cropped_kernel
    int gather_cls = 0;                // its buffer class (resize_cropped_stream_class)
    bool gather_shift = false;         // some row of some box of the rest starts off a dword boundary
};
CropPlan plan_cropped(const HashCall &c, const HashKnobs &k, const uint32_t *crops, const CropTableFit &fit = CropTableFit());

// The letterbox entry: small frames keep their boxes on the device; everything else detects, copies the boxes down and takes plan_cropped.
struct LetterboxPlan {
    bool small_frames;   // (needs the frame size's BoxTableSet to be usable, else the host route)
    bool one_tile;       // ... of at most 64 x 64: the fused detect + hash kernel for all but the last n_tail clips
    size_t n_tail;       // clips within 64 bytes of the buffer's end: the device-box route and its careful loader
};
LetterboxPlan plan_letterbox(const HashCall &c, const HashKnobs &k);

// ---- Clips of different frame sizes in one call (vdf_hash_clips_u8[_device]; DESIGN.md 4.1 "mixed sizes") ----------------------------------
// All clips live in ONE buffer of buf_bytes bytes and name their place by offset, so the loaders' one rule - loads may run past a row into
// the rest of the buffer, only the buffer's end takes the careful loader - holds unchanged, and every address is checked here, on the host,
// before anything is queued.  tests/cpp/mixed_plan_main.cpp walks every descriptor's address envelope on the CPU.
constexpr size_t kMaxClipsPerLaunch = 256 * 1024;  // x 16 frames x 256 threads stays under HIP's 2^32 work-item grid limit
struct MixedClip {  // = vdf_clip (include/vdf.h; api.cpp asserts the layout)
    uint64_t offset, frame_stride;
    uint32_t w, h;
    uint32_t crop[4];  // left, right, top, bottom
};
// What the mixed kernels read per clip.  h_table / v_table: the planner leaves the BOX sizes (bw, bh) there; the caller replaces them by the
// entries of the tables it uploads (api.cpp: hash_mixed_launch).
struct MixedClipDesc {
    uint64_t offset;        // first byte of frame 0, relative to the buffer
    uint64_t frame_stride;  // bytes between frames
    uint32_t x0, y0, bw, bh;
    uint32_t h_table, v_table;
    uint32_t out_index;     // the clip's position in the caller's array: where its hash goes (a launch covers a subset of the call)
    uint32_t pitch;         // bytes between rows = the frame's width
};
static_assert(sizeof(MixedClipDesc) == 48 && sizeof(MixedClipDesc) % 16 == 0, "descriptors are read as whole 16-byte pieces");
static_assert(offsetof(MixedClipDesc, offset) == 0 && offsetof(MixedClipDesc, frame_stride) == 8 && offsetof(MixedClipDesc, x0) == 16 &&
              offsetof(MixedClipDesc, y0) == 20 && offsetof(MixedClipDesc, bw) == 24 && offsetof(MixedClipDesc, bh) == 28 &&
              offsetof(MixedClipDesc, h_table) == 32 && offsetof(MixedClipDesc, v_table) == 36 && offsetof(MixedClipDesc, out_index) == 40 &&
              offsetof(MixedClipDesc, pitch) == 44, "MixedClipDesc layout");
static_assert(sizeof(MixedClip) == 40, "vdf_clip layout");

// The argument checks, in the order their codes are reported (as checked_launches): over ALL clips before anything is queued.
enum class MixedError { kNone, kNotEnoughFrames, kZeroDim, kStrideBelowFrame, kEmptyBox, kOutOfBuffer, kCropGiven /* the letterbox calls only: plan_letterbox_mixed */ };
struct MixedCheck { MixedError error = MixedError::kNone; size_t clip = 0; };
MixedCheck check_mixed(const MixedClip *clips, size_t n, uint32_t frames_per_clip, uint64_t buf_bytes);

// Which kernel reads a clip, by its FRAME size (the rules of plan_cropped): small = one workgroup per clip with the DCT fused
// (resize_dct_hash_mixed_small_kernel), lines / wide lines = one workgroup per frame (resize_mfma_mixed_kernel<false / true>, the latter
// with the vertical table in kMfmaLayoutVerticalWide order).
enum class MixedPart { kSmall, kLines, kWideLines };
MixedPart mixed_part_of(uint32_t w, uint32_t h, const HashKnobs &k);
constexpr uint32_t mixed_loader_overrun(MixedPart p) { return p == MixedPart::kWideLines ? 128u : 64u; }  // the careful-loader tests' margin
// The kernels' own careful-loader expression for frame f of a descriptor, in offsets: true = that frame takes the careful loader.
// (dct_hash.hip: src + bh * pitch + overrun > buf_end with src = buf + offset + f * frame_stride + y0 * pitch + x0)
inline bool mixed_frame_is_careful(const MixedClipDesc &d, MixedPart p, uint32_t f, uint64_t buf_bytes)
{
    return d.offset + (uint64_t)f * d.frame_stride + (uint64_t)d.y0 * d.pitch + d.x0 + (uint64_t)d.bh * d.pitch + mixed_loader_overrun(p) > buf_bytes;
}
struct MixedLaunch { MixedPart part; size_t first, count; };  // descs[first .. first + count)
struct MixedPlan {
    enum Kind { kUniform, kMixed } kind = kMixed;
    // kUniform: one frame size, one frame stride, offsets in arithmetic progression: today's hash_launch / hash_cropped_launch on
    // (base + offset0, clip_stride) - the same kernels, words and speed
    uint64_t offset0 = 0, clip_stride = 0;
    bool cropped = false;  // some clip has a box
    // kMixed: descriptors part by part (small, lines, wide lines), each part cut into launches of at most kMaxClipsPerLaunch clips
    std::vector<MixedClipDesc> descs;
    std::vector<MixedLaunch> launches;
    size_t n_small = 0;           // descs[n_small ..): the clips whose 16 x 16 frames go through ctx->small, slot = index - n_small
    uint32_t max_w = 0, max_h = 0;  // the largest box sizes: what the table index is sized by
};
// clips have passed check_mixed; n <= 2^32 - 1 (out_index is 32 bits)
MixedPlan plan_mixed(const MixedClip *clips, size_t n, const HashKnobs &k);

// ---- Letterbox detection on clips of different frame sizes (vdf_cropdetect_letterbox_clips_device, vdf_hash_clips_u8_letterbox[_device]) -------
// What the mixed detect kernels (cropdetect.hip: cropdetect_mixed_kernel, cropdetect_sides_mixed_kernel) read per CLIP: both probed frames
// (0 and 8) of a clip share one descriptor.  Probe p's frame starts at buf + offset + 8 p frame_stride; its rows are w bytes apart.
struct LetterboxProbeDesc {
    uint64_t offset;        // first byte of frame 0, relative to the buffer
    uint64_t frame_stride;  // bytes between frames
    uint32_t w, h;
    uint32_t slot;          // the clip's position in the caller's array: its box is crops[4 slot ..]
    uint32_t reserved;      // 0
};
static_assert(sizeof(LetterboxProbeDesc) == 32 && sizeof(LetterboxProbeDesc) % 16 == 0, "descriptors are read as whole 16-byte pieces");
static_assert(offsetof(LetterboxProbeDesc, offset) == 0 && offsetof(LetterboxProbeDesc, frame_stride) == 8 && offsetof(LetterboxProbeDesc, w) == 16 &&
              offsetof(LetterboxProbeDesc, h) == 20 && offsetof(LetterboxProbeDesc, slot) == 24 && offsetof(LetterboxProbeDesc, reserved) == 28,
              "LetterboxProbeDesc layout");
constexpr uint32_t kLetterboxProbes = 2;      // frames 0 and 8: the mixed call requires 16 frames per clip
constexpr uint32_t kLetterboxWorkLists = 64;  // pass 1 appends frame i to sub-list i % 64 of its launch's work list
// bytes of one work list for `frames` probed frames: 64 counters, then 64 sub-lists of cap = ceil(frames / 64) entries of four words
constexpr size_t letterbox_work_list_bytes(size_t frames)
{
    return (kLetterboxWorkLists + 4 * kLetterboxWorkLists * ((frames + kLetterboxWorkLists - 1) / kLetterboxWorkLists)) * sizeof(uint32_t);
}
// the column batch of pass 2 by frame height, as launch_letterbox chooses it (speed only: the crops are exact for every batch)
constexpr int letterbox_column_batch(uint32_t h) { return h >= 512 ? 32 : h >= 256 ? 16 : 8; }
struct LetterboxMixedLaunch {
    int column_batch;     // 8, 16 or 32: the cropdetect_sides_mixed_kernel instantiation
    size_t first, count;  // descs[first .. first + count): 2 count workgroups in pass 1
    size_t work_offset;   // bytes from the start of the work buffer to this launch's own work list
};
struct LetterboxMixedPlan {
    enum Kind { kUniform, kMixed, kCropGiven /* a clip came with a crop box: VDF_E_INVAL */ } kind = kMixed;
    size_t bad_clip = 0;  // kCropGiven: the first such clip
    // kUniform: one frame size, one frame stride, offsets one positive step apart: today's uniform letterbox route on (base + offset0, clip_stride)
    uint64_t offset0 = 0, clip_stride = 0;
    // kMixed: one descriptor per clip, class by class (column batch 8, 16, 32), each class cut into launches of at most kMaxClipsPerLaunch clips;
    // every launch has its own work list, so no frame is walked by two classes
    std::vector<LetterboxProbeDesc> descs;
    std::vector<LetterboxMixedLaunch> launches;
    size_t work_bytes = 0;  // all work lists
};
// clips have passed check_mixed; n <= 2^32 - 1.  The letterbox calls take the whole frame as the reference does: a caller-supplied crop box is
// refused (MixedError::kCropGiven), after every error of check_mixed.
LetterboxMixedPlan plan_letterbox_mixed(const MixedClip *clips, size_t n, const HashKnobs &k);

}  // namespace vdf
