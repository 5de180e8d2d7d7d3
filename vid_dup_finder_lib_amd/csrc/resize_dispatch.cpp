#include "resize_dispatch.h"

#include <algorithm>
#include <map>

namespace vdf {

uint32_t stream_pitch(uint32_t w)
{
#ifdef VDF_STREAM_REPITCH_ALL  // experiment: every line-aligned pitch from 640 columns up is re-pitched to an odd multiple of 16 bytes
    if (w % 16 == 0) return ((w % 256 == 0 && w >= 768) || (w % 128 == 0 && w >= 640 && (w / 16) % 2 == 0)) ? w + 16 : w;
#else
    if (w % 16 == 0) return (w % 256 == 0 && w >= 768) ? w + 16 : w;
#endif
    uint32_t wp = (w + (w % 4 ? 3u : 0u) + 15u) & ~15u;
    if ((wp / 16) % 2 == 0) wp += 16;
    return wp;
}

uint32_t stream_blocks_per_chunk(uint32_t wp, int buf_bytes)
{
    for (uint32_t nb = 4; nb >= 1; nb--)
        if ((size_t)((16u * nb * wp + 1023u) & ~1023u) + 128u <= (size_t)buf_bytes) return nb;  // a DMA instruction fills whole KBs
    return 0;
}

int stream_class(uint32_t w, uint32_t *nb)
{
    const int n_kt = (int)((w + 63) / 64);
    const uint32_t wp = stream_pitch(w);
    if (n_kt <= kStreamTabS && stream_blocks_per_chunk(wp, kStreamBufS) == 4) { *nb = 4; return 1; }
    *nb = stream_blocks_per_chunk(wp, kStreamBufM);
    if (n_kt <= kStreamTabM) return *nb >= 2 ? 2 : 0;
    return *nb >= 2 ? 3 : 0;
}

static bool wavestream_fits(uint32_t w, int nw)
{
    const uint32_t need = ((16u * stream_pitch(w) + 1023u) & ~1023u) + 128u;  // a DMA instruction fills whole KBs
    return need <= (uint32_t)wavestream_buf_bytes(nw) && w >= 256;
}

int resize_wavestream_waves(uint32_t w, int knob)
{
    if (knob < 0) return 0;  // VDF_NO_WAVESTREAM (measurements / tests): the chunk kernel everywhere
    if (knob > 0) return wavestream_fits(w, knob) ? knob : 0;  // VDF_WAVESTREAM_NW
    uint32_t nb = 0;
    const int cls = stream_class(w, &nb);
    // Frames up to 512 wide keep the chunk kernel (two workgroups per CU, whole table in LDS: 480 x 270 6.5 TB/s against 6.0 with eight
    // waves).  From there on one block stream per wave, with as many waves as block buffers fit: measured against the chunk kernel
    // (gpurun_out/r03_nw_sweep2.txt) 576 wide 5.9 -> 6.8 TB/s, 640 6.4 -> 6.8, 1152 5.3 -> 6.8, 1200 6.1 -> 6.7, 1366 5.4 -> 6.3,
    // 1440 5.6 -> 6.3, 1520 6.0 -> 6.8; level at 896 / 960.  (With FOUR waves the three-block widths had measured slower: 1280 x 720
    // 6.6 -> 5.8 - the point is the bytes in flight per CU, not the absence of the barrier.)
    if (cls == 1) return 0;
    for (int nw : {8, 6, 5, 4})
        if (cls >= 2 && wavestream_fits(w, nw)) return nw;
    // Wider than the four-wave buffers: three waves with 37 KB blocks (pitches up to 2368) - for the widths the K-split kernel cannot take
    // (not a multiple of 16: 1950 x 1096 3.2 -> 5.2 TB/s against the whole-line kernel).  Multiples of 16 stay with the K-split form,
    // which measured 2-4 % ahead of three waves (2048 wide 5.79 against 5.53, 2304 5.88 against 5.63; gpurun_out/r03nw3).
    if (w % 16 != 0 && wavestream_fits(w, 3)) return 3;
    return 0;
}

uint32_t box_stream_pitch(uint32_t frame_w, uint32_t x0, uint32_t box_w, int *mode)
{
    if (x0 == 0 && box_w == frame_w) {  // whole rows
        const uint32_t wp = stream_pitch(frame_w);
        *mode = wp == frame_w ? 0 : frame_w % 4 == 0 ? 1 : 2;
        return wp;
    }
    // a box: gathered row by row.  Rows of the box start at (row * frame_w + x0): off a dword unless both are multiples of 4, and then
    // the LDS row holds the up to 3 bytes in front of the box's first pixel too (MODE 2 shifts them out of the operands)
    const bool shifted = frame_w % 4 != 0 || x0 % 4 != 0;
    *mode = shifted ? 2 : 1;
    uint32_t wp = (box_w + (shifted ? 3u : 0u) + 15u) & ~15u;
    if ((wp / 16) % 2 == 0) wp += 16;  // an odd multiple of 16 bytes: the 16 rows of a block in 16 different bank groups
    return wp;
}

int resize_wavestream_waves_box(uint32_t frame_w, uint32_t x0, uint32_t box_w, int knob)
{
    if (x0 == 0 && box_w == frame_w) return resize_wavestream_waves(frame_w, knob);
    if (knob < 0 || box_w < 513) return 0;  // narrower boxes: the gather kernel with two workgroups per CU
    int mode = 0;
    const uint32_t need = ((16u * box_stream_pitch(frame_w, x0, box_w, &mode) + 1023u) & ~1023u) + 128u;
    for (int nw : {8, 6, 5, 4, 3})
        if (need <= (uint32_t)wavestream_buf_bytes(nw)) return nw;
    return 0;
}

bool resize_wavestream_table_fits(int nw, int band_stride)
{
    const int tab_bytes = 16 * band_stride + 128;  // + the zero slot
    return tab_bytes <= (nw <= 4 ? kWaveStreamTabBytes : nw == 5 ? kWaveStreamTabMid : kWaveStreamTabSmall);
}

bool resize_stream_wants_band(uint32_t w, int knob) { return resize_wavestream_waves(w, knob) != 0; }

bool resize_wavestream_applies(uint32_t w, int knob) { return resize_wavestream_waves(w, knob) != 0; }

bool resize_rowcrop_streams(uint32_t w)
{
    // Full-width crop boxes (top / bottom bars) through the ROWCROP stream kernels against the general cropped kernels, detect + crop +
    // hash of clips with 12 % bars (gpurun_out/r03v, r03w, r03y): 1600 wide 3.83 -> 2.87 ms, 1152 3.51 -> 3.12, 1280 4.39 -> 3.91,
    // 1366 1.73 -> 1.51, 3840 5.29 -> 4.65, 1920 4.76 -> 4.33, 1536 3.13 -> 2.90, 1024 2.80 -> 2.64, 640 / 768 / 854 -3 %, 2560 level;
    // 2048 wide (the K-split form with two-block chunks) lost 4 % to the whole-line cropped kernel and stays there.
    return w != 2048;
}

bool resize_stream_eligible(const uint8_t *frames, uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride, int knob)
{
    // narrow tall frames (portrait video) gain the most: 240 x 426 4.6 -> 6.1 TB/s, 160 x 200 3.5 -> 4.2 against the whole-line kernels
    if (w < 64 || (uint64_t)w * h >= (1ull << 31)) return false;
    // frames must also END on a 16-byte boundary: the buffer resource is sized to the frame and the range check drops a dword that
    // straddles its end (203 x 301 frames lost their last pixels: found by the strided-buffer test)
    if (((uint64_t)w * h) % 16 != 0) return false;
    if (((uintptr_t)frames | frame_stride | clip_stride) % 16 != 0) return false;
    uint32_t nb = 0;
    return stream_class(w, &nb) == 1 || resize_wavestream_applies(w, knob);  // the chunk form (frames up to 512 wide) or one block stream per wave
}

bool resize_short_prefers_stream(uint32_t w, uint32_t h)
{
    // Frames of at most 128 rows fuse resize and DCT in one kernel, one workgroup per clip (a frame at a time: 4 - 16 KB in flight per
    // workgroup).  That is the faster form for small frames only.  Measured against the linear-stream kernels + dct_hash_kernel, round 5
    // (TB/s of frame bytes, fused -> stream; gpurun_out/r05u, r05w = profiles/r05_short_frames.txt): 176 x 99 4.1 -> 4.1, 192 x 108 4.7 -> 4.8,
    // 160 x 120 4.4 -> 4.7, 200 x 112 3.7 -> 4.8, 208 x 117 3.6 -> 5.4, 224 x 126 3.9 -> 5.8, 256 x 128 4.8 -> 6.1, 320 x 96 4.5 -> 6.1,
    // 480 x 128 4.1 -> 6.4, 640 x 120 3.9 -> 5.8, 854 x 128 2.5 -> 5.7, 1920 x 128 3.5 -> 6.0, 1920 x 64 4.7 -> 6.0; the other way:
    // 128 x 128 4.8 -> 4.3, 160 x 90 4.2 -> 3.8, 192 x 80 4.3 -> 4.0, 128 x 96 4.6 -> 3.5, 512 x 64 4.8 -> 4.2 (one chunk per frame).
    // Later in round 5 frames of up to 256 x 128 with W % 16 == 0 got a persistent kernel of their own (resize_dct_hash_tiled_kernel), which moved
    // the line for those widths (tiled -> stream, gpurun_out/r06h against r05x): 160 x 120 5.3 -> 4.9, 192 x 108 5.6 -> 5.2, 192 x 128 5.7 -> 5.5,
    // 208 x 117 5.4 -> 5.4, 224 x 126 5.8 -> 6.3, 256 x 128 5.7 -> 6.5.
    if (h > 128) return false;  // (not asked: such frames never fuse)
    if (w > 512) return h >= 64;  // the per-wave form
    // (r06i, the same box for both: 192 x 128 5.7 -> 6.0, 208 x 117 5.5 -> 5.9, 240 x 100 5.4 -> 5.6, 256 x 96 6.0 -> 5.8: the line is at 24 000 pixels)
    if (w <= 256 && w % 16 == 0) return h > 64 && (uint64_t)w * h >= 24000;  // the tiled kernel's widths
    return h > 64 && (uint64_t)w * h >= 19000;
}

bool resize_tall_prefers_tiled(uint32_t w, uint32_t h)
{
    // Narrow frames of 129 ... 256 rows: the chunk-stream kernel moves 64 rows at a time whatever the width - 11 KB of a 176-wide frame, 4 KB of
    // a 64-wide one, two workgroups per CU: latency-bound.  The tiled persistent kernel (four row groups) keeps 16 KB per wave in flight.
    // Measured, stream -> tiled (TB/s, gpurun_out/r06l = profiles/r05_short_frames.txt): 64 x 160 2.4 -> 5.5, 64 x 256 2.7 -> 4.9, 80 x 240 3.1 -> 5.2,
    // 96 x 160 3.2 -> 5.1, 112 x 200 3.5 -> 5.4, 128 x 160 4.0 -> 5.4, 128 x 256 4.8 -> 5.4, 160 x 144 4.3 -> 4.9, 160 x 200 4.6 -> 5.0,
    // 176 x 144 4.6 -> 5.1; level at 144 x 256, 176 x 208, 192 x 144; the other way from there: 208 x 160 5.4 -> 5.0, 240 x 160 6.1 -> 5.0.
    // (any width since the persistent kernels take the last clip apart: 100 x 200 3.1 -> 4.7, gpurun_out/r06z)
    return h > 128 && h <= 256 && w >= 16 && w <= 176 && (uint64_t)w * h <= 36000;
}

uint32_t ksplit_geometry(uint32_t w, uint32_t *wp)
{
    uint32_t p = w;  // w % 16 == 0
    if ((p / 16) % 2 == 0) p += 16;
    *wp = p;
    return stream_blocks_per_chunk(p, kKsplitBuf);
}

bool resize_ksplit_eligible(const uint8_t *frames, uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride)
{
    if (w % 16 != 0 || w < 1024 || w > 4096 || (uint64_t)w * h >= (1ull << 31)) return false;
    if (((uintptr_t)frames | frame_stride | clip_stride) % 16 != 0) return false;
    uint32_t wp = 0;
    return ksplit_geometry(w, &wp) >= 1;
}

bool resize_cropped_stream_class(uint32_t pitch, int *cls)
{
    if (pitch < 64 || pitch > 1984) return false;
    uint32_t nb = 0;
    const int c = stream_class(pitch | 1u, &nb);  // | 1: size the buffers for the re-pitched form of a full-width box
    if (c == 0) return false;
    *cls = c == 1 ? 1 : 2;
    return true;
}

uint32_t resize_cropped_stream_blocks(uint32_t crop_w, uint32_t x0, uint32_t pitch, int cls, uint32_t *wp)
{
    uint32_t p = (crop_w + 3u + 15u) & ~15u;
    if ((p / 16) % 2 == 0) p += 16;
    // full-width box (top / bottom bars): the DMA is a linear copy - unless that pitch puts a block's 16 rows on one bank group
    if (x0 == 0 && crop_w == pitch && pitch % 16 == 0 && pitch % 256 != 0) p = pitch;
    *wp = p;
    return stream_blocks_per_chunk(p, cls == 1 ? kStreamBufS : kStreamBufM);
}

static bool aligned16(const HashCall &c) { return ((uintptr_t)c.base | c.frame_stride | c.clip_stride) % 16 == 0; }

// a stream route's values: the per-wave form (band table, nw waves) where the width takes it, else the chunk form; the K-split form
static void route_stream(HashPlan &p, uint32_t w, int nw)
{
    p.route = nw ? HashRoute::kWaveStream : HashRoute::kChunkStream;
    p.layout_h = nw ? kMfmaLayoutHorizontalBand : kMfmaLayoutHorizontal;
    p.waves = nw;
    if (!nw) stream_class(w, &p.nb);
}
static void route_ksplit(HashPlan &p, uint32_t w)
{
    uint32_t wp = 0;
    p.route = HashRoute::kKsplit;
    p.nb = ksplit_geometry(w, &wp);
}

// The fused family (one kernel resizes, transforms and hashes).  The persistent kernels load 16 bytes at a time without looking at the buffer's
// end.  With W % 16 == 0 no load crosses a row's end; with any other width a row's last load runs up to 15 bytes into what follows - the next row,
// frame or clip, all inside the buffer, at zero coefficients - except behind the LAST clip: that one goes to the one-workgroup-per-clip kernel and
// its careful loader (round 5).
static void plan_fused(const HashCall &c, const HashKnobs &k, HashPlan &p)
{
    const bool persistent_ok = !k.hash_no_persistent && p.n_kt <= 4 && p.n_rg <= 4;
    // (clips that overlap or repeat - clip_stride below 16, e.g. 0: one clip hashed n times - end within 15 bytes of the buffer's end more than
    // once: then no clip may take the unchecked loads, and all of them go to the one-workgroup-per-clip kernel)
    p.last_clip_apart = persistent_ok && c.w % 16 != 0 && c.n_clips >= 2 && c.clip_stride >= 16;
    if (!persistent_ok || !(c.w % 16 == 0 || p.last_clip_apart)) {
        p.route = HashRoute::kPerClipFused;
    } else if (p.n_kt == 1 && p.n_rg == 1) {
        p.route = HashRoute::kPersistentOneTile;
        p.full_tile = c.w == 64 && c.h == 64;
    } else {  // up to 256 x 256: units of eight loads per lane in flight, persistent; 129 ... 256 rows: four row groups (the fourth may be empty)
        p.route = HashRoute::kTiled;
        p.tiled_nrg = p.n_rg > 2 ? 4 : p.n_rg;
        p.waves = tiled_waves(p.n_kt, p.tiled_nrg);
    }
}

HashPlan plan_hash(const HashCall &c, const HashKnobs &k, TableFit fit)
{
    HashPlan p;
    p.n_kt = (int)((c.w + 63) / 64);
    p.n_rg = (int)((c.h + 63) / 64);
    if (c.w == 16 && c.h == 16 && aligned16(c)) { p.route = HashRoute::kDirect16; return p; }  // the resize is a copy
    if (k.resize_mode == 1) { p.route = HashRoute::kScalar; return p; }
    // tables that do not fit the i8 split: the scalar fixed-point kernel (any coefficient range); a forced mode refuses
    if (fit == TableFit::kNoPlain) { p.route = k.resize_mode == 0 ? HashRoute::kScalar : HashRoute::kRefused; return p; }
    // Resize on the matrix cores (exact i8 x i8 -> i32): small frames fuse the DCT into the same kernel.
    // frames taller than two 64-row groups go to the per-frame kernels; the whole-line form is the default
    // (round 5: except the wide, short ones that stream faster - resize_short_prefers_stream - where they are eligible to)
    // (and the narrow ones of up to 256 rows that the tiled persistent kernel serves better than the stream kernels - resize_tall_prefers_tiled)
    const bool eligible = resize_stream_eligible(c.base, c.w, c.h, c.frame_stride, c.clip_stride, k.wavestream_knob);
    const bool fused = k.resize_mode == 3 || (k.resize_mode == 0 && p.n_rg <= 2 && !(resize_short_prefers_stream(c.w, c.h) && eligible)) ||
                       (k.resize_mode == 0 && !k.hash_no_persistent && resize_tall_prefers_tiled(c.w, c.h));
    if (fused) { plan_fused(c, k, p); return p; }
    // tightly packed frames stream linearly through LDS where that is the faster form (resize_stream_eligible); wide frames take the horizontal
    // table in band form (= the per-wave form), and leave the stream form where that table does not fit
    const int nw = resize_wavestream_waves(c.w, k.wavestream_knob);
    const bool streamed = (k.resize_mode == 0 || k.resize_mode == 5) && eligible && !(nw != 0 && fit == TableFit::kNoBand);
    // frames wider than the per-wave buffers (1920 columns): the K-split form, table in registers (measured against the
    // whole-line kernel: 3840 wide 5.6 -> 6.7 TB/s, 2560 5.5 -> 6.2, 2000 3.6 -> 5.8, 2048 level)
    const bool ksplit = ((k.resize_mode == 0 && !streamed && c.w > 1920) || k.resize_mode == 6) &&
                        resize_ksplit_eligible(c.base, c.w, c.h, c.frame_stride, c.clip_stride);
    if (ksplit) route_ksplit(p, c.w);
    else if (streamed) route_stream(p, c.w, nw);
    else { p.route = HashRoute::kWholeLine; p.layout_v = kMfmaLayoutVerticalWide; }
    return p;
}

HashPlan plan_resize_only(const HashCall &c, const HashKnobs &k, TableFit fit)
{
    HashPlan p = plan_hash(c, k, fit);
    if (p.route == HashRoute::kPersistentOneTile || p.route == HashRoute::kTiled || p.route == HashRoute::kPerClipFused || p.route == HashRoute::kDirect16) {
        HashKnobs whole_line = k;
        whole_line.resize_mode = 4;
        p = plan_hash(c, whole_line, fit);
        if (p.route == HashRoute::kDirect16) {  // (16 x 16 frames on 16-byte boundaries: the windows calls read them in place and never ask)
            p.route = HashRoute::kWholeLine;
            p.layout_v = kMfmaLayoutVerticalWide;
        }
        if (p.route == HashRoute::kRefused) p.route = HashRoute::kScalar;  // (refused by the mode forced here, not by the caller's)
    }
    return p;
}

CropPlan plan_cropped(const HashCall &c, const HashKnobs &k, const uint32_t *crops, const CropTableFit &fit)
{
    CropPlan p;
    const uint32_t w = c.w, h = c.h;
    const auto bad_box = [&](size_t i) { return (uint64_t)crops[4 * i] + crops[4 * i + 1] >= w || (uint64_t)crops[4 * i + 2] + crops[4 * i + 3] >= h; };  // crop.rs:21-22
    const bool tall = (h + 63) / 64 > 2, ends16 = ((uint64_t)w * h) % 16 == 0 && (uint64_t)w * h < (1ull << 31);
    // small frames (round 5): one workgroup per CLIP, a wave per four frames, resize + DCT (resize_dct_hash_cropped_small_kernel); it checks
    // the boxes in its own single pass over them
    if (!tall && w <= 256 && k.resize_mode == 0 && !k.no_smallcrop) { p.kind = CropPlan::kSmall; return p; }
    // Three kernels read crop boxes in place; a call is dealt out between the first two by box shape, clip by clip (each entry of a
    // launch names its clip of the batch: CropStreamClip::src_clip), and one dct_hash launch follows over the whole batch:
    //  * ROWCROP stream kernels - full-width boxes (top / bottom bars only: a 2.39 : 1 film in a 16 : 9 frame, the commonest letterbox;
    //    clips without bars among them are boxes of the whole frame).  The box is a contiguous range of rows at the frame's own pitch,
    //    so it streams like a shorter frame: the kernel the uncropped call would take at that width (per-wave, chunk or K-split form)
    //    with a per-clip first row, height and vertical table.
    //  * the cropped stream kernel - boxes with side bars (pillarboxed clips): rows x0 .. x0 + w of the box go through LDS by gather
    //    DMA.  Also full-width boxes where no ROWCROP kernel applies and the pitch is not a multiple of the 128-byte line.
    //    Measured, detect + crop + hash against the whole-line kernel below: 854x480 1.68 -> 1.24 ms per 1000 clips, 720x576 1.42 -> 1.14,
    //    426x240 x4000 1.85 -> 1.33, 1366x768 x500 2.19 -> 1.95; pillarboxed 1920x1080 x1000 crop + hash 7.7 -> 5.5 ms, 1280x720 x2000
    //    6.4 -> 3.9, 1536x864 4.5 -> 2.9, 640x360 x4000 3.4 -> 2.5; 1024 wide 3.5 -> 3.8: stays (gpurun_out/r03pb).
    //  * the whole-line cropped kernel - everything else: misaligned buffers, frames that do not end on 16 bytes, short frames,
    //    boxes whose tables do not fit the i8 split, VDF_RESIZE_MODE=4.
    std::vector<uint32_t> side;
    for (size_t i = 0; i < c.n_clips; i++) {
        if (bad_box(i)) { p.kind = CropPlan::kBadBox; return p; }
        (crops[4 * i] == 0 && crops[4 * i + 1] == 0 ? p.rows : side).push_back((uint32_t)i);
    }
    // -- can the full-width boxes take a ROWCROP kernel, and which?
    if (k.resize_mode == 0 && tall && !p.rows.empty() && (resize_rowcrop_streams(w) || k.rowcrop_all) && !k.no_rowcrop && fit.rows_table && fit.height_tables) {
        if (resize_stream_eligible(c.base, w, h, c.frame_stride, c.clip_stride, k.wavestream_knob)) route_stream(p.rows_kernel, w, resize_wavestream_waves(w, k.wavestream_knob));
        else if (w > 1920 && resize_ksplit_eligible(c.base, w, h, c.frame_stride, c.clip_stride)) route_ksplit(p.rows_kernel, w);
    }
    if (p.rows_kernel.route == HashRoute::kRefused) p.rest.swap(p.rows);
    // -- boxes with side bars that share their column range: the per-wave kernel gathers the box (one launch per distinct range)
    if (k.resize_mode == 0 && tall && ends16 && aligned16(c) && !side.empty() && !k.no_boxstream && !k.no_rowcrop && fit.height_tables) {
        std::map<uint64_t, size_t> by_range;  // (x0, width) -> group
        std::vector<CropBoxGroup> cand;
        for (uint32_t i : side) {
            const uint32_t l = crops[4 * i], bw = w - l - crops[4 * i + 1];
            auto it = by_range.find(crop_range_key(l, bw));
            if (it == by_range.end()) {
                it = by_range.emplace(crop_range_key(l, bw), cand.size()).first;
                cand.push_back(CropBoxGroup{l, bw, resize_wavestream_waves_box(w, l, bw, k.wavestream_knob), {}});
            }
            cand[it->second].ids.push_back(i);
        }
        for (CropBoxGroup &g : cand) {
            // (a launch per range: ranges shared by fewer than four clips - a launch would leave most CUs idle - and the ranges beyond sixteen
            // are left to the gather kernel)
            const bool no_table = std::find(fit.ranges_without_table.begin(), fit.ranges_without_table.end(), crop_range_key(g.x0, g.box_w)) != fit.ranges_without_table.end();
            if (g.waves && g.ids.size() >= kMinCropBoxGroupClips && p.groups.size() < kMaxCropBoxGroups && !no_table) p.groups.push_back(std::move(g));
            else p.rest.insert(p.rest.end(), g.ids.begin(), g.ids.end());
        }
    } else {
        p.rest.insert(p.rest.end(), side.begin(), side.end());
    }
    if (p.rows.empty() && p.groups.empty()) {  // nothing streams per clip: the whole call through one general kernel
        p.rows_kernel = HashPlan();
        p.rest.resize(c.n_clips);
        for (size_t i = 0; i < c.n_clips; i++) p.rest[i] = (uint32_t)i;
    }
    // the general kernel for the rest: the cropped stream kernel for side-bar boxes at every pitch but 1024 and for full-width boxes where the
    // pitch is not line-aligned (measured above) - if every box fits its chunk buffers - else the whole-line kernel
    bool rest_has_side = false;
    for (uint32_t i : p.rest) rest_has_side = rest_has_side || crops[4 * i] != 0 || crops[4 * i + 1] != 0;
    p.rest_gather = !p.rest.empty() && fit.gather_tables && tall && ends16 && (((uintptr_t)c.base | c.frame_stride | c.clip_stride) & 3) == 0 &&
                    (k.resize_mode == 0 || k.resize_mode == 5) && resize_cropped_stream_class(w, &p.gather_cls) &&
                    (k.resize_mode == 5 || (rest_has_side ? w != 1024 : w % 128 != 0));
    p.gather_shift = (w & 3u) != 0;
    for (size_t j = 0; j < p.rest.size() && p.rest_gather; j++) {
        const uint32_t i = p.rest[j], x0 = crops[4 * i], bw = w - x0 - crops[4 * i + 1], bh = h - crops[4 * i + 2] - crops[4 * i + 3];
        uint32_t wp = 0;
        const uint32_t nb = resize_cropped_stream_blocks(bw, x0, w, p.gather_cls, &wp);
        p.gather_shift = p.gather_shift || (x0 & 3u) != 0;
        if (nb == 0 || (nb < 2 && bh > 16)) p.rest_gather = false;  // one block per chunk would leave three of the four waves idle
    }
    return p;
}

LetterboxPlan plan_letterbox(const HashCall &c, const HashKnobs &k)
{
    // Small frames (round 6): the boxes never visit the host.  Every box size's tables are resident, so
    //  * frames of at most 64 x 64 take ONE kernel that detects, crops, resizes, transforms and hashes (letterbox_resize_dct_hash_small_kernel);
    //    the clips within 64 bytes of the buffer's end (the last one, as a rule) take the route below for its careful loader;
    //  * other small frames: the two detect kernels, then the one-workgroup-per-clip kernel reads each clip's box where they left it.
    LetterboxPlan p{};
    p.small_frames = (c.h + 63) / 64 <= 2 && c.w <= 256 && k.resize_mode == 0 && !k.no_smallcrop && !k.lb_host_plan;
    p.one_tile = p.small_frames && c.w <= 64 && c.h <= 64 && !k.no_lb_fused;
    // clip i's loads stay inside the buffer iff it ends at least 64 bytes before the last clip does: (n - 1 - i) * clip_stride >= 64
    p.n_tail = !p.one_tile || c.clip_stride == 0 ? c.n_clips : std::min<size_t>(c.n_clips, (64 + c.clip_stride - 1) / c.clip_stride);
    return p;
}

// ---- clips of different frame sizes in one call ------------------------------------------------------------------------------------------
MixedCheck check_mixed(const MixedClip *clips, size_t n, uint32_t frames_per_clip, uint64_t buf_bytes)
{
    if (frames_per_clip < 16) return {MixedError::kNotEnoughFrames, 0};
    for (size_t i = 0; i < n; i++)
        if (clips[i].w == 0 || clips[i].h == 0) return {MixedError::kZeroDim, i};
    for (size_t i = 0; i < n; i++)
        if (clips[i].frame_stride < (uint64_t)clips[i].w * clips[i].h) return {MixedError::kStrideBelowFrame, i};
    for (size_t i = 0; i < n; i++) {
        const uint32_t *c = clips[i].crop;
        if ((uint64_t)c[0] + c[1] >= clips[i].w || (uint64_t)c[2] + c[3] >= clips[i].h) return {MixedError::kEmptyBox, i};  // crop.rs:21-22
    }
    for (size_t i = 0; i < n; i++) {  // the last byte of frame 15, in 128 bits: no offset or stride a caller can write wraps the sum
        const unsigned __int128 end = (unsigned __int128)clips[i].offset + (unsigned __int128)15 * clips[i].frame_stride + (uint64_t)clips[i].w * clips[i].h;
        if (end > buf_bytes) return {MixedError::kOutOfBuffer, i};
    }
    return {};
}

MixedPart mixed_part_of(uint32_t w, uint32_t h, const HashKnobs &k)
{
    if (w <= 256 && (h + 63) / 64 <= 2 && k.resize_mode == 0 && !k.no_smallcrop) return MixedPart::kSmall;  // CropPlan::kSmall's rule
    return w < 192 ? MixedPart::kLines : MixedPart::kWideLines;  // as launch_crop_parts picks the whole-line form
}

MixedPlan plan_mixed(const MixedClip *clips, size_t n, const HashKnobs &k)
{
    MixedPlan p;
    if (n == 0) return p;
    bool uniform = true;
    const uint64_t step = n > 1 ? clips[1].offset - clips[0].offset : 16 * clips[0].frame_stride;
    for (size_t i = 0; i < n; i++) {
        const MixedClip &c = clips[i];
        p.cropped = p.cropped || (c.crop[0] | c.crop[1] | c.crop[2] | c.crop[3]) != 0;
        uniform = uniform && c.w == clips[0].w && c.h == clips[0].h && c.frame_stride == clips[0].frame_stride;
        // offsets ascend by one positive step (equal or descending offsets are no clip_stride the uniform launchers know)
        if (i > 0) uniform = uniform && c.offset > clips[i - 1].offset && c.offset - clips[i - 1].offset == step;
    }
    if (uniform) {
        p.kind = MixedPlan::kUniform;
        p.offset0 = clips[0].offset;
        p.clip_stride = step;
        return p;
    }
    p.kind = MixedPlan::kMixed;
    p.descs.reserve(n);
    const MixedPart order[3] = {MixedPart::kSmall, MixedPart::kLines, MixedPart::kWideLines};
    for (MixedPart part : order) {
        const size_t first = p.descs.size();
        for (size_t i = 0; i < n; i++) {
            const MixedClip &c = clips[i];
            if (mixed_part_of(c.w, c.h, k) != part) continue;
            MixedClipDesc d{};
            d.offset = c.offset;
            d.frame_stride = c.frame_stride;
            d.x0 = c.crop[0]; d.y0 = c.crop[2];
            d.bw = c.w - c.crop[0] - c.crop[1]; d.bh = c.h - c.crop[2] - c.crop[3];
            d.h_table = d.bw; d.v_table = d.bh;
            d.out_index = (uint32_t)i;
            d.pitch = c.w;
            p.max_w = std::max(p.max_w, d.bw); p.max_h = std::max(p.max_h, d.bh);
            p.descs.push_back(d);
        }
        if (part == MixedPart::kSmall) p.n_small = p.descs.size();
        for (size_t at = first; at < p.descs.size(); at += kMaxClipsPerLaunch)
            p.launches.push_back(MixedLaunch{part, at, std::min(kMaxClipsPerLaunch, p.descs.size() - at)});
    }
    return p;
}

LetterboxMixedPlan plan_letterbox_mixed(const MixedClip *clips, size_t n, const HashKnobs &)
{
    LetterboxMixedPlan p;
    for (size_t i = 0; i < n; i++)
        if ((clips[i].crop[0] | clips[i].crop[1] | clips[i].crop[2] | clips[i].crop[3]) != 0) {
            p.kind = LetterboxMixedPlan::kCropGiven;
            p.bad_clip = i;
            return p;
        }
    if (n == 0) return p;
    bool uniform = true;  // plan_mixed's rule
    const uint64_t step = n > 1 ? clips[1].offset - clips[0].offset : 16 * clips[0].frame_stride;
    for (size_t i = 0; i < n; i++) {
        const MixedClip &c = clips[i];
        uniform = uniform && c.w == clips[0].w && c.h == clips[0].h && c.frame_stride == clips[0].frame_stride;
        if (i > 0) uniform = uniform && c.offset > clips[i - 1].offset && c.offset - clips[i - 1].offset == step;
    }
    if (uniform) {
        p.kind = LetterboxMixedPlan::kUniform;
        p.offset0 = clips[0].offset;
        p.clip_stride = step;
        return p;
    }
    p.descs.reserve(n);
    for (int batch : {8, 16, 32}) {
        const size_t first = p.descs.size();
        for (size_t i = 0; i < n; i++) {
            const MixedClip &c = clips[i];
            if (letterbox_column_batch(c.h) != batch) continue;
            p.descs.push_back(LetterboxProbeDesc{c.offset, c.frame_stride, c.w, c.h, (uint32_t)i, 0u});
        }
        for (size_t at = first; at < p.descs.size(); at += kMaxClipsPerLaunch) {
            const size_t count = std::min(kMaxClipsPerLaunch, p.descs.size() - at);
            p.launches.push_back(LetterboxMixedLaunch{batch, at, count, p.work_bytes});
            p.work_bytes += letterbox_work_list_bytes(count * kLetterboxProbes);
        }
    }
    return p;
}

}  // namespace vdf
