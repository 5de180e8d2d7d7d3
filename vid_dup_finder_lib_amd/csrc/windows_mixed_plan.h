// Window hashes of videos of DIFFERENT frame sizes and frame counts in one call (vdf_hash_windows_clips_u8[_device]): the
// argument checks in the order their codes are reported, first[] (the layout the align calls read), the segments of every video and the
// table a workgroup of dct_hash_windows_mixed_kernel finds its video in, the resize stage as 16-frame pseudo-clips for the mixed whole-line
// kernels (resize_mfma_mixed_kernel), and the one record per video the windows kernel reads.  Host-only arithmetic (no HIP types), shared by
// api.cpp and the kernel in dct_hash.hip; tests/cpp/windows_mixed_plan_main.cpp enumerates it on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "resize_dispatch.h"
#include "windows_plan.h"

#if defined(__HIPCC__)
#define VDF_WINDOWS_MIXED_HD __host__ __device__ inline
#else
#define VDF_WINDOWS_MIXED_HD inline
#endif

namespace vdf {

// What dct_hash_windows_mixed_kernel reads of its video, once, as one 32-byte piece.  Frame f of the video is in `small` at
// 256 (16 slot0 + f) for f < main_frames (the video's whole chunks are consecutive pseudo-clips) and at
// 256 (16 (slot0 + main_frames / 16) + f - tail_first) otherwise (the tail pseudo-clip follows them; main_frames == F: there is none).
struct WindowsVideoRecord {
    uint32_t slot0;        // the video's first pseudo-clip slot (4096 bytes each) in `small`
    uint32_t main_frames;  // 16 * (F / 16)
    uint32_t tail_first;   // F - 16
    uint32_t n_win;        // windows of the video
    uint32_t first;        // first[i]: window k goes to row first + k of the outputs
    uint32_t seg_first;    // the video's first segment (= workgroup) of the call
    uint32_t reserved[2];  // 0
};
static_assert(sizeof(WindowsVideoRecord) == 32, "the kernel reads a record as one 32-byte piece");

// The video that owns segment g: the last i with seg_first[i] <= g.  seg_first has n_videos + 1 ascending entries (strictly: every video has
// a segment), seg_first[0] == 0 and g < seg_first[n_videos].  This is the lookup the kernel runs - workgroup-uniform, about log2(n_videos)
// dependent loads - and the one the planner test maps every segment back with.
VDF_WINDOWS_MIXED_HD uint32_t windows_video_of(const uint32_t *seg_first, uint32_t n_videos, uint32_t g)
{
    uint32_t lo = 0, hi = n_videos;  // seg_first[lo] <= g < seg_first[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (seg_first[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The argument checks that need no context, in the order their codes are reported (include/vdf.h), over ALL videos before anything is queued.
enum class WindowsMixedError { kNone, kNotEnoughFrames, kZeroDim, kStrideBelowFrame, kEmptyBox, kOutOfBuffer, kZeroWindowStride, kFrameCount, kTooManyWindows };
struct WindowsMixedCheck { WindowsMixedError error = WindowsMixedError::kNone; size_t video = 0; };

// first[i] = windows of videos 0 .. i - 1; false: 2^32 windows or more (first is then unspecified).  stride > 0.
inline bool windows_first(const uint32_t *n_frames, size_t n, uint32_t stride, uint32_t *first)
{
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        first[i] = (uint32_t)at;
        at += window_count(n_frames[i], stride);
        if (at > 0xFFFFFFFFull) return false;
    }
    first[n] = (uint32_t)at;
    return true;
}

inline WindowsMixedCheck check_windows_mixed(const MixedClip *clips, const uint32_t *n_frames, size_t n, uint32_t stride, uint64_t buf_bytes)
{
    for (size_t i = 0; i < n; i++)
        if (n_frames[i] < kWindowFrames) return {WindowsMixedError::kNotEnoughFrames, i};
    for (size_t i = 0; i < n; i++)
        if (clips[i].w == 0 || clips[i].h == 0) return {WindowsMixedError::kZeroDim, i};
    for (size_t i = 0; i < n; i++)
        if (clips[i].frame_stride < (uint64_t)clips[i].w * clips[i].h) return {WindowsMixedError::kStrideBelowFrame, i};
    for (size_t i = 0; i < n; i++) {
        const uint32_t *c = clips[i].crop;
        if ((uint64_t)c[0] + c[1] >= clips[i].w || (uint64_t)c[2] + c[3] >= clips[i].h) return {WindowsMixedError::kEmptyBox, i};
    }
    for (size_t i = 0; i < n; i++) {  // the last byte of the video's LAST frame, in 128 bits: no offset, stride or count a caller can write wraps the sum
        const unsigned __int128 end = (unsigned __int128)clips[i].offset + (unsigned __int128)(n_frames[i] - 1) * clips[i].frame_stride + (uint64_t)clips[i].w * clips[i].h;
        if (end > buf_bytes) return {WindowsMixedError::kOutOfBuffer, i};
    }
    if (stride == 0) return {WindowsMixedError::kZeroWindowStride, 0};
    for (size_t i = 0; i < n; i++)
        if (n_frames[i] > 0xFFFFFFC0u) return {WindowsMixedError::kFrameCount, i};  // the kernel's frame arithmetic is 32-bit
    uint64_t windows = 0, slots = 0;
    for (size_t i = 0; i < n; i++) {  // ... and so are its rows of the outputs and its slots of `small`
        windows += window_count(n_frames[i], stride);
        slots += n_frames[i] / kWindowFrames + (n_frames[i] % kWindowFrames != 0);
        if (windows > 0xFFFFFFFFull || slots > 0xFFFFFFFFull) return {WindowsMixedError::kTooManyWindows, i};
    }
    return {};
}

struct WindowsMixedPlan {
    enum Kind { kUniform, kMixed } kind = kMixed;
    // kUniform: one (w, h, frame_stride, n_frames), no box, offsets one positive step apart: hash_windows_locked on (base + offset0, clip_stride) -
    // the uniform call's kernels, words and speed
    uint64_t offset0 = 0, clip_stride = 0;
    uint32_t per_seg = 0;                    // windows per segment: the same for every video of a call (plan_windows)
    std::vector<uint32_t> first, seg_first;  // [n_videos + 1]
    // kMixed: the pseudo-clips part by part (lines, wide lines), a video's one after the other; descs[s] is written to slot s of `small`
    std::vector<MixedClipDesc> descs;    // out_index: the video (for messages; the resize kernels do not read it)
    std::vector<MixedLaunch> launches;   // each at most kMaxClipsPerLaunch pseudo-clips of one part
    std::vector<WindowsVideoRecord> videos;
    uint32_t max_w = 0, max_h = 0;       // the largest box sizes: what the table index is sized by
    size_t small_bytes = 0;              // 256 bytes per pseudo-clip frame
};

// Small frames do not take the kernel that fuses the DCT: every frame goes through a whole-line part (HashKnobs::no_smallcrop's rule).
constexpr MixedPart windows_mixed_part_of(uint32_t w) { return w < 192 ? MixedPart::kLines : MixedPart::kWideLines; }

// the videos have passed check_windows_mixed
inline WindowsMixedPlan plan_windows_mixed(const MixedClip *clips, const uint32_t *n_frames, size_t n, uint32_t stride)
{
    WindowsMixedPlan p;
    p.first.assign(n + 1, 0);
    p.seg_first.assign(n + 1, 0);
    if (n == 0) return p;
    windows_first(n_frames, n, stride, p.first.data());
    p.per_seg = plan_windows(n_frames[0], stride).per_seg;
    bool uniform = true;  // plan_mixed's rule, with the frame count among what the videos share and no box
    const uint64_t step = n > 1 ? clips[1].offset - clips[0].offset : (uint64_t)n_frames[0] * clips[0].frame_stride;
    for (size_t i = 0; i < n; i++) {
        const MixedClip &c = clips[i];
        uniform = uniform && (c.crop[0] | c.crop[1] | c.crop[2] | c.crop[3]) == 0 && c.w == clips[0].w && c.h == clips[0].h &&
                  c.frame_stride == clips[0].frame_stride && n_frames[i] == n_frames[0];
        if (i > 0) uniform = uniform && c.offset > clips[i - 1].offset && c.offset - clips[i - 1].offset == step;
        p.seg_first[i + 1] = p.seg_first[i] + plan_windows(n_frames[i], stride).n_seg;  // (at most one segment per window: below 2^32)
    }
    if (uniform) {
        p.kind = WindowsMixedPlan::kUniform;
        p.offset0 = clips[0].offset;
        p.clip_stride = step;
        return p;
    }
    p.videos.resize(n);
    for (MixedPart part : {MixedPart::kLines, MixedPart::kWideLines}) {
        const size_t first_desc = p.descs.size();
        for (size_t i = 0; i < n; i++) {
            const MixedClip &c = clips[i];
            if (windows_mixed_part_of(c.w) != part) continue;
            const uint32_t F = n_frames[i], n_chunks = F / kWindowFrames;
            MixedClipDesc d{};
            d.frame_stride = c.frame_stride;
            d.x0 = c.crop[0]; d.y0 = c.crop[2];
            d.bw = c.w - c.crop[0] - c.crop[1]; d.bh = c.h - c.crop[2] - c.crop[3];
            d.h_table = d.bw; d.v_table = d.bh;
            d.out_index = (uint32_t)i;
            d.pitch = c.w;
            p.max_w = std::max(p.max_w, d.bw); p.max_h = std::max(p.max_h, d.bh);
            WindowsVideoRecord &v = p.videos[i];
            v.slot0 = (uint32_t)p.descs.size();
            v.main_frames = kWindowFrames * n_chunks;
            v.tail_first = F - kWindowFrames;
            v.n_win = p.first[i + 1] - p.first[i];
            v.first = p.first[i];
            v.seg_first = p.seg_first[i];
            for (uint32_t q = 0; q < n_chunks; q++) {
                d.offset = c.offset + (uint64_t)q * kWindowFrames * c.frame_stride;
                p.descs.push_back(d);
            }
            if (F % kWindowFrames) {  // the tail pseudo-clip: the video's last 16 frames, so that no frame past the last is ever named
                d.offset = c.offset + (uint64_t)(F - kWindowFrames) * c.frame_stride;
                p.descs.push_back(d);
            }
        }
        for (size_t at = first_desc; at < p.descs.size(); at += kMaxClipsPerLaunch)
            p.launches.push_back(MixedLaunch{part, at, std::min(kMaxClipsPerLaunch, p.descs.size() - at)});
    }
    p.small_bytes = p.descs.size() * 4096;
    return p;
}

// where frame f of a video is in `small`, in bytes: the rule the kernel uses
VDF_WINDOWS_MIXED_HD size_t windows_mixed_frame_offset(const WindowsVideoRecord &v, uint32_t f)
{
    return f < v.main_frames ? ((size_t)v.slot0 * 16 + f) * 256 : (((size_t)v.slot0 + v.main_frames / 16) * 16 + (f - v.tail_first)) * 256;
}

}  // namespace vdf
