// Hashes of every 16-frame window of a clip (vdf_hash_windows_u8[_device]): which windows a workgroup of
// dct_hash_windows_kernel serves, which frames it walks for them, and how the frames reach the resize kernels as 16-frame pseudo-clips.
// Host-only arithmetic (no HIP), shared by api.cpp and the launcher in dct_hash.hip; tests/cpp/windows_plan_main.cpp enumerates it on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vdf {

constexpr uint32_t kWindowFrames = 16;  // = VDF_DCT_SIZE
// A segment = the windows that start within one span of kWindowSegChunks chunks of 16 frames, all served by one workgroup.  Two chunks:
// a 7200-frame clip at stride 1 is 225 workgroups - one round of the 256 CUs - and a segment walks at most 47 frames for 32 windows
// (the 15 it shares with its successor are computed by both: per frame the spatial passes are 416 DCT-16, per window pass t is 100).
constexpr uint32_t kWindowSegChunks = 2;
constexpr uint32_t kWindowSegFrames = kWindowSegChunks * kWindowFrames;
constexpr size_t kMaxWindowGroupsPerLaunch = size_t(1) << 23;  // x 256 threads stays under HIP's 2^32 work-item grid limit

// windows of a clip of F frames: window k = frames [k * stride, k * stride + 16); 0 if F < 16 or stride == 0
constexpr size_t window_count(uint32_t F, uint32_t stride) { return (F < kWindowFrames || stride == 0) ? 0 : (size_t)(F - kWindowFrames) / stride + 1; }

struct WindowsPlan {
    uint32_t F = 0, stride = 0;
    uint32_t n_win = 0;     // windows per clip
    uint32_t per_seg = 0;   // windows per segment (the last segment of a clip may hold fewer): as many as start within kWindowSegFrames frames
    uint32_t n_seg = 0;     // segments (= workgroups) per clip
    // segment s of a clip
    uint32_t first_window(uint32_t s) const { return s * per_seg; }
    uint32_t end_window(uint32_t s) const { return (uint32_t)std::min<uint64_t>((uint64_t)(s + 1) * per_seg, n_win); }
    uint32_t segment_of(uint32_t k) const { return k / per_seg; }
    // the frames the segment's workgroup may read: [frame_begin, frame_end), all of them (strides above 16: per_seg = 1, the one window's 16 frames)
    uint32_t frame_begin(uint32_t s) const { return (uint32_t)((uint64_t)first_window(s) * stride); }
    uint32_t frame_end(uint32_t s) const { return (uint32_t)((uint64_t)(end_window(s) - 1) * stride + kWindowFrames); }
    // frames at the segment's start that its predecessor walks as well
    uint32_t lead_in(uint32_t s) const { return s == 0 ? 0 : (frame_end(s - 1) > frame_begin(s) ? frame_end(s - 1) - frame_begin(s) : 0); }
};

inline WindowsPlan plan_windows(uint32_t F, uint32_t stride)
{
    WindowsPlan p;
    p.F = F;
    p.stride = stride;
    p.n_win = (uint32_t)window_count(F, stride);  // < 2^32: at most F - 15
    if (p.n_win == 0) return p;
    p.per_seg = std::max<uint32_t>(1, kWindowSegFrames / stride);
    p.n_seg = (p.n_win + p.per_seg - 1) / p.per_seg;
    return p;
}

// ---- the resize stage: every frame once into 16 x 16 bytes, by the kernels of the plain call (16-frame clips at one clip stride) ----------
// A clip is F / 16 pseudo-clips of 16 consecutive frames ("chunks") plus, when F is no multiple of 16, one that starts at frame F - 16.
// The kernels write pseudo-clip i of a launch to small + 4096 i, so a launch is a run of pseudo-clips one source stride apart:
//   kPacked    clips follow each other without a gap and F is a multiple of 16: all chunks of all clips are ONE run
//   kByClip    one launch per clip over its chunks (16 frame strides apart)                  small chunk (c, j) at 4096 (c n_chunks + j)
//   kByChunk   one launch per chunk index over the clips (one clip stride apart)             small chunk (c, j) at 4096 (j n_clips + c)
// and the tail pseudo-clips of all clips are one more launch into a slab of their own behind the chunks.  kByClip or kByChunk, whichever
// has fewer launches: never more than F / 16 + 1, however many clips there are.
struct WindowsResizePlan {
    enum Layout { kPacked, kByClip, kByChunk } layout = kByClip;
    uint32_t n_chunks = 0;   // whole 16-frame chunks per clip
    bool tail = false;       // F % 16 != 0
    size_t clip_step = 0, chunk_step = 0;  // bytes in `small` between a clip's chunks 0 of consecutive clips / between consecutive chunks of a clip
    size_t tail_offset = 0;  // bytes from small to the tail slab (clip c's tail pseudo-clip at + 4096 c)
    size_t small_bytes = 0;
    size_t launches = 0;     // resize launches of at most kMaxClipsPerLaunch pseudo-clips, if no launch had to be cut
};

inline WindowsResizePlan plan_windows_resize(size_t n_clips, uint32_t F, size_t frame_stride, size_t clip_stride)
{
    WindowsResizePlan r;
    r.n_chunks = F / kWindowFrames;
    r.tail = F % kWindowFrames != 0;
    const size_t chunks = n_clips * r.n_chunks;
    if (!r.tail && (n_clips == 1 || clip_stride == (size_t)F * frame_stride)) r.layout = WindowsResizePlan::kPacked;
    else r.layout = n_clips <= r.n_chunks ? WindowsResizePlan::kByClip : WindowsResizePlan::kByChunk;
    if (r.layout == WindowsResizePlan::kByChunk) { r.clip_step = 4096; r.chunk_step = 4096 * n_clips; }
    else { r.clip_step = 4096 * (size_t)r.n_chunks; r.chunk_step = 4096; }
    r.tail_offset = 4096 * chunks;
    r.small_bytes = 4096 * (chunks + (r.tail ? n_clips : 0));
    r.launches = (r.layout == WindowsResizePlan::kPacked ? 1 : r.layout == WindowsResizePlan::kByClip ? n_clips : r.n_chunks) + (r.tail ? 1 : 0);
    return r;
}

// The launches of the plan: run = n pseudo-clips `step` bytes apart from src_offset (bytes behind frame 0 of clip 0), pseudo-clip i to
// small + dst_offset + 4096 i.  Each is planned like a plain call on (base + src_offset, clip_stride = step) - resize_dispatch.h: plan_resize_only.
struct WindowsResizeRun { size_t src_offset, n, step, dst_offset; };
inline std::vector<WindowsResizeRun> windows_resize_runs(const WindowsResizePlan &r, size_t n_clips, uint32_t F, size_t frame_stride, size_t clip_stride)
{
    std::vector<WindowsResizeRun> runs;
    const size_t chunk_bytes = kWindowFrames * frame_stride;
    switch (r.layout) {
    case WindowsResizePlan::kPacked: runs.push_back({0, n_clips * r.n_chunks, chunk_bytes, 0}); break;
    case WindowsResizePlan::kByClip:
        for (size_t c = 0; c < n_clips; c++) runs.push_back({c * clip_stride, r.n_chunks, chunk_bytes, c * r.clip_step});
        break;
    case WindowsResizePlan::kByChunk:
        for (size_t q = 0; q < r.n_chunks; q++) runs.push_back({q * chunk_bytes, n_clips, clip_stride, q * r.chunk_step});
        break;
    }
    if (r.tail) runs.push_back({(size_t)(F - kWindowFrames) * frame_stride, n_clips, clip_stride, r.tail_offset});
    return runs;
}

}  // namespace vdf
