// Stand-alone check of csrc/windows_plan.h (no HIP, no GPU; built with -fsanitize=address,undefined by tests/test_hash_windows_plan.py).
// For every (F, stride), F in 16 .. 200, stride in 1 .. 40:
//   - every window belongs to exactly one segment, and the segments cover the windows in order;
//   - a segment's frame range holds all 16 frames of each of its windows, and no frame index reaches F;
//   - the lead-in a segment shares with its predecessor is at most 15 frames;
//   - the kernel's walk, replayed here on a ring of 32 slots exactly as dct_hash_windows_kernel does it (chunks of 16, slot = (f - run) & 31; strides
//     above 16 give every window a segment of its own, so a segment's frames are one contiguous walk), finds every frame of every window resident in its slot when the window is packed, and touches no frame
//     outside the segment's range;
//   - the window count is window_count's (printed: the Python side holds it against vdf_hash_window_count).
// Then the resize stage: the pseudo-clips of plan_windows_resize place every frame of every clip exactly where the kernel's address rule looks for it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "windows_plan.h"

using namespace vdf;

#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static int walk_segment(const WindowsPlan &p, uint32_t seg, std::vector<int> &owner)
{
    const uint32_t k_begin = p.first_window(seg), k_end = p.end_window(seg), f_end = p.frame_end(seg);
    CHECK(k_begin < k_end && k_end <= p.n_win);
    CHECK(f_end <= p.F && p.frame_begin(seg) < f_end);
    std::vector<long> ring(32, -1);  // which frame a slot holds
    const uint32_t run = k_begin * p.stride;
    uint32_t k = k_begin, have = run;
    size_t spatial = 0;
    while (k < k_end) {
        const uint32_t s = k * p.stride;
        CHECK(s <= have);  // one contiguous walk: a segment's windows are at most 16 frames apart (strides above 16: a segment per window)
        while (have < s + 16) {
            for (uint32_t t = 0; t < 16; t++) {
                const uint32_t f = have + t;
                if (f < f_end) {
                    CHECK(f >= p.frame_begin(seg) && f < p.F);
                    ring[(f - run) & 31u] = f;
                    spatial++;
                }
            }
            CHECK((have - run) % 16 == 0);  // chunks begin at slot 0 or 16
            have += 16;
        }
        const uint32_t k_ready = std::min<uint32_t>(k_end, (have - 16) / p.stride + 1);
        CHECK(k_ready > k);
        for (uint32_t kk = k; kk < k_ready; kk++) {
            for (uint32_t t = 0; t < 16; t++) {
                const uint32_t f = kk * p.stride + t;
                CHECK(f < f_end);
                CHECK(ring[(f - run) & 31u] == (long)f);
            }
            CHECK(owner[kk] == -1);
            owner[kk] = (int)seg;
        }
        k = k_ready;
    }
    CHECK(spatial == f_end - p.frame_begin(seg));  // every frame of the range once
    if (p.stride > 16) CHECK(k_end - k_begin == 1 && spatial == 16);  // ... which above stride 16 is the one window's own frames
    return 0;
}

static int check_resize(size_t n_clips, uint32_t F, size_t frame_stride, size_t clip_stride)
{
    const WindowsResizePlan r = plan_windows_resize(n_clips, F, frame_stride, clip_stride);
    const size_t none = (size_t)-1;
    std::vector<size_t> small(r.small_bytes / 256, none);  // 16 x 16 frame slot -> source frame (byte offset of the frame in the caller's buffer)
    size_t launches = 0;
    for (const WindowsResizeRun &run : windows_resize_runs(r, n_clips, F, frame_stride, clip_stride)) {  // the resize kernels: pseudo-clip i, frame f -> dst + 4096 i + 256 f
        launches++;
        for (size_t i = 0; i < run.n; i++)
            for (size_t f = 0; f < 16; f++) {
                const size_t at = (run.dst_offset + 4096 * i) / 256 + f;
                CHECK(at < small.size());
                small[at] = run.src_offset + i * run.step + f * frame_stride;
            }
    }
    CHECK(launches == r.launches && launches <= (size_t)F / 16 + 1);
    // the kernel's address rule (dct_hash.hip: WindowsSource) finds frame f of clip c, and no source frame lies outside the clips
    const uint32_t main_frames = 16 * r.n_chunks, tail_first = F - 16;
    for (size_t c = 0; c < n_clips; c++)
        for (uint32_t f = 0; f < F; f++) {
            const size_t at = f < main_frames ? c * r.clip_step + (size_t)(f >> 4) * r.chunk_step + (size_t)(f & 15) * 256
                                              : r.tail_offset + c * 4096 + (size_t)(f - tail_first) * 256;
            CHECK(at % 256 == 0 && at / 256 < small.size());
            CHECK(small[at / 256] == c * clip_stride + f * frame_stride);
        }
    for (size_t v : small) CHECK(v != none && v <= (n_clips - 1) * clip_stride + (size_t)(F - 1) * frame_stride);
    return 0;
}

int main()
{
    static_assert(kWindowSegFrames == 16 * kWindowSegChunks && kWindowSegChunks >= 1, "segment length");
    CHECK(window_count(15, 1) == 0 && window_count(16, 0) == 0 && window_count(16, 1) == 1 && window_count(0xFFFFFFFFu, 1) == 0xFFFFFFFFull - 15);
    size_t windows = 0, segments = 0;
    for (uint32_t F = 16; F <= 200; F++)
        for (uint32_t stride = 1; stride <= 40; stride++) {
            const WindowsPlan p = plan_windows(F, stride);
            CHECK(p.n_win == (F - 16) / stride + 1 && p.n_win == window_count(F, stride));
            std::printf("count %u %u %u\n", F, stride, p.n_win);
            CHECK(p.per_seg >= 1 && p.per_seg * stride <= std::max(kWindowSegFrames, stride));
            CHECK((uint64_t)p.n_seg * p.per_seg >= p.n_win && (uint64_t)(p.n_seg - 1) * p.per_seg < p.n_win);
            std::vector<int> owner(p.n_win, -1);
            for (uint32_t s = 0; s < p.n_seg; s++) {
                if (walk_segment(p, s, owner)) return 1;
                CHECK(p.lead_in(s) <= 15);
                CHECK(s == 0 || p.first_window(s) == p.end_window(s - 1));
                CHECK(p.frame_end(s) - p.frame_begin(s) <= kWindowSegFrames + 15 || p.per_seg == 1);
            }
            for (uint32_t k = 0; k < p.n_win; k++) {
                CHECK(owner[k] == (int)p.segment_of(k));  // exactly one segment packed it (walk_segment refuses a second), the one the map names
                const uint32_t s = p.segment_of(k);
                CHECK(p.frame_begin(s) <= k * stride && k * stride + 16 <= p.frame_end(s) && p.frame_end(s) <= F);
            }
            windows += p.n_win;
            segments += p.n_seg;
        }
    // a long clip is many workgroups, not one serial walk
    CHECK(plan_windows(7200, 1).n_seg == (7200 - 15 + 31) / 32);
    // the resize stage: packed and padded clips, few and many, with and without a tail
    for (uint32_t F : {16u, 17u, 31u, 32u, 33u, 35u, 48u, 100u})
        for (size_t n_clips : {size_t(1), size_t(2), size_t(3), size_t(7), size_t(40)})
            for (size_t pad : {size_t(0), size_t(3)})
                for (size_t clip_pad : {size_t(0), size_t(5)}) {
                    const size_t fs = 100 + pad;
                    if (check_resize(n_clips, F, fs, (size_t)F * fs + clip_pad)) return 1;
                }
    CHECK(plan_windows_resize(1000, 64, 4096, 64 * 4096).launches == 1);
    CHECK(plan_windows_resize(1000, 64, 4096, 64 * 4096 + 16).launches == 4);
    CHECK(plan_windows_resize(1, 7200, 100, 0).launches == 1 && plan_windows_resize(1, 7201, 100, 0).launches == 2);
    std::printf("windows plan ok: %zu windows in %zu segments\n", windows, segments);
    return 0;
}
