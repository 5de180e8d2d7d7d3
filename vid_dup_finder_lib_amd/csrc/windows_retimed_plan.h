// Retimed window hashes (vdf_hash_windows_u8_retimed[_device]): the windows of a clip sampled at a rate num / den of its own
// frames - window k = the 16 frames k * stride + tap(i), tap(i) = floor(i * num / den) - so that a copy at another frame rate or speed has windows
// that hold the same pictures.  The taps, the window count, which windows a workgroup of dct_hash_windows_retimed_kernel serves, which frames it
// walks for them, and the size of its ring.  Host-only arithmetic (no HIP), shared by api.cpp and the launcher in dct_hash.hip;
// tests/cpp/windows_retimed_plan_main.cpp enumerates it on the CPU and replays the ring.  The resize stage is windows_plan.h's, unchanged.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "windows_plan.h"

namespace vdf {

constexpr uint32_t kRetimedMaxNum = 65535;
// The kernel's ring of spatially transformed frames.  It loads chunks of 16 frames until the window in hand is whole: have >= s + span, and
// have < s + span + 16 <= s + 47 since the chunk before was still needed.  The window's first frame s must still be resident, s >= have - slots:
// 48 slots would do, 64 keep `& 63` and chunks at slot 0 / 16 / 32 / 48 (dct_hash_block's bank pattern).
constexpr uint32_t kRetimedRingSlots = 64;

// a rate the calls take: 1 <= den <= num <= 2 den, num <= 65535 (rates below 1 would repeat frames: retime the side with more frames per second)
constexpr bool retimed_rate_ok(uint32_t num, uint32_t den) { return den >= 1 && num >= den && num <= 2 * (uint64_t)den && num <= kRetimedMaxNum; }
constexpr uint32_t retimed_tap(uint32_t i, uint32_t num, uint32_t den) { return i * num / den; }  // i <= 15, num <= 65535: below 2^20
constexpr uint32_t retimed_span(uint32_t num, uint32_t den) { return retimed_tap(kWindowFrames - 1, num, den) + 1; }  // 16 ... 31
// the taps are 0 ... 15: the plain windows (num == den, and every rate below 16 / 15)
constexpr bool retimed_is_plain(uint32_t num, uint32_t den) { return retimed_span(num, den) == kWindowFrames; }
// windows of a clip of F frames: window k = frames k * stride + tap(i); 0 if F < span, stride == 0 or the rate is not one
constexpr size_t retimed_window_count(uint32_t F, uint32_t stride, uint32_t num, uint32_t den)
{
    return (!retimed_rate_ok(num, den) || stride == 0 || F < retimed_span(num, den)) ? 0 : (size_t)(F - retimed_span(num, den)) / stride + 1;
}

struct WindowsRetimedPlan {
    uint32_t F = 0, stride = 0, num = 1, den = 1;
    uint32_t span = kWindowFrames;
    uint8_t tap[kWindowFrames] = {};
    uint64_t taps_lo = 0, taps_hi = 0;  // the taps as the kernel takes them: tap(i) in byte i & 7 of taps_lo (i < 8) / taps_hi
    uint32_t n_win = 0;     // windows per clip
    uint32_t per_seg = 0;   // windows per segment (the last of a clip may hold fewer): as many as start within kWindowSegFrames frames, as WindowsPlan
    uint32_t n_seg = 0;     // segments (= workgroups) per clip
    uint32_t first_window(uint32_t s) const { return s * per_seg; }
    uint32_t end_window(uint32_t s) const { return (uint32_t)std::min<uint64_t>((uint64_t)(s + 1) * per_seg, n_win); }
    uint32_t segment_of(uint32_t k) const { return k / per_seg; }
    // the frames the segment's workgroup walks: [frame_begin, frame_end), one contiguous run - frames between the taps included, they are
    // transformed and not read by pass t - of at most 31 + span <= 62 frames
    uint32_t frame_begin(uint32_t s) const { return (uint32_t)((uint64_t)first_window(s) * stride); }
    uint32_t frame_end(uint32_t s) const { return (uint32_t)((uint64_t)(end_window(s) - 1) * stride + span); }
};

inline WindowsRetimedPlan plan_windows_retimed(uint32_t F, uint32_t stride, uint32_t num, uint32_t den)
{
    WindowsRetimedPlan p;
    p.F = F;
    p.stride = stride;
    if (!retimed_rate_ok(num, den)) return p;
    p.num = num;
    p.den = den;
    p.span = retimed_span(num, den);
    for (uint32_t i = 0; i < kWindowFrames; i++) {
        p.tap[i] = (uint8_t)retimed_tap(i, num, den);
        (i < 8 ? p.taps_lo : p.taps_hi) |= (uint64_t)p.tap[i] << (8 * (i & 7));
    }
    p.n_win = (uint32_t)retimed_window_count(F, stride, num, den);  // < 2^32: at most F - 15
    if (p.n_win == 0) return p;
    p.per_seg = std::max<uint32_t>(1, kWindowSegFrames / stride);
    p.n_seg = (p.n_win + p.per_seg - 1) / p.per_seg;
    return p;
}

// The kernel's walk, in the planner's words (the kernel repeats these two lines; the replay in tests/cpp/windows_retimed_plan_main.cpp uses them):
// with frames [.., have) loaded, the windows k with k * stride + span <= have are whole (have >= span)
constexpr uint32_t retimed_windows_ready(uint32_t have, uint32_t span, uint32_t stride) { return (have - span) / stride + 1; }
// frame f of a segment that starts at frame `run` lives in this slot of the ring
constexpr uint32_t retimed_slot(uint32_t f, uint32_t run) { return (f - run) & (kRetimedRingSlots - 1); }

// grid cuts: launches of at most kMaxWindowGroupsPerLaunch workgroups over the n_clips * n_seg groups, as the plain call's
inline uint64_t retimed_groups(size_t n_clips, const WindowsRetimedPlan &p) { return (uint64_t)n_clips * p.n_seg; }
inline uint32_t retimed_grid(uint64_t groups, uint64_t first_group) { return (uint32_t)std::min<uint64_t>(kMaxWindowGroupsPerLaunch, groups - first_group); }

}  // namespace vdf
