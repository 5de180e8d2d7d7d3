// Retimed window hashes of videos of DIFFERENT frame sizes and frame counts in one call (vdf_hash_windows_clips_u8_retimed[_device];
// DESIGN.md 4.18): windows_mixed_plan.h's library (one buffer, a descriptor and a frame count per video, rows first[i] + k) with
// windows_retimed_plan.h's windows (window k = frames k stride + tap(t), tap(t) = floor(t num / den)).  The two checks that come behind the plain
// mixed call's, first[] from the retimed window count, the segments of every video and the table a workgroup of
// dct_hash_windows_mixed_retimed_kernel finds its video in, and the one record per video it reads.  The resize stage is plan_windows_mixed's,
// called as it is: every frame once, as 16-frame pseudo-clips, whatever the taps read.  Host-only arithmetic (no HIP types), shared by api.cpp
// and the kernel in dct_hash.hip; tests/cpp/windows_mixed_retimed_plan_main.cpp enumerates it on the CPU and replays the ring.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "windows_mixed_plan.h"
#include "windows_retimed_plan.h"

namespace vdf {

// The checks behind check_windows_mixed's (which has passed: stride > 0, every n_frames >= 16), in the order their codes are reported.
enum class WindowsMixedRetimedError { kNone, kBadRate, kShorterThanSpan };
struct WindowsMixedRetimedCheck { WindowsMixedRetimedError error = WindowsMixedRetimedError::kNone; size_t video = 0; };

inline WindowsMixedRetimedCheck check_windows_mixed_retimed(const uint32_t *n_frames, size_t n, uint32_t num, uint32_t den)
{
    if (!retimed_rate_ok(num, den)) return {WindowsMixedRetimedError::kBadRate, 0};
    const uint32_t span = retimed_span(num, den);
    for (size_t i = 0; i < n; i++)
        if (n_frames[i] < span) return {WindowsMixedRetimedError::kShorterThanSpan, i};  // a library call returns no 0-window video: every video has a segment
    return {};
}

// first[i] = retimed windows of videos 0 .. i - 1; false: 2^32 windows or more (first is then unspecified).  The rate is one, stride > 0 and
// every n_frames >= span.  (The retimed count never exceeds the plain one, so a library check_windows_mixed has passed cannot fail here.)
inline bool windows_first_retimed(const uint32_t *n_frames, size_t n, uint32_t stride, uint32_t num, uint32_t den, uint32_t *first)
{
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        first[i] = (uint32_t)at;
        at += retimed_window_count(n_frames[i], stride, num, den);
        if (at > 0xFFFFFFFFull) return false;
    }
    first[n] = (uint32_t)at;
    return true;
}

struct WindowsMixedRetimedPlan {
    // kPlain: the taps are 0 ... 15 - the plain mixed call, its route and its words (nothing else of this plan is filled in)
    // kUniform: plan_windows_mixed's uniform rule - the uniform retimed call on (base + offset0, clip_stride)
    // kMixed: dct_hash_windows_mixed_retimed_kernel on `small`
    enum Kind { kPlain, kUniform, kMixed } kind = kMixed;
    uint64_t offset0 = 0, clip_stride = 0;
    WindowsRetimedPlan rate;                 // span and taps (its F, n_win and n_seg are those of video 0: the uniform route's)
    uint32_t per_seg = 0;                    // windows per segment: max(1, 32 / stride), the same for every video
    std::vector<uint32_t> first, seg_first;  // [n_videos + 1]; seg_first strictly ascending
    // kMixed: plan_windows_mixed's resize stage, and its records with n_win, first and seg_first the retimed ones
    std::vector<MixedClipDesc> descs;
    std::vector<MixedLaunch> launches;
    std::vector<WindowsVideoRecord> videos;
    uint32_t max_w = 0, max_h = 0;
    size_t small_bytes = 0;
};

// the videos have passed check_windows_mixed and check_windows_mixed_retimed
inline WindowsMixedRetimedPlan plan_windows_mixed_retimed(const MixedClip *clips, const uint32_t *n_frames, size_t n, uint32_t stride, uint32_t num, uint32_t den)
{
    WindowsMixedRetimedPlan p;
    p.first.assign(n + 1, 0);
    p.seg_first.assign(n + 1, 0);
    if (retimed_is_plain(num, den)) {
        p.kind = WindowsMixedRetimedPlan::kPlain;
        return p;
    }
    if (n == 0) return p;
    p.rate = plan_windows_retimed(n_frames[0], stride, num, den);
    p.per_seg = p.rate.per_seg;
    windows_first_retimed(n_frames, n, stride, num, den, p.first.data());
    for (size_t i = 0; i < n; i++)  // (at most one segment per window: below 2^32)
        p.seg_first[i + 1] = p.seg_first[i] + plan_windows_retimed(n_frames[i], stride, num, den).n_seg;
    // The resize stage does not know the rate: plan_windows_mixed's pseudo-clips, parts and launches as they are, and its uniform rule.
    WindowsMixedPlan m = plan_windows_mixed(clips, n_frames, n, stride);
    if (m.kind == WindowsMixedPlan::kUniform) {
        p.kind = WindowsMixedRetimedPlan::kUniform;
        p.offset0 = m.offset0;
        p.clip_stride = m.clip_stride;
        return p;
    }
    p.descs = std::move(m.descs);
    p.launches = std::move(m.launches);
    p.videos = std::move(m.videos);
    p.max_w = m.max_w;
    p.max_h = m.max_h;
    p.small_bytes = m.small_bytes;
    for (size_t i = 0; i < n; i++) {  // slot0, main_frames and tail_first stay: where a frame is does not depend on which windows read it
        WindowsVideoRecord &v = p.videos[i];
        v.n_win = p.first[i + 1] - p.first[i];
        v.first = p.first[i];
        v.seg_first = p.seg_first[i];
    }
    return p;
}

}  // namespace vdf
