// Retimed window hashes of videos of DIFFERENT frame sizes and frame counts at SEVERAL rates in one call (vdf_hash_windows_clips_u8_rates[_device];
// DESIGN.md 4.21): windows_mixed_retimed_plan.h's library (one buffer, a descriptor and a frame count per video) with windows_rates_plan.h's list of
// rates (one read, one resize and one spatial transform of every frame; only pass t depends on the rate).  The checks that come behind the plain
// mixed call's, first[] and rate_first[] (rate-major: every block is a library the align calls read), what the kernel takes per rate, the segments of
// every video - by window START over the rate with the most windows, as the uniform rates call - the table a workgroup of
// dct_hash_windows_mixed_rates_kernel finds its video in, and the table of output rows row0[r n_videos + i].  The resize stage and the uniform rule
// are plan_windows_mixed's, called as it is.  Host-only arithmetic (no HIP types), shared by api.cpp and the kernel in dct_hash.hip;
// tests/cpp/windows_mixed_rates_plan_main.cpp enumerates it on the CPU and replays the ring.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "windows_mixed_plan.h"
#include "windows_mixed_retimed_plan.h"
#include "windows_rates_plan.h"

namespace vdf {

// The kernel's by-value argument: what differs between the rates and not between the videos (WindowsRatesArgs without n_win and out_first, which
// are per video here: n_win_r = (F_v - span_r) / stride + 1, the row from row0).  Indexed by the workgroup-uniform rate r: scalar loads.
struct WindowsMixedRatesArgs {
    uint64_t taps_lo[kWindowsMaxRates] = {}, taps_hi[kWindowsMaxRates] = {};  // as WindowsRetimedPlan's: tap(i) in byte i & 7
    uint32_t span[kWindowsMaxRates] = {};
    uint32_t n_rates = 0;
};

// The checks behind check_windows_mixed's (which has passed: stride > 0, every n_frames >= 16), in the order their codes are reported.
enum class WindowsMixedRatesError { kNone, kRateCount, kBadRate, kShorterThanSpan, kTooManyRows };
struct WindowsMixedRatesCheck { WindowsMixedRatesError error = WindowsMixedRatesError::kNone; uint32_t rate = 0; size_t video = 0; };

inline WindowsMixedRatesCheck check_windows_mixed_rates(const uint32_t *n_frames, size_t n, uint32_t stride, uint32_t n_rates, const uint32_t *num,
                                                        const uint32_t *den)
{
    if (n_rates < 1 || n_rates > kWindowsMaxRates || !num || !den) return {WindowsMixedRatesError::kRateCount, 0, 0};
    for (uint32_t r = 0; r < n_rates; r++)
        if (!retimed_rate_ok(num[r], den[r])) return {WindowsMixedRatesError::kBadRate, r, 0};
    for (uint32_t r = 0; r < n_rates; r++) {  // in list order: the first rate some video is too short for, and the first such video
        const WindowsMixedRetimedCheck one = check_windows_mixed_retimed(n_frames, n, num[r], den[r]);
        if (one.error != WindowsMixedRetimedError::kNone) return {WindowsMixedRatesError::kShorterThanSpan, r, one.video};
    }
    uint64_t rows = 0;
    for (uint32_t r = 0; r < n_rates; r++)
        for (size_t i = 0; i < n; i++) {
            rows += retimed_window_count(n_frames[i], stride, num[r], den[r]);  // (at most 2^32 a video: no wrap before the test)
            if (rows > 0xFFFFFFFFull) return {WindowsMixedRatesError::kTooManyRows, r, i};
        }
    return {};
}

// first[r (n + 1) + i] = windows_first_retimed at rate r (the retimed windows of videos 0 .. i - 1); rate_first[r] (nullable, n_rates + 1 entries) =
// the rows of the blocks before r, the last entry the total.  false: 2^32 rows or more in all (the arrays are then unspecified).  The rates are ones
// the calls take, 1 <= n_rates <= kWindowsMaxRates, stride > 0.
inline bool windows_first_rates(const uint32_t *n_frames, size_t n, uint32_t stride, uint32_t n_rates, const uint32_t *num, const uint32_t *den,
                                uint32_t *first, uint64_t *rate_first)
{
    uint64_t at = 0;
    for (uint32_t r = 0; r < n_rates; r++) {
        uint32_t *row = first + (size_t)r * (n + 1);
        if (!windows_first_retimed(n_frames, n, stride, num[r], den[r], row)) return false;
        if (rate_first) rate_first[r] = at;
        at += row[n];
        if (at > 0xFFFFFFFFull) return false;
    }
    if (rate_first) rate_first[n_rates] = at;
    return true;
}

struct WindowsMixedRatesPlan {
    // kUniform: plan_windows_mixed's uniform rule - the uniform rates call on (base + offset0, clip_stride), whose rows coincide: first[r][c] = c n_win_r
    // kMixed: dct_hash_windows_mixed_rates_kernel on `small` - everything else, a one-rate list and plain-tap rates included
    enum Kind { kUniform, kMixed } kind = kMixed;
    uint64_t offset0 = 0, clip_stride = 0;
    WindowsRatesPlan uniform;                // kUniform: plan_windows_rates of (n_videos, n_frames[0])
    uint32_t stride = 0;
    WindowsMixedRatesArgs a;
    uint32_t per_seg = 0;                    // window STARTS per segment: max(1, 32 / stride), the same for every video and rate
    std::vector<uint32_t> first;             // [n_rates][n_videos + 1]
    std::vector<uint64_t> rate_first;        // [n_rates + 1]; the last entry, the total, is below 2^32
    std::vector<uint32_t> seg_first;         // [n_videos + 1], strictly ascending: n_seg_i = ceil(max_r n_win_r(i) / per_seg)
    std::vector<uint32_t> row0;              // [n_rates][n_videos]: rate_first[r] + first[r][i], the row of window 0 of video i at rate r
    // kMixed: plan_windows_mixed's resize stage, and its records with n_win = max_r n_win_r(i) (what the segments are cut from), first = row0[0][i]
    // and seg_first the ones above.  The kernel takes the video's frame count from the record as it is: F = tail_first + 16 (reserved stays 0).
    std::vector<MixedClipDesc> descs;
    std::vector<MixedLaunch> launches;
    std::vector<WindowsVideoRecord> videos;
    uint32_t max_w = 0, max_h = 0;
    size_t small_bytes = 0;

    uint32_t n_win(uint32_t r, size_t i) const { return first[(size_t)r * seg_first.size() + i + 1] - first[(size_t)r * seg_first.size() + i]; }
    // segment s of video i serves, of rate r, the windows [first_window(s), end_window(s, r, i)): none if that is empty (long spans, last segments)
    uint32_t first_window(uint32_t s) const { return s * per_seg; }
    uint32_t end_window(uint32_t s, uint32_t r, size_t i) const { return (uint32_t)std::min<uint64_t>((uint64_t)(s + 1) * per_seg, n_win(r, i)); }
    bool owns(uint32_t s, uint32_t r, size_t i) const { return end_window(s, r, i) > first_window(s); }
    // the frames the segment's workgroup walks: one contiguous run to the last tap of the rates that own a window in it, never past F_i
    uint32_t frame_begin(uint32_t s) const { return (uint32_t)((uint64_t)first_window(s) * stride); }
    uint32_t frame_end(uint32_t s, size_t i) const
    {
        uint32_t e = 0;
        for (uint32_t r = 0; r < a.n_rates; r++)
            if (owns(s, r, i)) e = std::max(e, (uint32_t)((uint64_t)(end_window(s, r, i) - 1) * stride + a.span[r]));
        return e;
    }
};

// The frame count of a video as the kernel takes it from the record plan_windows_mixed wrote.
VDF_WINDOWS_MIXED_HD uint32_t windows_mixed_rates_frames(const WindowsVideoRecord &v) { return v.tail_first + kWindowFrames; }

// the videos have passed check_windows_mixed and check_windows_mixed_rates
inline WindowsMixedRatesPlan plan_windows_mixed_rates(const MixedClip *clips, const uint32_t *n_frames, size_t n, uint32_t stride, uint32_t n_rates,
                                                      const uint32_t *num, const uint32_t *den)
{
    WindowsMixedRatesPlan p;
    p.stride = stride;
    p.a.n_rates = n_rates;
    p.first.assign((size_t)n_rates * (n + 1), 0);
    p.rate_first.assign((size_t)n_rates + 1, 0);
    p.seg_first.assign(n + 1, 0);
    p.per_seg = std::max<uint32_t>(1, kWindowSegFrames / stride);
    for (uint32_t r = 0; r < n_rates; r++) {
        const WindowsRetimedPlan one = plan_windows_retimed(n ? n_frames[0] : 0, stride, num[r], den[r]);  // (taps and span do not depend on F)
        p.a.taps_lo[r] = one.taps_lo;
        p.a.taps_hi[r] = one.taps_hi;
        p.a.span[r] = one.span;
    }
    if (n == 0) return p;
    windows_first_rates(n_frames, n, stride, n_rates, num, den, p.first.data(), p.rate_first.data());
    p.row0.resize((size_t)n_rates * n);
    for (uint32_t r = 0; r < n_rates; r++)
        for (size_t i = 0; i < n; i++) p.row0[(size_t)r * n + i] = (uint32_t)(p.rate_first[r] + p.first[(size_t)r * (n + 1) + i]);
    std::vector<uint32_t> max_win(n, 0);
    for (size_t i = 0; i < n; i++) {
        for (uint32_t r = 0; r < n_rates; r++) max_win[i] = std::max(max_win[i], p.n_win(r, i));
        p.seg_first[i + 1] = p.seg_first[i] + (max_win[i] + p.per_seg - 1) / p.per_seg;  // (at most one segment per window of one rate: below 2^32)
    }
    // The resize stage does not know the rates: plan_windows_mixed's pseudo-clips, parts and launches as they are, and its uniform rule.
    WindowsMixedPlan m = plan_windows_mixed(clips, n_frames, n, stride);
    if (m.kind == WindowsMixedPlan::kUniform) {
        p.kind = WindowsMixedRatesPlan::kUniform;
        p.offset0 = m.offset0;
        p.clip_stride = m.clip_stride;
        p.uniform = plan_windows_rates(n, n_frames[0], stride, n_rates, num, den);
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
        v.n_win = max_win[i];
        v.first = p.row0[i];
        v.seg_first = p.seg_first[i];
    }
    return p;
}

}  // namespace vdf
