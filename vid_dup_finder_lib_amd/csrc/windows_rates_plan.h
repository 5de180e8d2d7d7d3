// Retimed window hashes at several rates from one read of the frames (vdf_hash_windows_u8_rates[_device]): only pass t of a
// retimed window depends on its rate, so one workgroup of dct_hash_windows_rates_kernel walks a segment's frames once - one resize, one pair of
// spatial passes per frame - and hashes from its ring the windows of up to kWindowsMaxRates rates.  What the kernel takes per rate (taps, span,
// window count, first output row), which windows of which rate a workgroup serves, and which frames it walks for them.  Host-only arithmetic (no
// HIP), on top of windows_retimed_plan.h, shared by api.cpp and the launcher in dct_hash.hip; tests/cpp/windows_rates_plan_main.cpp enumerates it
// on the CPU and replays the ring.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "windows_retimed_plan.h"

namespace vdf {

constexpr uint32_t kWindowsMaxRates = 8;  // = VDF_WINDOWS_MAX_RATES

// The kernel's by-value argument: what differs between the rates.  Indexed by the workgroup-uniform rate r, so every read is a scalar load.
struct WindowsRatesArgs {
    uint64_t taps_lo[kWindowsMaxRates] = {}, taps_hi[kWindowsMaxRates] = {};  // as WindowsRetimedPlan's: tap(i) in byte i & 7
    uint64_t out_first[kWindowsMaxRates] = {};  // rate-major: the row of window 0 of clip 0 at rate r = n_clips * (n_win of the rates before r)
    uint32_t span[kWindowsMaxRates] = {};
    uint32_t n_win[kWindowsMaxRates] = {};      // windows per clip at rate r
    uint32_t n_rates = 0;
};

struct WindowsRatesPlan {
    uint32_t F = 0, stride = 0;
    bool ok = false;         // 1 <= n_rates <= kWindowsMaxRates, every rate one the calls take and F >= its span
    WindowsRatesArgs a;
    uint64_t n_out = 0;      // rows of all rates: n_clips * the sum of n_win
    uint32_t max_n_win = 0;
    uint32_t per_seg = 0;    // window STARTS per segment, as WindowsRetimedPlan's
    uint32_t n_seg = 0;      // segments (= workgroups) per clip: of the rate with the most windows
    // segment s serves, of rate r, the windows [first_window(s), end_window(s, r)): none if that is empty (long spans, last segments)
    uint32_t first_window(uint32_t s) const { return s * per_seg; }
    uint32_t end_window(uint32_t s, uint32_t r) const { return (uint32_t)std::min<uint64_t>((uint64_t)(s + 1) * per_seg, a.n_win[r]); }
    bool owns(uint32_t s, uint32_t r) const { return end_window(s, r) > first_window(s); }
    // the frames the segment's workgroup walks: one contiguous run of at most 31 + 31 = 62 frames, to the last tap of the rates that own a window
    uint32_t frame_begin(uint32_t s) const { return (uint32_t)((uint64_t)first_window(s) * stride); }
    uint32_t frame_end(uint32_t s) const
    {
        uint32_t e = 0;
        for (uint32_t r = 0; r < a.n_rates; r++)
            if (owns(s, r)) e = std::max(e, (uint32_t)((uint64_t)(end_window(s, r) - 1) * stride + a.span[r]));
        return e;
    }
};

// Duplicate and unreduced rates are taken as they come: the taps depend only on the quotient, and every listed rate gets its block of rows.
inline WindowsRatesPlan plan_windows_rates(size_t n_clips, uint32_t F, uint32_t stride, uint32_t n_rates, const uint32_t *num, const uint32_t *den)
{
    WindowsRatesPlan p;
    p.F = F;
    p.stride = stride;
    if (n_rates < 1 || n_rates > kWindowsMaxRates || !num || !den || stride == 0) return p;
    p.a.n_rates = n_rates;
    for (uint32_t r = 0; r < n_rates; r++) {
        const WindowsRetimedPlan one = plan_windows_retimed(F, stride, num[r], den[r]);
        if (!retimed_rate_ok(num[r], den[r]) || one.n_win == 0) return p;
        p.a.taps_lo[r] = one.taps_lo;
        p.a.taps_hi[r] = one.taps_hi;
        p.a.span[r] = one.span;
        p.a.n_win[r] = one.n_win;
        p.a.out_first[r] = p.n_out;
        p.n_out += (uint64_t)n_clips * one.n_win;  // < 2^64 / 8 a rate: n_clips * n_win < 2^32 is windows_checks'
        p.max_n_win = std::max(p.max_n_win, one.n_win);
    }
    p.per_seg = std::max<uint32_t>(1, kWindowSegFrames / stride);
    p.n_seg = (p.max_n_win + p.per_seg - 1) / p.per_seg;
    p.ok = true;
    return p;
}

// The kernel's walk, in the planner's words (the kernel uses this function; the replay in tests/cpp/windows_rates_plan_main.cpp as well): with
// frames [.., have) loaded, the windows k of a rate with k * stride + span <= have are whole - NONE while have < span, where have - span would
// wrap around (a span above 16 on a clip's first chunk).  After the chunk that ends at `have` the workgroup hashes, of each rate, the windows
// [max(k_begin, ready(have - 16)), min(k_end_r, ready(have))): its cursor is the count that was ready one chunk ago, no state per rate.
constexpr uint32_t rates_windows_ready(uint32_t have, uint32_t span, uint32_t stride) { return have < span ? 0u : (have - span) / stride + 1; }

inline uint64_t rates_groups(size_t n_clips, const WindowsRatesPlan &p) { return (uint64_t)n_clips * p.n_seg; }

}  // namespace vdf
