// The planner behind vdf_hash_windows_u8_rates[_device] (csrc/windows_rates_plan.h) enumerated on the CPU, under -fsanitize=address,undefined:
// every F in 16 .. 140 x stride {1, 2, 3, 16, 17, 40} x every non-empty subset of {1/1, 6/5, 5/4, 3/2, 31/16, 2/1}, plus one list of 8 rates with
// a duplicate and an unreduced one.  Checked per case: taps, span, n_win and the rate-major out_first against their definitions; and a replay of
// dct_hash_windows_rates_kernel's walk with the header's own functions (chunks of 16 frames into the ring of kRetimedRingSlots slots while
// have < f_end; behind each chunk, rate by rate, the windows [max(k_begin, ready(have - 16)), min(k_end_r, ready(have)))):
//   - every window of every rate is hashed exactly once, by the segment that owns it;
//   - every tap of a window is resident in its slot of the ring when pass t reads it - the slot holds THAT frame, not a later one;
//   - the ring argument of the kernel's header: a window hashed behind the chunk ending at `have` starts above have - 47;
//   - no frame at or past f_end is touched, f_end <= F, and a segment walks at most 62 frames;
//   - no rate is hashed while have < span_r (the difference would wrap around).
// Prints "first F stride n_clips r0,r1,.. out_first.. total" for the cases the test holds against the library's vdf_hash_window_count_rates, and
// "windows rates plan ok".
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "windows_rates_plan.h"

using namespace vdf;

#define CHECK(c)                                                                                              \
    do {                                                                                                      \
        if (!(c)) {                                                                                           \
            std::printf("FAILED %s (line %d): F %u stride %u rates %u\n", #c, __LINE__, F, stride, n_rates); \
            return 1;                                                                                         \
        }                                                                                                     \
    } while (0)

static int one(uint32_t F, uint32_t stride, uint32_t n_rates, const uint32_t *num, const uint32_t *den, size_t n_clips, bool print)
{
    const WindowsRatesPlan p = plan_windows_rates(n_clips, F, stride, n_rates, num, den);
    bool fits = true;
    for (uint32_t r = 0; r < n_rates; r++) fits = fits && retimed_window_count(F, stride, num[r], den[r]) > 0;
    CHECK(p.ok == fits);
    if (!p.ok) return 0;
    CHECK(p.a.n_rates == n_rates);
    uint32_t tap[kWindowsMaxRates][16], max_n = 0;
    uint64_t first = 0;
    for (uint32_t r = 0; r < n_rates; r++) {
        for (uint32_t i = 0; i < 16; i++) {
            tap[r][i] = (uint32_t)(((uint64_t)i * num[r]) / den[r]);
            CHECK(((i < 8 ? p.a.taps_lo[r] : p.a.taps_hi[r]) >> (8 * (i & 7)) & 255u) == tap[r][i]);
        }
        CHECK(p.a.span[r] == tap[r][15] + 1);
        uint32_t n = 0;
        while ((uint64_t)n * stride + p.a.span[r] <= F) n++;
        CHECK(p.a.n_win[r] == n && n == retimed_window_count(F, stride, num[r], den[r]));
        CHECK(p.a.out_first[r] == first);
        first += (uint64_t)n_clips * n;
        max_n = std::max(max_n, n);
    }
    CHECK(p.n_out == first && p.max_n_win == max_n);
    CHECK(p.per_seg == std::max<uint32_t>(1, kWindowSegFrames / stride) && p.n_seg == (max_n + p.per_seg - 1) / p.per_seg);
    CHECK(rates_groups(3, p) == 3ull * p.n_seg);
    if (print) {
        std::printf("first %u %u %zu ", F, stride, n_clips);
        for (uint32_t r = 0; r < n_rates; r++) std::printf("%s%u/%u", r ? "," : "", num[r], den[r]);
        for (uint32_t r = 0; r < n_rates; r++) std::printf(" %llu", (unsigned long long)p.a.out_first[r]);
        std::printf(" %llu\n", (unsigned long long)p.n_out);
    }
    std::vector<std::vector<uint32_t>> hashed(n_rates);
    for (uint32_t r = 0; r < n_rates; r++) hashed[r].assign(p.a.n_win[r], 0);
    for (uint32_t s = 0; s < p.n_seg; s++) {
        const uint32_t k_begin = p.first_window(s), run = p.frame_begin(s), f_end = p.frame_end(s);
        bool any = false;
        for (uint32_t r = 0; r < n_rates; r++) {
            any = any || p.owns(s, r);
            if (p.owns(s, r)) CHECK((p.end_window(s, r) - 1) * stride + p.a.span[r] <= f_end);
        }
        CHECK(any && f_end <= F && f_end > run && f_end - run <= 62);
        // ---- the kernel's walk: what each slot of the ring holds
        std::vector<int64_t> ring(kRetimedRingSlots, -1);
        uint32_t have = run;
        while (have < f_end) {
            for (uint32_t t = 0; t < 16; t++)
                if (have + t < f_end) {
                    CHECK(have + t < F);
                    ring[retimed_slot(have + t, run)] = have + t;
                }
            have += 16;
            for (uint32_t r = 0; r < n_rates; r++) {
                const uint32_t span = p.a.span[r];
                const uint32_t k_end = p.end_window(s, r);
                const uint32_t k_from = std::max(k_begin, rates_windows_ready(have - 16, span, stride));
                const uint32_t k_ready = std::min(k_end, rates_windows_ready(have, span, stride));
                if (have < span) CHECK(k_ready == 0 && rates_windows_ready(have, span, stride) == 0);
                for (uint32_t kk = k_from; kk < k_ready; kk++) {
                    CHECK(kk >= k_begin && kk < k_end && kk < p.a.n_win[r] && kk / p.per_seg == s);
                    CHECK(have >= span && (uint64_t)kk * stride + span <= have);
                    CHECK(kk * stride + 47 > have);  // the ring argument: not whole one chunk ago
                    hashed[r][kk]++;
                    for (uint32_t i = 0; i < 16; i++) {
                        const uint32_t s0 = kk * stride - run;  // as the kernel forms the slot: (s0 + tap) & 63
                        CHECK(kk * stride + tap[r][i] < f_end);
                        CHECK(ring[(s0 + tap[r][i]) & (kRetimedRingSlots - 1)] == (int64_t)(kk * stride + tap[r][i]));
                    }
                }
            }
        }
        // behind the walk every window of the segment has been hashed
        for (uint32_t r = 0; r < n_rates; r++)
            for (uint32_t kk = k_begin; kk < p.end_window(s, r); kk++) CHECK(hashed[r][kk] == 1);
    }
    for (uint32_t r = 0; r < n_rates; r++)
        for (uint32_t kk = 0; kk < p.a.n_win[r]; kk++) CHECK(hashed[r][kk] == 1);
    return 0;
}

int main()
{
    const uint32_t base[6][2] = {{1, 1}, {6, 5}, {5, 4}, {3, 2}, {31, 16}, {2, 1}};
    const uint32_t strides[] = {1, 2, 3, 16, 17, 40};
    const uint32_t eight_num[8] = {2, 1, 6, 3, 5, 12, 31, 2}, eight_den[8] = {1, 1, 5, 2, 4, 10, 16, 1};
    for (uint32_t F = 16; F <= 140; F++)
        for (uint32_t stride : strides) {
            for (uint32_t mask = 1; mask < 64; mask++) {
                uint32_t num[6], den[6], n = 0;
                for (uint32_t b = 0; b < 6; b++)
                    if (mask >> b & 1) { num[n] = base[b][0]; den[n] = base[b][1]; n++; }
                // (the library is asked about a sample of them: the full lists, and the pairs of 1/1 with one other rate)
                const bool print = F % 9 == 2 && (mask == 63 || (mask & 1 && __builtin_popcount(mask) == 2));
                if (one(F, stride, n, num, den, 3, print)) return 1;
            }
            if (one(F, stride, 8, eight_num, eight_den, 5, F % 9 == 2)) return 1;
            // the rates in descending span: the first listed rate is not the one with the most windows
            const uint32_t dn[3] = {2, 3, 1}, dd[3] = {1, 2, 1};
            if (one(F, stride, 3, dn, dd, 2, false)) return 1;
        }
    // lists the planner refuses
    const uint32_t bn[2] = {1, 5}, bd[2] = {1, 2}, nine[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
    if (plan_windows_rates(1, 100, 1, 0, bn, bd).ok || plan_windows_rates(1, 100, 1, 2, bn, bd).ok || plan_windows_rates(1, 100, 1, 9, nine, nine).ok ||
        plan_windows_rates(1, 100, 1, 1, nullptr, bd).ok || plan_windows_rates(1, 100, 0, 1, bn, bd).ok || !plan_windows_rates(1, 100, 1, 8, nine, nine).ok ||
        rates_windows_ready(16, 31, 1) != 0 || rates_windows_ready(31, 31, 1) != 1 || rates_windows_ready(47, 31, 3) != 6) {
        std::printf("FAILED the refused lists\n");
        return 1;
    }
    std::printf("windows rates plan ok\n");
    return 0;
}
