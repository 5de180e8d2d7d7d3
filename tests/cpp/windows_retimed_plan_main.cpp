// The planner behind vdf_hash_windows_u8_retimed[_device] (csrc/windows_retimed_plan.h) enumerated on the CPU, under -fsanitize=address,undefined:
// every F in 16 .. 130 x stride 1 .. 40 x rate {1/1, 25/24, 6/5, 5/4, 3/2, 31/16, 2/1}.  Checked: the window count against its definition; the
// segments tile the windows; a segment's frame walk holds every tap of each of its windows and no frame >= F; and a replay of the kernel's walk
// (chunks of 16 frames into the ring of kRetimedRingSlots slots, windows hashed as soon as they are whole) finds every tap of every window
// resident in its slot when pass t reads it - the slot holds THAT frame, not a later one that overwrote it.
// Prints "count F stride num den n" per case (the test holds them against the library's vdf_hash_window_count_retimed) and "windows retimed plan ok".
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "windows_retimed_plan.h"

using namespace vdf;

#define CHECK(c)                                                                                                       \
    do {                                                                                                               \
        if (!(c)) {                                                                                                    \
            std::printf("FAILED %s (line %d): F %u stride %u rate %u/%u\n", #c, __LINE__, F, stride, num, den);      \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

static int one(uint32_t F, uint32_t stride, uint32_t num, uint32_t den)
{
    const WindowsRetimedPlan p = plan_windows_retimed(F, stride, num, den);
    // taps and span by the definition, in 64-bit
    uint32_t tap[16];
    for (uint32_t i = 0; i < 16; i++) {
        tap[i] = (uint32_t)(((uint64_t)i * num) / den);
        CHECK(p.tap[i] == tap[i]);
        CHECK(((i < 8 ? p.taps_lo : p.taps_hi) >> (8 * (i & 7)) & 255u) == tap[i]);
        CHECK(i == 0 || (tap[i] > tap[i - 1] && tap[i] <= tap[i - 1] + 2));
    }
    const uint32_t span = tap[15] + 1;
    CHECK(p.span == span && span >= 16 && span <= 31);
    CHECK(retimed_is_plain(num, den) == (span == 16));
    uint32_t n = 0;
    while ((uint64_t)n * stride + span <= F) n++;  // windows whose last tap is a frame of the clip
    CHECK(p.n_win == n && retimed_window_count(F, stride, num, den) == n);
    std::printf("count %u %u %u %u %u\n", F, stride, num, den, n);
    if (n == 0) return 0;
    CHECK(p.per_seg >= 1 && p.n_seg >= 1);
    CHECK(retimed_groups(3, p) == 3ull * p.n_seg && retimed_grid(retimed_groups(3, p), 0) == 3 * p.n_seg);
    uint32_t next = 0;
    for (uint32_t s = 0; s < p.n_seg; s++) {
        const uint32_t k0 = p.first_window(s), k1 = p.end_window(s);
        CHECK(k0 == next && k1 > k0 && k1 <= n);
        next = k1;
        const uint32_t f0 = p.frame_begin(s), f1 = p.frame_end(s);
        CHECK(f1 <= F && f0 < f1 && f1 - f0 <= 31 + span);
        for (uint32_t k = k0; k < k1; k++) {
            CHECK(p.segment_of(k) == s);
            for (uint32_t i = 0; i < 16; i++) CHECK(k * stride + tap[i] >= f0 && k * stride + tap[i] < f1);
        }
        // ---- the kernel's walk: what each slot of the ring holds
        std::vector<int64_t> ring(kRetimedRingSlots, -1);
        const uint32_t run = f0;
        uint32_t have = run, k = k0, done = 0;
        while (k < k1) {
            const uint32_t st = k * stride;
            while (have < st + span) {
                for (uint32_t t = 0; t < 16; t++)
                    if (have + t < f1) {
                        CHECK(have + t < F);
                        ring[retimed_slot(have + t, run)] = have + t;
                    }
                have += 16;
            }
            const uint32_t k_ready = std::min(k1, retimed_windows_ready(have, span, stride));
            CHECK(k_ready > k);
            for (uint32_t kk = k; kk < k_ready; kk++, done++)
                for (uint32_t i = 0; i < 16; i++) {
                    const uint32_t s0 = kk * stride - run;  // as the kernel forms the slot: (s0 + tap) & 63
                    CHECK(ring[(s0 + tap[i]) & (kRetimedRingSlots - 1)] == (int64_t)(kk * stride + tap[i]));
                }
            k = k_ready;
        }
        CHECK(done == k1 - k0);
    }
    CHECK(next == n);
    return 0;
}

int main()
{
    const uint32_t rates[][2] = {{1, 1}, {25, 24}, {6, 5}, {5, 4}, {3, 2}, {31, 16}, {2, 1}};
    for (const auto &r : rates)
        for (uint32_t F = 16; F <= 130; F++)
            for (uint32_t stride = 1; stride <= 40; stride++)
                if (one(F, stride, r[0], r[1])) return 1;
    // rates the calls refuse, and the edges of the range
    if (retimed_rate_ok(1, 0) || retimed_rate_ok(0, 1) || retimed_rate_ok(4, 5) || retimed_rate_ok(5, 2) || retimed_rate_ok(65536, 65536) ||
        retimed_rate_ok(65536, 40000) || !retimed_rate_ok(65535, 65535) || !retimed_rate_ok(65535, 32768) || !retimed_rate_ok(2, 1) ||
        retimed_window_count(100, 1, 5, 2) != 0 || retimed_window_count(100, 0, 6, 5) != 0 || retimed_window_count(30, 1, 2, 1) != 0 ||
        retimed_window_count(31, 1, 2, 1) != 1 || retimed_span(65535, 32768) != 30 || retimed_span(65535, 65535) != 16) {
        std::printf("FAILED the range of rates\n");
        return 1;
    }
    std::printf("windows retimed plan ok\n");
    return 0;
}
