// Stand-alone check of csrc/windows_mixed_rates_plan.h (no HIP, no GPU; built with -fsanitize=address,undefined by
// tests/test_hash_windows_mixed_rates_plan.py).  Libraries of 1 .. 6 videos, frame counts drawn from {31, 32, 33, 47, 48, 49, 63, 64, 65, 130}, widths on both
// sides of 192, with and without boxes, strides 1, 2, 7, 16, 17, 33, 40, rate lists: subsets of {1/1, 6/5, 5/4, 3/2, 31/16, 2/1} and one 8-rate list with a
// duplicate and an unreduced rate:
//   - first[r] is windows_first_retimed at rate r, rate_first its totals, row0 = rate_first[r] + first[r][i] (first and rate_first printed: the Python side
//     holds them against vdf_hash_windows_clips_first_rates and numpy);
//   - every segment index maps back to its video by windows_video_of, the lookup the kernel runs; seg_first is strictly ascending;
//   - every window of every rate is hashed exactly once, in the segment that owns its START, by the kernel's own cursor arithmetic;
//   - a replay of the kernel's walk (chunks of 16 frames into the ring of 64 slots) finds every tap of every window resident when pass t reads it, and no
//     rate is served while have < span_r;
//   - nothing is read at or past frame_end <= F_i, F_i is what the kernel derives from the record, and every frame resolves, by
//     windows_mixed_frame_offset, inside the planned small_bytes, to the pseudo-clip frame that holds that frame of that video;
//   - the resize stage is plan_windows_mixed's, descriptor for descriptor.
// Then the check codes in the order the header reports them and the uniform rule.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "windows_mixed_rates_plan.h"

using namespace vdf;

#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static const uint32_t kSizes[][2] = {{16, 16}, {33, 17}, {191, 40}, {192, 40}, {300, 130}};  // w x h: both sides of the 192-column split
static const uint32_t kRates[][2] = {{1, 1}, {6, 5}, {5, 4}, {3, 2}, {31, 16}, {2, 1}};
static const uint32_t kEight[][2] = {{2, 1}, {1, 1}, {6, 5}, {3, 2}, {5, 4}, {12, 10}, {31, 16}, {2, 1}};  // 12/10 = 6/5 unreduced, 2/1 twice

static int check_set(const std::vector<MixedClip> &clips, const std::vector<uint32_t> &nf, uint32_t stride, const std::vector<uint32_t> &num,
                     const std::vector<uint32_t> &den, bool print)
{
    const size_t n = clips.size();
    const uint32_t R = (uint32_t)num.size();
    CHECK(check_windows_mixed(clips.data(), nf.data(), n, stride, ~0ull).error == WindowsMixedError::kNone);
    CHECK(check_windows_mixed_rates(nf.data(), n, stride, R, num.data(), den.data()).error == WindowsMixedRatesError::kNone);
    const WindowsMixedRatesPlan p = plan_windows_mixed_rates(clips.data(), nf.data(), n, stride, R, num.data(), den.data());
    const WindowsMixedPlan m = plan_windows_mixed(clips.data(), nf.data(), n, stride);
    CHECK(p.kind == WindowsMixedRatesPlan::kMixed && m.kind == WindowsMixedPlan::kMixed);
    CHECK(p.first.size() == (size_t)R * (n + 1) && p.rate_first.size() == R + 1 && p.seg_first.size() == n + 1 && p.videos.size() == n &&
          p.row0.size() == (size_t)R * n && p.seg_first[0] == 0 && p.rate_first[0] == 0);
    CHECK(p.stride == stride && p.per_seg == std::max<uint32_t>(1, 32 / stride) && p.a.n_rates == R);
    std::vector<std::vector<uint32_t>> tap(R, std::vector<uint32_t>(16));
    std::vector<uint32_t> span(R);
    for (uint32_t r = 0; r < R; r++) {
        span[r] = retimed_span(num[r], den[r]);
        CHECK(p.a.span[r] == span[r]);
        for (uint32_t t = 0; t < 16; t++) {
            tap[r][t] = (uint32_t)(((uint64_t)t * num[r]) / den[r]);
            CHECK(((t < 8 ? p.a.taps_lo[r] : p.a.taps_hi[r]) >> (8 * (t & 7)) & 255u) == tap[r][t]);
        }
    }
    // first, rate_first, row0: every block is the one-rate library call's
    uint64_t total = 0;
    for (uint32_t r = 0; r < R; r++) {
        std::vector<uint32_t> first(n + 1);
        CHECK(windows_first_retimed(nf.data(), n, stride, num[r], den[r], first.data()));
        CHECK(p.rate_first[r] == total);
        for (size_t i = 0; i <= n; i++) CHECK(p.first[(size_t)r * (n + 1) + i] == first[i]);
        for (size_t i = 0; i < n; i++) {
            CHECK(p.row0[(size_t)r * n + i] == total + first[i]);
            CHECK(p.n_win(r, i) == retimed_window_count(nf[i], stride, num[r], den[r]) && p.n_win(r, i) >= 1);
        }
        total += first[n];
    }
    CHECK(p.rate_first[R] == total && total <= 0xFFFFFFFFull);
    if (print) {
        std::printf("first %u", stride);
        for (uint32_t r = 0; r < R; r++) std::printf(" %u/%u", num[r], den[r]);
        std::printf(" |");
        for (size_t i = 0; i < n; i++) std::printf(" %u", nf[i]);
        std::printf(" :");
        for (uint32_t x : p.first) std::printf(" %u", x);
        std::printf(" :");
        for (uint64_t x : p.rate_first) std::printf(" %llu", (unsigned long long)x);
        std::printf("\n");
    }
    for (size_t i = 0; i < n; i++) {
        uint32_t most = 0;
        for (uint32_t r = 0; r < R; r++) most = std::max(most, p.n_win(r, i));
        CHECK(p.seg_first[i + 1] - p.seg_first[i] == (most + p.per_seg - 1) / p.per_seg && p.seg_first[i + 1] > p.seg_first[i]);  // strictly ascending
        const WindowsVideoRecord &v = p.videos[i], &mv = m.videos[i];
        CHECK(v.n_win == most && v.first == p.row0[i] && v.seg_first == p.seg_first[i] && v.reserved[0] == 0 && v.reserved[1] == 0);
        CHECK(v.slot0 == mv.slot0 && v.main_frames == mv.main_frames && v.tail_first == mv.tail_first);
        CHECK(windows_mixed_rates_frames(v) == nf[i]);  // what the kernel computes every n_win_r from
    }
    // the resize stage is the plain mixed call's, descriptor for descriptor
    CHECK(p.small_bytes == m.small_bytes && p.small_bytes == p.descs.size() * 4096 && p.descs.size() == m.descs.size() && p.launches.size() == m.launches.size());
    CHECK(p.max_w == m.max_w && p.max_h == m.max_h);
    std::vector<long> src_video(p.small_bytes / 256, -1), src_frame(p.small_bytes / 256, -1);
    size_t covered = 0;
    for (size_t li = 0; li < p.launches.size(); li++) {
        const MixedLaunch &l = p.launches[li];
        CHECK(l.part == m.launches[li].part && l.first == m.launches[li].first && l.count == m.launches[li].count);
        CHECK(l.count >= 1 && l.count <= kMaxClipsPerLaunch && l.first == covered);
        covered += l.count;
        for (size_t s = l.first; s < l.first + l.count; s++) {
            const MixedClipDesc &d = p.descs[s], &e = m.descs[s];
            const size_t i = d.out_index;
            CHECK(d.offset == e.offset && d.out_index == e.out_index && d.bw == e.bw && d.bh == e.bh && d.x0 == e.x0 && d.y0 == e.y0 && d.pitch == e.pitch &&
                  d.frame_stride == e.frame_stride && d.h_table == e.h_table && d.v_table == e.v_table);
            CHECK(i < n && windows_mixed_part_of(clips[i].w) == l.part);
            const uint64_t f0 = (d.offset - clips[i].offset) / clips[i].frame_stride;
            CHECK(f0 + 16 <= nf[i]);
            for (uint32_t f = 0; f < 16; f++) {
                CHECK(src_video[s * 16 + f] == -1);
                src_video[s * 16 + f] = (long)i;
                src_frame[s * 16 + f] = (long)(f0 + f);
            }
        }
    }
    CHECK(covered == p.descs.size());
    // every segment of the call: the kernel's lookup, its windows, its frames, where it looks for them, and its ring
    const uint32_t n_groups = p.seg_first[n];
    std::vector<int> owner((size_t)total, -1);
    for (uint32_t g = 0; g < n_groups; g++) {
        const uint32_t i = windows_video_of(p.seg_first.data(), (uint32_t)n, g);
        CHECK(i < n && p.seg_first[i] <= g && g < p.seg_first[i + 1]);
        const WindowsVideoRecord &v = p.videos[i];
        const uint32_t F = windows_mixed_rates_frames(v), seg = g - v.seg_first, k_begin = seg * p.per_seg, run = k_begin * stride;
        // f_end as the kernel forms it, against the plan's own words
        uint32_t f_end = 0;
        bool some = false;
        for (uint32_t r = 0; r < R; r++) {
            const uint32_t n_win = (F - span[r]) / stride + 1;
            CHECK(n_win == p.n_win(r, i));
            const uint32_t k_end = (uint32_t)std::min<uint64_t>((uint64_t)k_begin + p.per_seg, n_win);
            CHECK(k_end == p.end_window(seg, r, i) && k_begin == p.first_window(seg) && (k_end > k_begin) == p.owns(seg, r, i));
            if (k_end > k_begin) { f_end = std::max(f_end, (k_end - 1) * stride + span[r]); some = true; }
        }
        CHECK(some && f_end == p.frame_end(seg, i) && run == p.frame_begin(seg) && f_end > run && f_end <= nf[i]);
        for (uint32_t f = run; f < f_end; f++) {  // (the kernel clamps the lanes past f_end to f_end - 1)
            const size_t at = windows_mixed_frame_offset(v, f);
            CHECK(at % 256 == 0 && at + 256 <= p.small_bytes);
            CHECK(src_video[at / 256] == (long)i && src_frame[at / 256] == (long)f);
        }
        // the kernel's walk: what each slot of the ring holds when pass t reads it
        std::vector<int64_t> ring(kRetimedRingSlots, -1);
        std::vector<uint32_t> done(R, 0);
        uint32_t have = run;
        while (have < f_end) {
            for (uint32_t t = 0; t < 16; t++)
                if (have + t < f_end) ring[retimed_slot(have + t, run)] = have + t;  // nothing at or past f_end is read or stored
            have += 16;
            for (uint32_t r = 0; r < R; r++) {
                const uint32_t n_win = (F - span[r]) / stride + 1;
                const uint32_t k_end = (uint32_t)std::min<uint64_t>((uint64_t)k_begin + p.per_seg, n_win);
                const uint32_t k_from = std::max(k_begin, rates_windows_ready(have - 16, span[r], stride));
                const uint32_t k_ready = std::min(k_end, rates_windows_ready(have, span[r], stride));
                if (have < span[r]) CHECK(k_ready == 0);  // no rate is served while have < span_r (have - span_r would wrap)
                for (uint32_t kk = k_from; kk < k_ready; kk++, done[r]++) {
                    CHECK(kk * stride + span[r] <= have && kk / p.per_seg == seg);  // whole, and in the segment that owns its start
                    const size_t row = (size_t)p.row0[(size_t)r * n + i] + kk;
                    CHECK(row < total && owner[row] == -1);
                    owner[row] = (int)g;
                    for (uint32_t t = 0; t < 16; t++) {
                        const uint32_t s0 = kk * stride - run;  // as the kernel forms the slot: (s0 + tap) & 63
                        CHECK(ring[(s0 + tap[r][t]) & (kRetimedRingSlots - 1)] == (int64_t)(kk * stride + tap[r][t]));
                    }
                }
            }
        }
        for (uint32_t r = 0; r < R; r++) CHECK(done[r] == (p.owns(seg, r, i) ? p.end_window(seg, r, i) - k_begin : 0));
    }
    for (int o : owner) CHECK(o >= 0);  // every window of every rate hashed, and (above) once
    return 0;
}

static int check_routes()
{
    std::vector<MixedClip> c(5);
    std::vector<uint32_t> nf(5, 40);
    for (size_t i = 0; i < 5; i++) c[i] = MixedClip{100 + i * 40 * 70, 70, 8, 8, {0, 0, 0, 0}};
    const uint32_t num[3] = {1, 6, 2}, den[3] = {1, 5, 1};
    WindowsMixedRatesPlan p = plan_windows_mixed_rates(c.data(), nf.data(), 5, 3, 3, num, den);
    CHECK(p.kind == WindowsMixedRatesPlan::kUniform && p.offset0 == 100 && p.clip_stride == 40 * 70 && p.descs.empty());
    const WindowsRatesPlan u = plan_windows_rates(5, 40, 3, 3, num, den);
    CHECK(p.uniform.ok && u.ok && p.uniform.n_out == u.n_out && p.uniform.n_seg == u.n_seg && p.rate_first[3] == u.n_out);
    for (uint32_t r = 0; r < 3; r++) {  // the rows coincide: first[r][c] = c n_win_r behind the same rate_first
        CHECK(p.rate_first[r] == u.a.out_first[r] && p.uniform.a.out_first[r] == u.a.out_first[r] && p.uniform.a.n_win[r] == u.a.n_win[r]);
        for (size_t i = 0; i < 5; i++) CHECK(p.row0[r * 5 + i] == u.a.out_first[r] + i * u.a.n_win[r]);
    }
    CHECK(plan_windows_mixed_rates(c.data(), nf.data(), 1, 3, 3, num, den).kind == WindowsMixedRatesPlan::kUniform);
    std::vector<uint32_t> g = nf;
    g[3] = 41;
    CHECK(plan_windows_mixed_rates(c.data(), g.data(), 5, 3, 3, num, den).kind == WindowsMixedRatesPlan::kMixed);  // one differing F
    std::vector<MixedClip> d = c;
    d[2].crop[3] = 1;
    CHECK(plan_windows_mixed_rates(d.data(), nf.data(), 5, 3, 3, num, den).kind == WindowsMixedRatesPlan::kMixed);  // one box
    d = c;
    d[4].offset += 1;
    CHECK(plan_windows_mixed_rates(d.data(), nf.data(), 5, 3, 3, num, den).kind == WindowsMixedRatesPlan::kMixed);  // one irregular offset
    // a one-rate list and plain-tap rates take the new kernel on a mixed library: there is no plain kind
    const uint32_t one[1] = {1}, one25[1] = {25}, one24[1] = {24};
    CHECK(plan_windows_mixed_rates(d.data(), nf.data(), 5, 3, 1, one, one).kind == WindowsMixedRatesPlan::kMixed);
    CHECK(plan_windows_mixed_rates(d.data(), g.data(), 5, 3, 1, one25, one24).kind == WindowsMixedRatesPlan::kMixed);
    CHECK(plan_windows_mixed_rates(c.data(), nf.data(), 5, 3, 1, one, one).kind == WindowsMixedRatesPlan::kUniform);
    // no videos: the tables have their shapes and nothing is planned
    p = plan_windows_mixed_rates(nullptr, nullptr, 0, 3, 3, num, den);
    CHECK(p.seg_first.size() == 1 && p.seg_first[0] == 0 && p.first.size() == 3 && p.rate_first.size() == 4 && p.rate_first[3] == 0 && p.row0.empty() && p.descs.empty());
    return 0;
}

// the planner checks in the order api.cpp runs them: 1 .. 8 = WindowsMixedError, then 8 + WindowsMixedRatesError (9 rate count, 10 bad rate, 11 too short,
// 12 too many rows)
static int code_of(const std::vector<MixedClip> &c, const std::vector<uint32_t> &f, uint32_t stride, uint64_t bytes, uint32_t R, const uint32_t *num,
                   const uint32_t *den, uint32_t *rate, size_t *video)
{
    const WindowsMixedCheck a = check_windows_mixed(c.data(), f.data(), c.size(), stride, bytes);
    *video = a.video;
    *rate = 99;
    if (a.error != WindowsMixedError::kNone) return (int)a.error;
    const WindowsMixedRatesCheck b = check_windows_mixed_rates(f.data(), c.size(), stride, R, num, den);
    *video = b.video;
    *rate = b.rate;
    return b.error == WindowsMixedRatesError::kNone ? 0 : 8 + (int)b.error;
}

static int check_errors()
{
    const MixedClip good{0, 64, 8, 8, {0, 0, 0, 0}};
    std::vector<MixedClip> c(3, good);
    for (size_t i = 0; i < 3; i++) c[i].offset = i * 40 * 64;
    std::vector<uint32_t> f{40, 20, 17};  // at 2/1 (span 31) videos 1 and 2 are too short, at 6/5 (span 19) video 2
    const uint64_t bytes = 3 * 40 * 64;
    size_t v = 99;
    uint32_t r = 99;
    const uint32_t n_ok[3] = {1, 6, 2}, d_ok[3] = {1, 5, 1};
    CHECK(code_of(c, f, 1, bytes, 3, n_ok, d_ok, &r, &v) == 11 && r == 1 && v == 2);  // in LIST order: 6/5 comes before 2/1, and names video 2
    const uint32_t n_sw[3] = {1, 2, 6}, d_sw[3] = {1, 1, 5};
    CHECK(code_of(c, f, 1, bytes, 3, n_sw, d_sw, &r, &v) == 11 && r == 1 && v == 1);  // 2/1 first: its first too-short video is 1
    CHECK(code_of(c, f, 1, bytes, 1, n_ok, d_ok, &r, &v) == 0);
    const uint32_t n25[2] = {25, 1}, d24[2] = {24, 1};
    CHECK(code_of(c, f, 1, bytes, 2, n25, d24, &r, &v) == 0);
    // n_rates and the rate arrays, in front of the rates themselves
    const uint32_t n_bad[3] = {1, 5, 2}, d_bad[3] = {1, 2, 1};
    CHECK(code_of(c, f, 1, bytes, 0, n_bad, d_bad, &r, &v) == 9 && code_of(c, f, 1, bytes, 9, n_bad, d_bad, &r, &v) == 9);
    CHECK(code_of(c, f, 1, bytes, 3, nullptr, d_bad, &r, &v) == 9 && code_of(c, f, 1, bytes, 3, n_bad, nullptr, &r, &v) == 9);
    // a bad rate in front of a too-short video (2/1 is listed behind it and video 1 is too short for it) ...
    CHECK(code_of(c, f, 1, bytes, 3, n_bad, d_bad, &r, &v) == 10 && r == 1);
    const uint32_t n_b2[4] = {2, 1, 4, 65536}, d_b2[4] = {1, 0, 5, 65536};
    CHECK(code_of(c, f, 1, bytes, 2, n_b2, d_b2, &r, &v) == 10 && r == 1);  // a bad rate BEHIND a rate a video is too short for: still the rate first
    CHECK(code_of(c, f, 1, bytes, 1, n_b2 + 2, d_b2 + 2, &r, &v) == 10 && r == 0 && code_of(c, f, 1, bytes, 1, n_b2 + 3, d_b2 + 3, &r, &v) == 10);
    // ... and behind every check of the plain mixed call: an out-of-buffer video, a zero stride, 2^32 windows
    CHECK(code_of(c, f, 1, bytes - 40 * 64, 3, n_bad, d_bad, &r, &v) == (int)WindowsMixedError::kOutOfBuffer && v == 2);
    CHECK(code_of(c, f, 0, bytes, 3, n_bad, d_bad, &r, &v) == (int)WindowsMixedError::kZeroWindowStride);
    std::vector<uint32_t> big{0xFFFFFF00u, 0x00000200u, 17};
    CHECK(code_of(c, big, 1, ~0ull, 3, n_bad, d_bad, &r, &v) == (int)WindowsMixedError::kTooManyWindows && v == 1);
    CHECK(code_of(c, big, 2, ~0ull, 3, n_bad, d_bad, &r, &v) == 10);
    CHECK(code_of(c, big, 2, ~0ull, 3, n_ok, d_ok, &r, &v) == 11 && r == 1 && v == 2);
    f[1] = 15;  // fewer than 16 frames comes first of all
    CHECK(code_of(c, f, 0, 10, 3, n_bad, d_bad, &r, &v) == (int)WindowsMixedError::kNotEnoughFrames && v == 1);
    // 2^32 rows in all: each block fits, their sum does not - behind the span check
    std::vector<MixedClip> one(1, good);
    std::vector<uint32_t> huge{0x80000020u};
    const uint32_t n3[3] = {1, 1, 1}, d3[3] = {1, 1, 1};
    CHECK(code_of(one, huge, 1, ~0ull, 1, n3, d3, &r, &v) == 0 && code_of(one, huge, 1, ~0ull, 2, n3, d3, &r, &v) == 12 && r == 1);
    std::vector<uint32_t> huge_short{0x80000020u, 20};
    std::vector<MixedClip> two(2, good);
    const uint32_t n4[3] = {1, 1, 2}, d4[3] = {1, 1, 1};
    CHECK(code_of(two, huge_short, 1, ~0ull, 3, n4, d4, &r, &v) == 11 && r == 2 && v == 1);
    // windows_first_rates: the blocks, rate_first nullable, and the 2^32 rule
    uint32_t first[12];
    uint64_t rf[4];
    const uint32_t nf3[3] = {40, 31, 65};
    const uint32_t n2[2] = {2, 1}, d2[2] = {1, 1};
    CHECK(windows_first_rates(nf3, 3, 2, 2, n2, d2, first, rf) && first[0] == 0 && first[1] == 5 && first[2] == 6 && first[3] == 24 && first[4] == 0 &&
          first[5] == 13 && first[6] == 21 && first[7] == 46 && rf[0] == 0 && rf[1] == 24 && rf[2] == 70);
    CHECK(windows_first_rates(nf3, 3, 2, 2, n2, d2, first, nullptr) && first[7] == 46);
    CHECK(!windows_first_rates(huge.data(), 1, 1, 2, n3, d3, first, rf) && windows_first_rates(huge.data(), 1, 1, 1, n3, d3, first, rf) && rf[1] == 0x80000011ull);
    CHECK(check_windows_mixed_rates(nullptr, 0, 1, 3, n_ok, d_ok).error == WindowsMixedRatesError::kNone);
    return 0;
}

int main()
{
    const uint32_t strides[] = {1, 2, 7, 16, 17, 33, 40};
    const uint32_t counts[] = {31, 32, 33, 47, 48, 49, 63, 64, 65, 130};
    std::mt19937 rng(20240421);
    size_t sets = 0, windows = 0;
    for (uint32_t mask = 1; mask <= 64; mask++) {  // 1 .. 63: the subsets of the six rates; 64: the 8-rate list
        std::vector<uint32_t> num, den;
        if (mask == 64)
            for (const auto &r : kEight) { num.push_back(r[0]); den.push_back(r[1]); }
        else
            for (int b = 0; b < 6; b++)
                if (mask >> b & 1) { num.push_back(kRates[b][0]); den.push_back(kRates[b][1]); }
        if (mask % 3 == 0 && num.size() > 1) { std::swap(num.front(), num.back()); std::swap(den.front(), den.back()); }  // the list's order is the caller's
        for (uint32_t stride : strides)
            for (int round = 0; round < 4; round++) {
                const size_t n = 1 + (mask + round * 2 + stride) % 6;
                const bool boxes = round >= 2;
                std::vector<MixedClip> clips(n);
                std::vector<uint32_t> nf(n);
                uint64_t at = 1 + rng() % 7;
                for (size_t i = 0; i < n; i++) {
                    const uint32_t *sz = kSizes[rng() % 5];
                    nf[i] = counts[rng() % 10];
                    MixedClip &c = clips[i];
                    c.w = sz[0]; c.h = sz[1];
                    c.frame_stride = (uint64_t)c.w * c.h + (rng() % 3 == 0 ? 3 : 0);
                    c.offset = at;
                    for (int e = 0; e < 4; e++) c.crop[e] = boxes && rng() % 2 == 0 ? 1 + rng() % 4 : 0;
                    at += (uint64_t)nf[i] * c.frame_stride + rng() % 9;
                }
                if (n == 1) clips[0].crop[0] = 1;  // (one plain video alone is the uniform kind)
                else nf[0] = nf[1] == 31 ? 32 : 31;  // (equal videos one step apart would be, too)
                if (check_set(clips, nf, stride, num, den, round == 3 && (mask % 8 == 0 || mask == 63))) return 1;
                sets++;
                for (size_t r = 0; r < num.size(); r++)
                    for (size_t i = 0; i < n; i++) windows += retimed_window_count(nf[i], stride, num[r], den[r]);
            }
    }
    if (check_routes() || check_errors()) return 1;
    std::printf("windows mixed rates plan ok: %zu sets, %zu windows\n", sets, windows);
    return 0;
}
