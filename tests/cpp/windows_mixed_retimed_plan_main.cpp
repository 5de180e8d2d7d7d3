// Stand-alone check of csrc/windows_mixed_retimed_plan.h (no HIP, no GPU; built with -fsanitize=address,undefined by
// tests/test_hash_windows_mixed_retimed_plan.py).  Libraries of 1 .. 6 videos, frame counts drawn from {span, span + 1, 31, 32, 33, 47, 48, 63, 64, 65,
// 130} (those below span left out), widths on both sides of 192, with and without boxes, strides 1, 2, 7, 16, 17, 33, 40, rates 6/5, 5/4, 3/2, 31/16, 2/1:
//   - first is the prefix sums of retimed_window_count (printed: the Python side holds them against vdf_hash_windows_clips_first_retimed);
//   - every segment index maps back to its video by windows_video_of, the lookup the kernel runs; every window is in exactly one segment;
//   - every frame a segment walks is below F_i and resolves, by windows_mixed_frame_offset, inside the planned small_bytes, to the pseudo-clip frame
//     that holds that frame of that video;
//   - a replay of the kernel's walk (chunks of 16 frames into the ring of 64 slots) finds every tap of every window resident when pass t reads it;
//   - the resize stage is plan_windows_mixed's, pseudo-clip for pseudo-clip.
// Then the check codes in the order the header reports them, the uniform rule and the plain-tap rates.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "windows_mixed_retimed_plan.h"

using namespace vdf;

#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static const uint32_t kSizes[][2] = {{16, 16}, {33, 17}, {191, 40}, {192, 40}, {300, 130}};  // w x h: both sides of the 192-column split

static int check_set(const std::vector<MixedClip> &clips, const std::vector<uint32_t> &nf, uint32_t stride, uint32_t num, uint32_t den, bool print)
{
    const size_t n = clips.size();
    CHECK(check_windows_mixed(clips.data(), nf.data(), n, stride, ~0ull).error == WindowsMixedError::kNone);
    CHECK(check_windows_mixed_retimed(nf.data(), n, num, den).error == WindowsMixedRetimedError::kNone);
    const WindowsMixedRetimedPlan p = plan_windows_mixed_retimed(clips.data(), nf.data(), n, stride, num, den);
    const WindowsMixedPlan m = plan_windows_mixed(clips.data(), nf.data(), n, stride);
    CHECK(p.kind == WindowsMixedRetimedPlan::kMixed && m.kind == WindowsMixedPlan::kMixed);
    CHECK(p.first.size() == n + 1 && p.seg_first.size() == n + 1 && p.videos.size() == n && p.first[0] == 0 && p.seg_first[0] == 0);
    const uint32_t span = retimed_span(num, den);
    CHECK(p.rate.span == span && p.rate.stride == stride && p.per_seg == std::max<uint32_t>(1, 32 / stride) && p.rate.per_seg == p.per_seg);
    uint32_t tap[16];
    for (uint32_t t = 0; t < 16; t++) {
        tap[t] = (uint32_t)(((uint64_t)t * num) / den);
        CHECK(((t < 8 ? p.rate.taps_lo : p.rate.taps_hi) >> (8 * (t & 7)) & 255u) == tap[t]);
    }
    std::vector<uint32_t> first(n + 1);
    CHECK(windows_first_retimed(nf.data(), n, stride, num, den, first.data()));
    if (print) {
        std::printf("first %u %u %u", stride, num, den);
        for (size_t i = 0; i < n; i++) std::printf(" %u", nf[i]);
        std::printf(" :");
        for (size_t i = 0; i <= n; i++) std::printf(" %u", first[i]);
        std::printf("\n");
    }
    for (size_t i = 0; i < n; i++) {
        const WindowsRetimedPlan w = plan_windows_retimed(nf[i], stride, num, den);
        CHECK(w.n_win >= 1 && first[i + 1] - first[i] == w.n_win && p.first[i] == first[i]);
        CHECK(w.per_seg == p.per_seg && p.seg_first[i + 1] - p.seg_first[i] == w.n_seg && w.n_seg >= 1);  // strictly ascending
        const WindowsVideoRecord &v = p.videos[i], &mv = m.videos[i];
        CHECK(v.n_win == w.n_win && v.first == first[i] && v.seg_first == p.seg_first[i] && v.reserved[0] == 0 && v.reserved[1] == 0);
        CHECK(v.slot0 == mv.slot0 && v.main_frames == mv.main_frames && v.tail_first == mv.tail_first);
    }
    CHECK(p.first[n] == first[n]);
    // the resize stage is the plain mixed call's
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
            const MixedClipDesc &d = p.descs[s];
            const size_t i = d.out_index;
            CHECK(d.offset == m.descs[s].offset && d.out_index == m.descs[s].out_index && d.bw == m.descs[s].bw && d.bh == m.descs[s].bh);
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
    std::vector<int> owner(first[n], -1);
    for (uint32_t g = 0; g < n_groups; g++) {
        const uint32_t i = windows_video_of(p.seg_first.data(), (uint32_t)n, g);
        CHECK(i < n && p.seg_first[i] <= g && g < p.seg_first[i + 1]);
        const WindowsVideoRecord &v = p.videos[i];
        const uint32_t seg = g - v.seg_first, k_begin = seg * p.per_seg;
        const uint32_t k_end = (uint32_t)std::min<uint64_t>((uint64_t)k_begin + p.per_seg, v.n_win);
        CHECK(k_begin < k_end);
        const uint32_t f_end = (k_end - 1) * stride + span;
        CHECK(f_end <= nf[i]);
        for (uint32_t k = k_begin; k < k_end; k++) {
            CHECK(owner[v.first + k] == -1);
            owner[v.first + k] = (int)g;
        }
        const uint32_t run = k_begin * stride;
        for (uint32_t f = run; f < f_end; f++) {  // (the kernel clamps the lanes past f_end to f_end - 1)
            const size_t at = windows_mixed_frame_offset(v, f);
            CHECK(at % 256 == 0 && at + 256 <= p.small_bytes);
            CHECK(src_video[at / 256] == (long)i && src_frame[at / 256] == (long)f);
        }
        // the kernel's walk: what each slot of the ring holds when pass t reads it
        std::vector<int64_t> ring(kRetimedRingSlots, -1);
        uint32_t have = run, k = k_begin, done = 0;
        while (k < k_end) {
            const uint32_t st = k * stride;
            while (have < st + span) {
                for (uint32_t t = 0; t < 16; t++)
                    if (have + t < f_end) ring[retimed_slot(have + t, run)] = have + t;
                have += 16;
            }
            const uint32_t k_ready = std::min(k_end, retimed_windows_ready(have, span, stride));
            CHECK(k_ready > k);
            for (uint32_t kk = k; kk < k_ready; kk++, done++)
                for (uint32_t t = 0; t < 16; t++) {
                    const uint32_t s0 = kk * stride - run;  // as the kernel forms the slot: (s0 + tap) & 63
                    CHECK(ring[(s0 + tap[t]) & (kRetimedRingSlots - 1)] == (int64_t)(kk * stride + tap[t]));
                }
            k = k_ready;
        }
        CHECK(done == k_end - k_begin);
    }
    for (int o : owner) CHECK(o >= 0);
    return 0;
}

static int check_routes()
{
    std::vector<MixedClip> c(5);
    std::vector<uint32_t> nf(5, 40);
    for (size_t i = 0; i < 5; i++) c[i] = MixedClip{100 + i * 40 * 70, 70, 8, 8, {0, 0, 0, 0}};
    WindowsMixedRetimedPlan p = plan_windows_mixed_retimed(c.data(), nf.data(), 5, 3, 6, 5);
    CHECK(p.kind == WindowsMixedRetimedPlan::kUniform && p.offset0 == 100 && p.clip_stride == 40 * 70 && p.descs.empty());
    CHECK(p.rate.F == 40 && p.rate.span == 19 && p.rate.n_win == retimed_window_count(40, 3, 6, 5));
    CHECK(p.first[5] == 5 * retimed_window_count(40, 3, 6, 5) && p.seg_first[5] == 5 * plan_windows_retimed(40, 3, 6, 5).n_seg);
    CHECK(plan_windows_mixed_retimed(c.data(), nf.data(), 1, 3, 2, 1).kind == WindowsMixedRetimedPlan::kUniform);
    {
        std::vector<uint32_t> g = nf;
        g[3] = 41;
        CHECK(plan_windows_mixed_retimed(c.data(), g.data(), 5, 3, 6, 5).kind == WindowsMixedRetimedPlan::kMixed);  // one differing F
        std::vector<MixedClip> d = c;
        d[2].crop[3] = 1;
        CHECK(plan_windows_mixed_retimed(d.data(), nf.data(), 5, 3, 6, 5).kind == WindowsMixedRetimedPlan::kMixed);  // one box
        d = c;
        d[4].offset += 1;
        CHECK(plan_windows_mixed_retimed(d.data(), nf.data(), 5, 3, 6, 5).kind == WindowsMixedRetimedPlan::kMixed);  // one irregular offset
        // the taps are 0 ... 15: the plain mixed call, whatever the library looks like
        for (const auto &lib : {c, d}) {
            CHECK(plan_windows_mixed_retimed(lib.data(), nf.data(), 5, 3, 1, 1).kind == WindowsMixedRetimedPlan::kPlain);
            CHECK(plan_windows_mixed_retimed(lib.data(), g.data(), 5, 3, 25, 24).kind == WindowsMixedRetimedPlan::kPlain);
        }
        CHECK(plan_windows_mixed_retimed(d.data(), g.data(), 5, 3, 16, 15).kind == WindowsMixedRetimedPlan::kMixed);  // tap(15) = 16: not plain
    }
    return 0;
}

// the two planner checks in the order api.cpp runs them: 1 .. 8 = WindowsMixedError, 9 = a bad rate, 10 = a video shorter than the span
static int code_of(const std::vector<MixedClip> &c, const std::vector<uint32_t> &f, uint32_t stride, uint64_t bytes, uint32_t num, uint32_t den, size_t *video)
{
    const WindowsMixedCheck a = check_windows_mixed(c.data(), f.data(), c.size(), stride, bytes);
    *video = a.video;
    if (a.error != WindowsMixedError::kNone) return (int)a.error;
    const WindowsMixedRetimedCheck b = check_windows_mixed_retimed(f.data(), c.size(), num, den);
    *video = b.video;
    return b.error == WindowsMixedRetimedError::kNone ? 0 : 8 + (int)b.error;
}

static int check_errors()
{
    const MixedClip good{0, 64, 8, 8, {0, 0, 0, 0}};
    std::vector<MixedClip> c(3, good);
    for (size_t i = 0; i < 3; i++) c[i].offset = i * 40 * 64;
    std::vector<uint32_t> f{40, 20, 17};  // at 2/1 (span 31) videos 1 and 2 are too short, at 6/5 (span 19) video 2
    const uint64_t bytes = 3 * 40 * 64;
    size_t v = 99;
    CHECK(code_of(c, f, 1, bytes, 2, 1, &v) == 10 && v == 1);
    CHECK(code_of(c, f, 1, bytes, 6, 5, &v) == 10 && v == 2);
    CHECK(code_of(c, f, 1, bytes, 1, 1, &v) == 0 && code_of(c, f, 1, bytes, 25, 24, &v) == 0);
    // a bad rate in front of a too-short video ...
    CHECK(code_of(c, f, 1, bytes, 5, 2, &v) == 9 && code_of(c, f, 1, bytes, 1, 0, &v) == 9 && code_of(c, f, 1, bytes, 4, 5, &v) == 9 &&
          code_of(c, f, 1, bytes, 65536, 65536, &v) == 9);
    // ... and behind every check of the plain mixed call: an out-of-buffer video, a zero stride, 2^32 windows
    CHECK(code_of(c, f, 1, bytes - 40 * 64, 5, 2, &v) == (int)WindowsMixedError::kOutOfBuffer && v == 2);
    CHECK(code_of(c, f, 0, bytes, 5, 2, &v) == (int)WindowsMixedError::kZeroWindowStride);
    std::vector<uint32_t> big{0xFFFFFF00u, 0x00000200u, 17};
    CHECK(code_of(c, big, 1, ~0ull, 5, 2, &v) == (int)WindowsMixedError::kTooManyWindows && v == 1);
    CHECK(code_of(c, big, 2, ~0ull, 5, 2, &v) == 9);
    CHECK(code_of(c, big, 2, ~0ull, 2, 1, &v) == 10 && v == 2);
    f[1] = 15;  // fewer than 16 frames comes first of all
    CHECK(code_of(c, f, 0, 10, 5, 2, &v) == (int)WindowsMixedError::kNotEnoughFrames && v == 1);
    // first[]: the retimed counts, and the 2^32 rule
    uint32_t first[4];
    const uint32_t nf3[3] = {40, 31, 65};
    CHECK(windows_first_retimed(nf3, 3, 2, 2, 1, first) && first[0] == 0 && first[1] == 5 && first[2] == 6 && first[3] == 24);
    const uint32_t huge[2] = {0x8000001Eu, 0x8000001Eu};  // 2^31 windows each at 2/1
    CHECK(!windows_first_retimed(huge, 2, 1, 2, 1, first) && windows_first_retimed(huge, 1, 1, 2, 1, first) && first[1] == 0x80000000u);
    CHECK(check_windows_mixed_retimed(nullptr, 0, 6, 5).error == WindowsMixedRetimedError::kNone);
    return 0;
}

int main()
{
    const uint32_t rates[][2] = {{6, 5}, {5, 4}, {3, 2}, {31, 16}, {2, 1}};
    const uint32_t strides[] = {1, 2, 7, 16, 17, 33, 40};
    std::mt19937 rng(20240418);
    size_t sets = 0, windows = 0;
    for (const auto &r : rates) {
        const uint32_t span = retimed_span(r[0], r[1]);
        const uint32_t counts[] = {span, span + 1, 31, 32, 33, 47, 48, 63, 64, 65, 130};
        for (uint32_t stride : strides)
            for (int round = 0; round < 12; round++) {
                const size_t n = 1 + round % 6;
                const bool boxes = round >= 6;
                std::vector<MixedClip> clips(n);
                std::vector<uint32_t> nf(n);
                uint64_t at = 1 + rng() % 7;
                for (size_t i = 0; i < n; i++) {
                    const uint32_t *sz = kSizes[rng() % 5];
                    do nf[i] = counts[rng() % 11];
                    while (nf[i] < span);
                    MixedClip &c = clips[i];
                    c.w = sz[0]; c.h = sz[1];
                    c.frame_stride = (uint64_t)c.w * c.h + (rng() % 3 == 0 ? 3 : 0);
                    c.offset = at;
                    for (int e = 0; e < 4; e++) c.crop[e] = boxes && rng() % 2 == 0 ? 1 + rng() % 4 : 0;
                    at += (uint64_t)nf[i] * c.frame_stride + rng() % 9;
                }
                if (n == 1) clips[0].crop[0] = 1;  // (one plain video alone is the uniform kind)
                else nf[0] = nf[1] == span ? span + 1 : span;  // (equal videos one step apart would be, too)
                if (check_set(clips, nf, stride, r[0], r[1], round == 5)) return 1;
                sets++;
                for (size_t i = 0; i < n; i++) windows += retimed_window_count(nf[i], stride, r[0], r[1]);
            }
    }
    if (check_routes() || check_errors()) return 1;
    std::printf("windows mixed retimed plan ok: %zu sets, %zu windows\n", sets, windows);
    return 0;
}
