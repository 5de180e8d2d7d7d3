// Stand-alone check of csrc/windows_mixed_plan.h (no HIP, no GPU; built with -fsanitize=address,undefined by tests/test_hash_windows_mixed_plan.py).
// For random sets of 1 .. 40 videos of mixed sizes, F in 16 .. 100 and every stride 1 .. 40:
//   - first is the prefix sums of window_count (printed: the Python side holds them against vdf_hash_windows_clips_first);
//   - every segment index maps back to its video by windows_video_of, the lookup the kernel runs;
//   - every window of every video is owned by exactly one segment, every frame a segment reads is below F_i;
//   - every frame the windows kernel can address in `small` (windows_mixed_frame_offset) is written by exactly one pseudo-clip frame, that frame is
//     the video's frame f, and no pseudo-clip names a frame at or past F_i; launches hold one part and at most kMaxClipsPerLaunch pseudo-clips;
//   - the uniform rule: equal videos one step apart give the uniform kind; one differing F, one box, one irregular offset do not.
// Then the argument checks in the order the header reports them.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "windows_mixed_plan.h"

using namespace vdf;

#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static const uint32_t kSizes[][2] = {{16, 16}, {33, 17}, {64, 48}, {191, 40}, {192, 40}, {300, 130}};  // w x h

static int check_set(const std::vector<MixedClip> &clips, const std::vector<uint32_t> &nf, uint32_t stride, bool print)
{
    const size_t n = clips.size();
    const WindowsMixedPlan p = plan_windows_mixed(clips.data(), nf.data(), n, stride);
    CHECK(p.kind == WindowsMixedPlan::kMixed);
    CHECK(p.first.size() == n + 1 && p.seg_first.size() == n + 1 && p.videos.size() == n);
    CHECK(p.first[0] == 0 && p.seg_first[0] == 0);
    std::vector<uint32_t> first(n + 1);
    CHECK(windows_first(nf.data(), n, stride, first.data()));
    if (print) {
        std::printf("first %u", stride);
        for (size_t i = 0; i < n; i++) std::printf(" %u", nf[i]);
        std::printf(" :");
        for (size_t i = 0; i <= n; i++) std::printf(" %u", first[i]);
        std::printf("\n");
    }
    for (size_t i = 0; i < n; i++) {
        CHECK(first[i + 1] - first[i] == window_count(nf[i], stride) && p.first[i] == first[i]);
        const WindowsPlan w = plan_windows(nf[i], stride);
        CHECK(w.per_seg == p.per_seg && p.seg_first[i + 1] - p.seg_first[i] == w.n_seg && w.n_seg >= 1);
        const WindowsVideoRecord &v = p.videos[i];
        CHECK(v.n_win == w.n_win && v.first == first[i] && v.seg_first == p.seg_first[i] && v.main_frames == 16 * (nf[i] / 16) && v.tail_first == nf[i] - 16);
    }
    CHECK(p.first[n] == first[n]);
    // the resize stage: which source frame (video, frame) each 256-byte slot of `small` receives, written once
    CHECK(p.small_bytes == p.descs.size() * 4096);
    std::vector<long> src_video(p.small_bytes / 256, -1), src_frame(p.small_bytes / 256, -1);
    size_t covered = 0;
    for (const MixedLaunch &l : p.launches) {
        CHECK(l.count >= 1 && l.count <= kMaxClipsPerLaunch && l.first == covered);
        covered += l.count;
        for (size_t s = l.first; s < l.first + l.count; s++) {
            const MixedClipDesc &d = p.descs[s];
            const size_t i = d.out_index;
            CHECK(i < n && windows_mixed_part_of(clips[i].w) == l.part && d.pitch == clips[i].w && d.frame_stride == clips[i].frame_stride);
            CHECK(d.x0 == clips[i].crop[0] && d.y0 == clips[i].crop[2] && d.bw == clips[i].w - clips[i].crop[0] - clips[i].crop[1] &&
                  d.bh == clips[i].h - clips[i].crop[2] - clips[i].crop[3] && d.bw <= p.max_w && d.bh <= p.max_h);
            CHECK(d.offset >= clips[i].offset && (d.offset - clips[i].offset) % clips[i].frame_stride == 0);
            const uint64_t f0 = (d.offset - clips[i].offset) / clips[i].frame_stride;
            CHECK(f0 + 16 <= nf[i]);  // no pseudo-clip names a frame at or past F_i
            for (uint32_t f = 0; f < 16; f++) {
                CHECK(src_video[s * 16 + f] == -1);
                src_video[s * 16 + f] = (long)i;
                src_frame[s * 16 + f] = (long)(f0 + f);
            }
        }
    }
    CHECK(covered == p.descs.size());
    for (long v : src_video) CHECK(v >= 0);
    // every segment of the call: the kernel's lookup, its windows, its frames and where it looks for them
    const uint32_t n_groups = p.seg_first[n];
    std::vector<int> owner(first[n], -1);
    for (uint32_t g = 0; g < n_groups; g++) {
        const uint32_t i = windows_video_of(p.seg_first.data(), (uint32_t)n, g);
        CHECK(i < n && p.seg_first[i] <= g && g < p.seg_first[i + 1]);
        const WindowsVideoRecord &v = p.videos[i];
        const uint32_t seg = g - v.seg_first, k_begin = seg * p.per_seg;
        const uint32_t k_end = (uint32_t)std::min<uint64_t>((uint64_t)k_begin + p.per_seg, v.n_win);
        CHECK(k_begin < k_end);
        const uint32_t f_end = (k_end - 1) * stride + 16;
        CHECK(f_end <= nf[i]);
        for (uint32_t k = k_begin; k < k_end; k++) {
            CHECK(owner[v.first + k] == -1);
            owner[v.first + k] = (int)g;
        }
        for (uint32_t f = k_begin * stride; f < f_end; f++) {  // (the kernel clamps the lanes past f_end to f_end - 1)
            const size_t at = windows_mixed_frame_offset(v, f);
            CHECK(at % 256 == 0 && at / 256 < src_video.size());
            CHECK(src_video[at / 256] == (long)i && src_frame[at / 256] == (long)f);
        }
    }
    for (int o : owner) CHECK(o >= 0);
    // ... and every frame of every video is addressable, whether this stride's windows use it or not
    for (size_t i = 0; i < n; i++)
        for (uint32_t f = 0; f < nf[i]; f++) {
            const size_t at = windows_mixed_frame_offset(p.videos[i], f);
            CHECK(at / 256 < src_video.size() && src_video[at / 256] == (long)i && src_frame[at / 256] == (long)f);
        }
    return 0;
}

static int check_uniform_rule()
{
    std::vector<MixedClip> c(5);
    std::vector<uint32_t> nf(5, 40);
    for (size_t i = 0; i < 5; i++) c[i] = MixedClip{100 + i * 40 * 70, 70, 8, 8, {0, 0, 0, 0}};
    WindowsMixedPlan p = plan_windows_mixed(c.data(), nf.data(), 5, 3);
    CHECK(p.kind == WindowsMixedPlan::kUniform && p.offset0 == 100 && p.clip_stride == 40 * 70 && p.descs.empty());
    CHECK(p.first[5] == 5 * window_count(40, 3) && p.seg_first[5] == 5 * plan_windows(40, 3).n_seg);
    p = plan_windows_mixed(c.data(), nf.data(), 1, 3);
    CHECK(p.kind == WindowsMixedPlan::kUniform && p.clip_stride == 40 * 70);
    for (size_t i = 1; i < 5; i++) c[i].offset += 5 * i;  // padded between the videos: still one step
    CHECK(plan_windows_mixed(c.data(), nf.data(), 5, 3).kind == WindowsMixedPlan::kUniform);
    {
        std::vector<uint32_t> g = nf;
        g[3] = 41;
        CHECK(plan_windows_mixed(c.data(), g.data(), 5, 3).kind == WindowsMixedPlan::kMixed);  // one differing F
    }
    {
        std::vector<MixedClip> d = c;
        d[2].crop[3] = 1;
        CHECK(plan_windows_mixed(d.data(), nf.data(), 5, 3).kind == WindowsMixedPlan::kMixed);  // one box
        d = c;
        d[4].offset += 1;
        CHECK(plan_windows_mixed(d.data(), nf.data(), 5, 3).kind == WindowsMixedPlan::kMixed);  // one irregular offset
        d = c;
        std::swap(d[0], d[1]);
        CHECK(plan_windows_mixed(d.data(), nf.data(), 5, 3).kind == WindowsMixedPlan::kMixed);  // descending
        d = c;
        d[1].frame_stride = 71;
        CHECK(plan_windows_mixed(d.data(), nf.data(), 5, 3).kind == WindowsMixedPlan::kMixed);
        d = c;
        d[1].w = 4; d[1].h = 16;
        CHECK(plan_windows_mixed(d.data(), nf.data(), 5, 3).kind == WindowsMixedPlan::kMixed);
    }
    return 0;
}

static int check_errors()
{
    using E = WindowsMixedError;
    const MixedClip good{0, 64, 8, 8, {0, 0, 0, 0}};
    std::vector<MixedClip> c(3, good);
    for (size_t i = 0; i < 3; i++) c[i].offset = i * 20 * 64;
    const std::vector<uint32_t> nf(3, 20);
    const uint64_t bytes = 3 * 20 * 64;
    auto chk = [&](const std::vector<MixedClip> &cc, const std::vector<uint32_t> &ff, uint32_t stride, uint64_t b) { return check_windows_mixed(cc.data(), ff.data(), cc.size(), stride, b); };
    CHECK(chk(c, nf, 1, bytes).error == E::kNone && chk({}, {}, 0, 0).error == E::kZeroWindowStride && chk({}, {}, 1, 0).error == E::kNone);
    // every later error is present as well: the earlier one is reported, with its first video
    std::vector<MixedClip> bad = c;
    std::vector<uint32_t> f = nf;
    f[2] = 0xFFFFFFF0u;  // 7: within 64 of 2^32 (and 5: out of the buffer)
    WindowsMixedCheck r = chk(bad, f, 0, bytes);
    CHECK(r.error == E::kOutOfBuffer && r.video == 2);
    CHECK(chk(bad, f, 0, ~0ull).error == E::kZeroWindowStride);
    r = chk(bad, f, 1, ~0ull);
    CHECK(r.error == E::kFrameCount && r.video == 2);
    f[2] = 0xFFFFFF00u; f[1] = 0x00000200u;  // 8: 2^32 windows or more at stride 1, reached at video 2
    r = chk(bad, f, 1, ~0ull);
    CHECK(r.error == E::kTooManyWindows && r.video == 2);
    CHECK(chk(bad, f, 2, ~0ull).error == E::kNone);
    f = nf;
    bad[1].crop[0] = 4; bad[1].crop[1] = 4;  // 4
    r = chk(bad, f, 0, 10);
    CHECK(r.error == E::kEmptyBox && r.video == 1);
    bad[2].frame_stride = 63;  // 3
    r = chk(bad, f, 0, 10);
    CHECK(r.error == E::kStrideBelowFrame && r.video == 2);
    bad[0].h = 0;  // 2
    r = chk(bad, f, 0, 10);
    CHECK(r.error == E::kZeroDim && r.video == 0);
    f[1] = 15;  // 1
    r = chk(bad, f, 0, 10);
    CHECK(r.error == E::kNotEnoughFrames && r.video == 1);
    // 5 covers the LAST frame, not frame 15, in 128 bits
    CHECK(chk(c, nf, 1, bytes - 1).error == E::kOutOfBuffer && chk(c, nf, 1, bytes - 1).video == 2);
    bad = c;
    bad[1].offset = ~0ull - 10; bad[1].frame_stride = ~0ull;
    r = chk(bad, nf, 1, ~0ull);
    CHECK(r.error == E::kOutOfBuffer && r.video == 1);
    uint32_t first[4];
    CHECK(windows_first(nf.data(), 3, 2, first) && first[0] == 0 && first[1] == 3 && first[3] == 9);
    const uint32_t big[2] = {0x80000010u, 0x80000010u};
    CHECK(!windows_first(big, 2, 1, first) && windows_first(big, 1, 1, first) && first[1] == 0x80000001u);
    return 0;
}

int main()
{
    std::mt19937 rng(20240615);
    size_t sets = 0, windows = 0;
    for (uint32_t stride = 1; stride <= 40; stride++)
        for (int round = 0; round < 12; round++) {
            const size_t n = 1 + rng() % 40;
            std::vector<MixedClip> clips(n);
            std::vector<uint32_t> nf(n);
            uint64_t at = 1 + rng() % 7;
            for (size_t i = 0; i < n; i++) {
                const uint32_t *sz = kSizes[rng() % 6];
                nf[i] = 16 + rng() % 85;
                MixedClip &c = clips[i];
                c.w = sz[0]; c.h = sz[1];
                c.frame_stride = (uint64_t)c.w * c.h + (rng() % 3 == 0 ? 3 : 0);
                c.offset = at;
                for (int e = 0; e < 4; e++) c.crop[e] = rng() % 4 == 0 ? rng() % 5 : 0;
                at += (uint64_t)nf[i] * c.frame_stride + rng() % 9;
            }
            if (n == 1) clips[0].crop[0] = 1;  // (one plain video alone is the uniform kind)
            if (check_set(clips, nf, stride, round == 0)) return 1;
            sets++;
            for (size_t i = 0; i < n; i++) windows += window_count(nf[i], stride);
        }
    if (check_uniform_rule() || check_errors()) return 1;
    std::printf("windows mixed plan ok: %zu sets, %zu windows\n", sets, windows);
    return 0;
}
