// The planner of vdf_hash_clips_u8[_device] (csrc/resize_dispatch.cpp: check_mixed, plan_mixed) on the CPU, the pattern of resize_dispatch_main.cpp:
// compiled with g++ from resize_dispatch.cpp and resize_tables.cpp alone (no HIP, no GPU) by tests/test_hash_mixed_plan.py.
//   parts      every clip of every pair of sizes and of random batches of 1 .. 300 clips lands in exactly one part whose kernel accepts it
//   uniform    one size at a constant positive step (with and without boxes) is the uniform call; equal or descending offsets are not
//   cuts       no launch has more than kMaxClipsPerLaunch clips, the launches tile the descriptors
//   envelope   for every descriptor: the frames whose loads could pass the buffer's end are exactly those the kernels' own expression sends to
//              the careful loader, and no fast-path load reaches past the end - clips ending on the last byte, 1, 63, 64, 127 ... before it, odd offsets
//   errors     every rejection of check_mixed, with the clip it names
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "../../vid_dup_finder_lib_amd/csrc/resize_dispatch.h"

using namespace vdf;

static int g_bad = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            if (g_bad < 20) { std::printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
            g_bad++;                                              \
        }                                                         \
    } while (0)

static const uint32_t kSizes[][2] = {{1, 1}, {7, 5}, {16, 16}, {17, 33}, {64, 64}, {65, 64}, {96, 96}, {160, 90}, {256, 128}, {256, 129}, {257, 128},
                                     {191, 130}, {192, 130}, {320, 240}, {641, 361}, {1280, 720}, {1920, 1080}};
constexpr size_t kNSizes = sizeof kSizes / sizeof kSizes[0];

static MixedPart documented_part(uint32_t w, uint32_t h)
{
    if (w <= 256 && (h + 63) / 64 <= 2) return MixedPart::kSmall;
    return w < 192 ? MixedPart::kLines : MixedPart::kWideLines;
}

// clips laid out one after the other with the given gaps; returns the buffer size that ends `tail` bytes behind the last clip
static uint64_t lay_out(std::vector<MixedClip> &clips, std::mt19937 &rng, bool odd, uint64_t tail)
{
    uint64_t at = odd ? 1 : 0;
    for (MixedClip &c : clips) {
        c.offset = at;
        if (c.frame_stride == 0) c.frame_stride = (uint64_t)c.w * c.h;
        at += 15 * c.frame_stride + (uint64_t)c.w * c.h + (odd ? 2 * (rng() % 40) + 1 : 64 * (rng() % 3));
        if (odd) at |= 1;
    }
    const MixedClip &l = clips.back();
    return l.offset + 15 * l.frame_stride + (uint64_t)l.w * l.h + tail;
}

static MixedPart part_of_desc(const MixedPlan &p, size_t i)
{
    for (const MixedLaunch &l : p.launches)
        if (i >= l.first && i < l.first + l.count) return l.part;
    CHECK(false, "descriptor %zu in no launch", i);
    return MixedPart::kSmall;
}

// what the plan must be for these clips, whatever they are
static void check_plan(const std::vector<MixedClip> &clips, const MixedPlan &p, uint64_t buf_bytes)
{
    const size_t n = clips.size();
    CHECK(p.kind == MixedPlan::kMixed, "not mixed");
    CHECK(p.descs.size() == n, "%zu descriptors for %zu clips", p.descs.size(), n);
    std::vector<int> seen(n, 0);
    size_t covered = 0;
    for (const MixedLaunch &l : p.launches) {
        CHECK(l.first == covered && l.count >= 1 && l.count <= kMaxClipsPerLaunch, "launch [%zu, +%zu) after %zu", l.first, l.count, covered);
        CHECK((l.part == MixedPart::kSmall) == (l.first < p.n_small) && (l.part == MixedPart::kSmall ? l.first + l.count <= p.n_small : true), "small part is not first");
        covered += l.count;
    }
    CHECK(covered == n, "launches cover %zu of %zu", covered, n);
    for (size_t i = 0; i < p.descs.size(); i++) {
        const MixedClipDesc &d = p.descs[i];
        CHECK(d.out_index < n, "out_index %u of %zu", d.out_index, n);
        if (d.out_index >= n) continue;
        seen[d.out_index]++;
        const MixedClip &c = clips[d.out_index];
        const MixedPart part = part_of_desc(p, i);
        CHECK(part == documented_part(c.w, c.h), "clip %u (%u x %u) in part %d", d.out_index, c.w, c.h, (int)part);
        // the kernel of the part accepts it: the fused small kernel holds a frame of at most 4 x 2 tiles; the whole-line form wants 1.5 windows
        if (part == MixedPart::kSmall) CHECK(c.w <= 256 && c.h <= 128, "small part got %u x %u", c.w, c.h);
        if (part == MixedPart::kWideLines) CHECK(c.w >= 192, "whole-line part got %u wide", c.w);
        if (part == MixedPart::kLines) CHECK(c.w < 192 && c.h > 128, "line part got %u x %u", c.w, c.h);
        CHECK(d.offset == c.offset && d.frame_stride == c.frame_stride && d.pitch == c.w && d.x0 == c.crop[0] && d.y0 == c.crop[2] &&
              d.bw == c.w - c.crop[0] - c.crop[1] && d.bh == c.h - c.crop[2] - c.crop[3], "descriptor of clip %u", d.out_index);
        CHECK(d.bw >= 1 && d.bh >= 1 && d.bw <= p.max_w && d.bh <= p.max_h && d.h_table == d.bw && d.v_table == d.bh, "box / table sizes of clip %u", d.out_index);
        // ---- the address envelope, frame by frame
        const uint64_t overrun = mixed_loader_overrun(part);
        const bool uncropped = (c.crop[0] | c.crop[1] | c.crop[2] | c.crop[3]) == 0;
        for (uint32_t f = 0; f < 16; f++) {
            const bool careful = mixed_frame_is_careful(d, part, f, buf_bytes);
            const uint64_t src = d.offset + (uint64_t)f * d.frame_stride + (uint64_t)d.y0 * d.pitch + d.x0;
            const uint64_t box_end = src + (uint64_t)(d.bh - 1) * d.pitch + d.bw;  // one past the last pixel of the box in this frame
            const uint64_t envelope = box_end + overrun;                             // ... plus the loader's documented overrun
            // every loader reads 16 bytes at columns 0, 16, 32 ... < bw of rows < bh: the last byte a fast-path load touches
            const uint64_t touched = src + (uint64_t)(d.bh - 1) * d.pitch + 16 * (uint64_t)((d.bw - 1) / 16) + 16;
            CHECK(touched <= envelope, "clip %u frame %u: loads reach %llu, envelope %llu", d.out_index, f, (unsigned long long)touched, (unsigned long long)envelope);
            if (envelope > buf_bytes) CHECK(careful, "clip %u frame %u: envelope %llu passes the end %llu on the fast path", d.out_index, f, (unsigned long long)envelope, (unsigned long long)buf_bytes);
            if (!careful) CHECK(touched <= buf_bytes && envelope <= buf_bytes, "clip %u frame %u: fast path reads past the end", d.out_index, f);
            if (uncropped) CHECK(careful == (envelope > buf_bytes), "clip %u frame %u: careful %d, envelope %llu, end %llu", d.out_index, f, (int)careful, (unsigned long long)envelope, (unsigned long long)buf_bytes);
        }
        // the small kernel's all-loads-first path is taken when frame 15 is not careful: then no frame is
        if (!mixed_frame_is_careful(d, part, 15, buf_bytes))
            for (uint32_t f = 0; f < 15; f++) CHECK(!mixed_frame_is_careful(d, part, f, buf_bytes), "clip %u: frame %u careful but not frame 15", d.out_index, f);
    }
    for (size_t i = 0; i < n; i++) CHECK(seen[i] == 1, "clip %zu in %d descriptors", i, seen[i]);
}

static MixedClip clip_of(uint32_t w, uint32_t h) { return MixedClip{0, 0, w, h, {0, 0, 0, 0}}; }

int main()
{
    const HashKnobs knobs;
    std::mt19937 rng(7);
    const uint64_t tails[] = {0, 1, 63, 64, 127, 128, 129, 4096};
    size_t n_plans = 0, n_careful_clips = 0;
    // ---- every pair of sizes, both orders, every tail, even and odd offsets
    for (size_t a = 0; a < kNSizes; a++)
        for (size_t b = 0; b < kNSizes; b++) {
            if (a == b) continue;
            for (uint64_t tail : tails)
                for (int odd = 0; odd < 2; odd++) {
                    std::vector<MixedClip> clips = {clip_of(kSizes[a][0], kSizes[a][1]), clip_of(kSizes[b][0], kSizes[b][1])};
                    if ((a + b) % 3 == 0) clips[1].frame_stride = (uint64_t)clips[1].w * clips[1].h + 37;
                    const uint64_t buf_bytes = lay_out(clips, rng, odd != 0, tail);
                    const MixedCheck chk = check_mixed(clips.data(), clips.size(), 16, buf_bytes);
                    CHECK(chk.error == MixedError::kNone, "valid pair rejected: %d clip %zu", (int)chk.error, chk.clip);
                    const MixedPlan p = plan_mixed(clips.data(), clips.size(), knobs);
                    check_plan(clips, p, buf_bytes);
                    n_plans++;
                    // the last clip's frame 15 is careful exactly when fewer than `overrun` bytes follow it
                    const MixedPart part = documented_part(clips[1].w, clips[1].h);
                    for (const MixedClipDesc &d : p.descs)
                        if (d.out_index == 1) {
                            const bool careful = mixed_frame_is_careful(d, part, 15, buf_bytes);
                            CHECK(careful == (tail < mixed_loader_overrun(part)), "tail %llu, part %d: careful %d", (unsigned long long)tail, (int)part, (int)careful);
                            n_careful_clips += careful;
                        }
                }
        }
    // ---- random batches of 1 .. 300 clips with boxes and padded frames
    for (int round = 0; round < 200; round++) {
        static const size_t kFirst[4] = {1, 2, 299, 300};
        const size_t n = round < 4 ? kFirst[round] : 1 + rng() % 300;
        std::vector<MixedClip> clips;
        for (size_t i = 0; i < n; i++) {
            const uint32_t *s = kSizes[rng() % kNSizes];
            MixedClip c = clip_of(s[0], s[1]);
            if (rng() % 3 == 0) c.frame_stride = (uint64_t)c.w * c.h + rng() % 100;
            if (rng() % 4 == 0 && c.w > 4 && c.h > 4) { c.crop[0] = rng() % (c.w / 3); c.crop[1] = rng() % (c.w / 3); c.crop[2] = rng() % (c.h / 3); c.crop[3] = rng() % (c.h / 3); }
            clips.push_back(c);
        }
        const uint64_t buf_bytes = lay_out(clips, rng, round % 2 != 0, tails[round % 8]);
        const MixedCheck chk = check_mixed(clips.data(), n, 16, buf_bytes);
        CHECK(chk.error == MixedError::kNone, "valid batch rejected: %d clip %zu", (int)chk.error, chk.clip);
        MixedPlan p = plan_mixed(clips.data(), n, knobs);
        if (p.kind == MixedPlan::kUniform) continue;  // (one clip, or by chance one size evenly spaced)
        check_plan(clips, p, buf_bytes);
        n_plans++;
    }
    // ---- uniform batches
    for (int cropped = 0; cropped < 2; cropped++)
        for (uint64_t pad : {0ull, 64ull, 37ull}) {
            std::vector<MixedClip> clips;
            const uint32_t w = 160, h = 90;
            const uint64_t fs = (uint64_t)w * h + 16, step = 16 * fs + pad;
            for (size_t i = 0; i < 33; i++) {
                MixedClip c = clip_of(w, h);
                c.frame_stride = fs;
                c.offset = 5 + i * step;
                if (cropped && i % 2) { c.crop[2] = 10; c.crop[3] = 12; }
                clips.push_back(c);
            }
            MixedPlan p = plan_mixed(clips.data(), clips.size(), knobs);
            CHECK(p.kind == MixedPlan::kUniform && p.offset0 == 5 && p.clip_stride == step && p.cropped == (cropped != 0), "uniform batch, pad %llu", (unsigned long long)pad);
            CHECK(p.descs.empty() && p.launches.empty(), "uniform plan carries descriptors");
            // one clip out of step / of another size / of another frame stride: mixed
            std::vector<MixedClip> v = clips;
            v[20].offset += 1;
            CHECK(plan_mixed(v.data(), v.size(), knobs).kind == MixedPlan::kMixed, "uneven step taken for uniform");
            v = clips; v[7].w = 161;
            CHECK(plan_mixed(v.data(), v.size(), knobs).kind == MixedPlan::kMixed, "two sizes taken for uniform");
            v = clips; v[32].frame_stride += 1;
            CHECK(plan_mixed(v.data(), v.size(), knobs).kind == MixedPlan::kMixed, "two frame strides taken for uniform");
            // equal offsets (one clip hashed n times) and descending offsets: no positive clip_stride
            v = clips;
            for (MixedClip &c : v) c.offset = 5;
            MixedPlan q = plan_mixed(v.data(), v.size(), knobs);
            CHECK(q.kind == MixedPlan::kMixed && q.descs.size() == v.size(), "equal offsets taken for uniform");
            v = clips;
            std::reverse(v.begin(), v.end());
            q = plan_mixed(v.data(), v.size(), knobs);
            CHECK(q.kind == MixedPlan::kMixed, "descending offsets taken for uniform");
            check_plan(v, q, clips.back().offset + 16 * fs);
        }
    {
        std::vector<MixedClip> one = {clip_of(641, 361)};
        one[0].frame_stride = 641 * 361;
        one[0].offset = 3;
        const MixedPlan p = plan_mixed(one.data(), 1, knobs);
        CHECK(p.kind == MixedPlan::kUniform && p.offset0 == 3 && p.clip_stride >= 16, "a single clip is the uniform call");
        CHECK(plan_mixed(one.data(), 0, knobs).launches.empty(), "no clips, no launches");
    }
    // ---- launch cuts: more clips of one part than a launch takes (sizes alternate so that the batch is not uniform)
    {
        const size_t n = 2 * kMaxClipsPerLaunch + 5;
        std::vector<MixedClip> clips(n);
        uint64_t at = 0;
        for (size_t i = 0; i < n; i++) {
            clips[i] = clip_of(i % 2 ? 8 : 9, 4);
            clips[i].frame_stride = (uint64_t)clips[i].w * 4;
            clips[i].offset = at;
            at += 16 * clips[i].frame_stride;
        }
        clips[n - 1] = clip_of(320, 240);
        clips[n - 1].frame_stride = 320 * 240;
        clips[n - 1].offset = at;
        at += 16 * 320 * 240;
        const MixedPlan p = plan_mixed(clips.data(), n, knobs);
        CHECK(p.launches.size() == 4 && p.launches[0].count == kMaxClipsPerLaunch && p.launches[1].count == kMaxClipsPerLaunch && p.launches[2].count == 4 &&
              p.launches[3].part == MixedPart::kWideLines && p.launches[3].count == 1 && p.n_small == n - 1, "cuts: %zu launches", p.launches.size());
        for (const MixedLaunch &l : p.launches) CHECK((uint64_t)l.count * 16 * 256 < (1ull << 32), "grid of %zu clips", l.count);
        check_plan(clips, p, at);
    }
    // ---- knobs that switch the small kernel off send its clips to the per-frame parts
    {
        HashKnobs k;
        k.no_smallcrop = true;
        CHECK(mixed_part_of(64, 64, k) == MixedPart::kLines && mixed_part_of(256, 128, k) == MixedPart::kWideLines && mixed_part_of(64, 64, knobs) == MixedPart::kSmall, "knobs");
    }
    // ---- every rejection, with the clip it names
    {
        std::vector<MixedClip> ok = {clip_of(64, 64), clip_of(320, 240), clip_of(17, 33)};
        const uint64_t buf_bytes = lay_out(ok, rng, true, 0);
        const auto expect = [&](std::vector<MixedClip> v, uint32_t fpc, uint64_t bytes, MixedError e, size_t clip, const char *what) {
            const MixedCheck c = check_mixed(v.data(), v.size(), fpc, bytes);
            CHECK(c.error == e && c.clip == clip, "%s: error %d at clip %zu", what, (int)c.error, c.clip);
        };
        expect(ok, 16, buf_bytes, MixedError::kNone, 0, "valid call");
        expect(ok, 17, buf_bytes, MixedError::kNone, 0, "more frames than needed");
        expect(ok, 15, buf_bytes, MixedError::kNotEnoughFrames, 0, "15 frames");
        expect(ok, 0, buf_bytes, MixedError::kNotEnoughFrames, 0, "no frames");
        std::vector<MixedClip> v = ok; v[1].w = 0;
        expect(v, 16, buf_bytes, MixedError::kZeroDim, 1, "zero width");
        v = ok; v[2].h = 0; v[0].frame_stride = 1;  // (the order of the codes: dimensions before strides)
        expect(v, 16, buf_bytes, MixedError::kZeroDim, 2, "zero height");
        v = ok; v[1].frame_stride = 320 * 240 - 1;
        expect(v, 16, buf_bytes, MixedError::kStrideBelowFrame, 1, "short stride");
        v = ok; v[0].crop[0] = 32; v[0].crop[1] = 32;
        expect(v, 16, buf_bytes, MixedError::kEmptyBox, 0, "box without columns");
        v = ok; v[2].crop[2] = 0xFFFFFFFFu; v[2].crop[3] = 2;
        expect(v, 16, buf_bytes, MixedError::kEmptyBox, 2, "box whose bars wrap 32 bits");
        expect(ok, 16, buf_bytes - 1, MixedError::kOutOfBuffer, 2, "one byte short");
        v = ok; v[1].offset = ~0ull - 5;
        expect(v, 16, buf_bytes, MixedError::kOutOfBuffer, 1, "offset that wraps 64 bits");
        v = ok; v[0].frame_stride = ~0ull / 2;
        expect(v, 16, buf_bytes, MixedError::kOutOfBuffer, 0, "stride that wraps 64 bits");
    }
    std::printf("%zu plans checked, %zu last clips on the careful loader\n", n_plans, n_careful_clips);
    std::puts(g_bad ? "mixed plan FAILED" : "mixed plan ok");
    return g_bad ? 1 : 0;
}
