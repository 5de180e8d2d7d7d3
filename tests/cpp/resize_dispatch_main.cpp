// Host-only check of csrc/resize_dispatch.cpp: for every width the geometry the launchers will use must fit the kernels'
// LDS buffers, keep the operand reads aligned and conflict-free where the rules say so, and the documented sizes must land
// on the documented kernels.  Then the planner (plan_hash / plan_cropped / plan_letterbox): every planned route's preconditions - the
// conditions under which its launcher refuses - hold for every width, knob setting, base and stride; the route table of DESIGN.md 4.1, the
// size list of tests/test_gpu_diff_sweep.py and bench.py's named kernels land where they say; cropped plans put every clip in exactly one
// part whose kernel accepts its box.  Built with g++ (no HIP).
#include <cstdio>
#include <cstdint>
#include <set>

#include "../../vid_dup_finder_lib_amd/csrc/resize_dispatch.h"

using namespace vdf;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); fails++; } } while (0)

static const uint8_t *const kAligned = reinterpret_cast<const uint8_t *>(uintptr_t(0x10000));

struct KnobCase { const char *name; HashKnobs k; };
static std::vector<KnobCase> knob_cases()  // every setting tests/test_gpu_diff_sweep.py and tests/test_gpu_knobs.py use that bears on hashing
{
    std::vector<KnobCase> v;
    const auto add = [&](const char *name, void (*set)(HashKnobs &)) { KnobCase c{name, HashKnobs()}; set(c.k); v.push_back(c); };
    add("default", [](HashKnobs &) {});
    add("mode1", [](HashKnobs &k) { k.resize_mode = 1; });
    add("mode3", [](HashKnobs &k) { k.resize_mode = 3; });
    add("mode4", [](HashKnobs &k) { k.resize_mode = 4; });
    add("mode5", [](HashKnobs &k) { k.resize_mode = 5; });
    add("mode6", [](HashKnobs &k) { k.resize_mode = 6; });
    add("no_wavestream", [](HashKnobs &k) { k.wavestream_knob = -1; });
    add("nw4", [](HashKnobs &k) { k.wavestream_knob = 4; });
    add("nw6", [](HashKnobs &k) { k.wavestream_knob = 6; });
    add("no_persistent", [](HashKnobs &k) { k.hash_no_persistent = true; });
    add("no_rowcrop", [](HashKnobs &k) { k.no_rowcrop = true; });
    add("rowcrop_all", [](HashKnobs &k) { k.rowcrop_all = true; });
    add("no_boxstream", [](HashKnobs &k) { k.no_boxstream = true; });
    add("no_smallcrop", [](HashKnobs &k) { k.no_smallcrop = true; });
    add("no_lb_fused", [](HashKnobs &k) { k.no_lb_fused = true; });
    add("lb_host_plan", [](HashKnobs &k) { k.lb_host_plan = true; });
    add("mode4_no_rowcrop_no_smallcrop", [](HashKnobs &k) { k.resize_mode = 4; k.no_rowcrop = k.no_smallcrop = true; });  // the sweeps' reference
    return v;
}

static HashCall packed_call(uint32_t w, uint32_t h, size_t n_clips = 1000, const uint8_t *base = kAligned)
{
    return HashCall{base, w, h, (size_t)w * h, (size_t)w * h * 16, n_clips};
}

// the preconditions of a planned stream / K-split route: what launch_resize_mfma_frames_stream / _ksplit refuse (also the ROWCROP launch of a cropped plan)
static void check_stream_route(const HashPlan &p, const HashCall &c, const HashKnobs &k, const char *what)
{
    uint32_t nb = 0, wp = 0;
    if (p.route == HashRoute::kWaveStream) {
        CHECK(p.waves != 0 && p.waves == resize_wavestream_waves(c.w, k.wavestream_knob) && p.layout_h == kMfmaLayoutHorizontalBand,
              "%s %s %ux%u: per-wave route needs a wave count and the band table (waves %d)", what, "wavestream", c.w, c.h, p.waves);
        CHECK(resize_stream_eligible(c.base, c.w, c.h, c.frame_stride, c.clip_stride, k.wavestream_knob), "%s %ux%u: per-wave route on an ineligible call", what, c.w, c.h);
    } else if (p.route == HashRoute::kChunkStream) {
        CHECK(stream_class(c.w, &nb) == 1 && nb == p.nb && p.layout_h == kMfmaLayoutHorizontal && resize_wavestream_waves(c.w, k.wavestream_knob) == 0,
              "%s %ux%u: chunk route needs the S class and the plain table", what, c.w, c.h);
        CHECK(resize_stream_eligible(c.base, c.w, c.h, c.frame_stride, c.clip_stride, k.wavestream_knob), "%s %ux%u: chunk route on an ineligible call", what, c.w, c.h);
    } else if (p.route == HashRoute::kKsplit) {
        CHECK(resize_ksplit_eligible(c.base, c.w, c.h, c.frame_stride, c.clip_stride) && p.nb >= 1 && p.nb == ksplit_geometry(c.w, &wp) && p.layout_h == kMfmaLayoutHorizontal,
              "%s %ux%u: K-split route on an ineligible call", what, c.w, c.h);
    }
}

static void check_plain_plans()
{
    const std::vector<KnobCase> knobs = knob_cases();
    for (uint32_t w = 1; w <= 4200; w++)
        for (uint32_t h : {16u, 48u, 64u, 128u, 129u, 256u, 270u, 1080u, 1088u})
            for (int geom = 0; geom < 4; geom++) {  // aligned / misaligned base x packed / padded strides
                const size_t fs = (size_t)w * h + (geom & 2 ? 16 + (16 - (size_t)w * h % 16) % 16 : 0);
                for (size_t n_clips : {size_t(1), size_t(1000)}) {
                    const HashCall c{kAligned + (geom & 1 ? 4 : 0), w, h, fs, 16 * fs + (geom & 2 ? 32 : 0), n_clips};
                    for (const KnobCase &kc : knobs)
                        for (TableFit fit : {TableFit::kAll, TableFit::kNoBand, TableFit::kNoPlain}) {
                            const HashKnobs &k = kc.k;
                            const HashPlan p = plan_hash(c, k, fit);
                            const bool direct = w == 16 && h == 16 && !(geom & 1);
                            CHECK((p.route == HashRoute::kDirect16) == direct, "%s %ux%u geom %d: direct route", kc.name, w, h, geom);
                            if (direct) continue;
                            CHECK(p.n_kt == (int)((w + 63) / 64) && p.n_rg == (int)((h + 63) / 64), "%s %ux%u: tile counts", kc.name, w, h);
                            if (k.resize_mode == 1) { CHECK(p.route == HashRoute::kScalar, "%s %ux%u: mode 1 is the scalar kernel", kc.name, w, h); continue; }
                            if (fit == TableFit::kNoPlain) {  // a forced mode that cannot serve a size refuses; mode 0 has the scalar kernel
                                CHECK(p.route == (k.resize_mode == 0 ? HashRoute::kScalar : HashRoute::kRefused), "%s %ux%u: tables that do not fit", kc.name, w, h);
                                continue;
                            }
                            CHECK(p.route != HashRoute::kScalar && p.route != HashRoute::kRefused, "%s %ux%u: fitting tables take a matrix-core kernel", kc.name, w, h);
                            check_stream_route(p, c, k, kc.name);
                            if (fit == TableFit::kNoBand) CHECK(p.route != HashRoute::kWaveStream && p.layout_h != kMfmaLayoutHorizontalBand, "%s %ux%u: no band table, no band route", kc.name, w, h);
                            CHECK((p.layout_v == kMfmaLayoutVerticalWide) == (p.route == HashRoute::kWholeLine), "%s %ux%u: vertical layout", kc.name, w, h);
                            if (p.route != HashRoute::kWaveStream) CHECK(p.layout_h == kMfmaLayoutHorizontal, "%s %ux%u: plain horizontal table", kc.name, w, h);
                            const bool persistent = p.route == HashRoute::kPersistentOneTile || p.route == HashRoute::kTiled;
                            if (persistent) {
                                CHECK(p.n_kt <= 4 && p.n_rg <= 4 && !k.hash_no_persistent, "%s %ux%u: persistent kernels take at most 4 x 4 tiles", kc.name, w, h);
                                CHECK(p.last_clip_apart == (w % 16 != 0), "%s %ux%u: unchecked 16-byte loads need W %% 16 == 0 or the last clip apart", kc.name, w, h);
                                if (p.last_clip_apart) CHECK(c.n_clips >= 2 && c.clip_stride >= 16, "%s %ux%u: a last clip to take apart", kc.name, w, h);
                            } else {
                                CHECK(!p.last_clip_apart, "%s %ux%u: last clip apart without a persistent kernel", kc.name, w, h);
                            }
                            if (p.route == HashRoute::kPersistentOneTile) CHECK(p.n_kt == 1 && p.n_rg == 1 && p.full_tile == (w == 64 && h == 64), "%s %ux%u: one tile", kc.name, w, h);
                            if (p.route == HashRoute::kTiled)
                                CHECK((p.tiled_nrg == 4 ? p.n_rg > 2 : p.n_rg == p.tiled_nrg) && p.waves != 0 && p.waves == tiled_waves(p.n_kt, p.tiled_nrg) && !(p.n_kt == 1 && p.n_rg == 1),
                                      "%s %ux%u: tiled <%d, %d, %d>", kc.name, w, h, p.n_kt, p.tiled_nrg, p.waves);
                            const bool fused = persistent || p.route == HashRoute::kPerClipFused;
                            if (k.resize_mode == 3) CHECK(fused, "%s %ux%u: mode 3 is the fused family", kc.name, w, h);
                            if (k.resize_mode == 4) CHECK(p.route == HashRoute::kWholeLine, "%s %ux%u: mode 4 is the whole-line kernel", kc.name, w, h);
                            if (k.resize_mode == 5) CHECK(p.route == HashRoute::kChunkStream || p.route == HashRoute::kWaveStream || p.route == HashRoute::kWholeLine, "%s %ux%u: mode 5", kc.name, w, h);
                            if (k.resize_mode == 6) CHECK(p.route == HashRoute::kKsplit || p.route == HashRoute::kWholeLine, "%s %ux%u: mode 6", kc.name, w, h);
                            if (geom & 1) CHECK(fused || p.route == HashRoute::kWholeLine, "%s %ux%u: a misaligned base streams nowhere", kc.name, w, h);
                            if (k.resize_mode == 0 && h > 256) CHECK(!fused, "%s %ux%u: tall frames do not fuse", kc.name, w, h);
                        }
                }
            }
    // the measured WAVES table is the one the tiled launcher instantiates
    static_assert(tiled_waves(4, 4) == 2 && tiled_waves(3, 4) == 3 && tiled_waves(2, 4) == 2 && tiled_waves(1, 4) == 3 && tiled_waves(4, 2) == 2 && tiled_waves(4, 1) == 2 &&
                  tiled_waves(3, 2) == 3 && tiled_waves(3, 1) == 3 && tiled_waves(2, 2) == 3 && tiled_waves(2, 1) == 1 && tiled_waves(1, 2) == 1 && tiled_waves(1, 1) == 0, "WAVES by (NKT, NRG)");
}

struct Want { uint32_t w, h; HashRoute route; int a, b; bool last_apart; };  // a, b: tiled <NKT = a, NRG = b>; wave count a; else unused
static void check_want(const char *what, const Want &q, const HashCall &c, const HashKnobs &k = HashKnobs(), TableFit fit = TableFit::kAll)
{
    const HashPlan p = plan_hash(c, k, fit);
    bool ok = p.route == q.route && p.last_clip_apart == q.last_apart;
    if (q.route == HashRoute::kTiled) ok = ok && p.n_kt == q.a && p.tiled_nrg == q.b;
    if (q.route == HashRoute::kWaveStream) ok = ok && p.waves == q.a;
    CHECK(ok, "%s %ux%u: route %d (n_kt %d, nrg %d, waves %d, last apart %d), expected route %d (%d, %d, last apart %d)", what, q.w, q.h, (int)p.route, p.n_kt, p.tiled_nrg,
          p.waves, (int)p.last_clip_apart, (int)q.route, q.a, q.b, (int)q.last_apart);
}

static void check_documented_routes()
{
    using R = HashRoute;
    // DESIGN.md 4.1, row by row (packed frames on an aligned base, many clips)
    const Want design[] = {{16, 16, R::kDirect16, 0, 0, false},
                           {64, 64, R::kPersistentOneTile, 0, 0, false}, {48, 36, R::kPersistentOneTile, 0, 0, false}, {47, 33, R::kPersistentOneTile, 0, 0, true},
                           {128, 128, R::kTiled, 2, 2, false}, {256, 64, R::kTiled, 4, 1, false}, {160, 120, R::kTiled, 3, 2, false}, {64, 256, R::kTiled, 1, 4, false},
                           {176, 144, R::kTiled, 3, 4, false}, {100, 200, R::kTiled, 2, 4, true},
                           {320, 64, R::kPerClipFused, 0, 0, false}, {1920, 48, R::kPerClipFused, 0, 0, false},
                           {320, 96, R::kChunkStream, 0, 0, false}, {256, 128, R::kChunkStream, 0, 0, false}, {1920, 128, R::kWaveStream, 4, 0, false}, {854, 128, R::kWaveStream, 8, 0, false},
                           {480, 270, R::kChunkStream, 0, 0, false}, {64, 1080, R::kChunkStream, 0, 0, false}, {448, 1080, R::kChunkStream, 0, 0, false},
                           {528, 1080, R::kWaveStream, 8, 0, false}, {640, 360, R::kWaveStream, 8, 0, false}, {1152, 648, R::kWaveStream, 6, 0, false}, {1280, 720, R::kWaveStream, 6, 0, false},
                           {1920, 1080, R::kWaveStream, 4, 0, false}, {1950, 1096, R::kWaveStream, 3, 0, false},
                           {1936, 1080, R::kKsplit, 0, 0, false}, {2560, 1440, R::kKsplit, 0, 0, false}, {3840, 2160, R::kKsplit, 0, 0, false}, {4096, 2160, R::kKsplit, 0, 0, false},
                           {4112, 2160, R::kWholeLine, 0, 0, false}, {48, 1080, R::kWholeLine, 0, 0, false}, {2353, 1088, R::kWholeLine, 0, 0, false}};
    for (const Want &q : design) check_want("DESIGN 4.1", q, packed_call(q.w, q.h));
    for (const Want &q : design) {  // ... and its last two rows: odd bases and strides take the whole-line kernel where the size does not fuse, unfitting tables the scalar one
        if (q.h > 256) check_want("misaligned base", Want{q.w, q.h, R::kWholeLine, 0, 0, false}, packed_call(q.w, q.h, 1000, kAligned + 1));
        if (q.h > 256) check_want("odd stride", Want{q.w, q.h, R::kWholeLine, 0, 0, false}, HashCall{kAligned, q.w, q.h, (size_t)q.w * q.h + 8, ((size_t)q.w * q.h + 8) * 16, 1000});
        if (q.route != R::kDirect16) check_want("tables that do not fit", Want{q.w, q.h, R::kScalar, 0, 0, false}, packed_call(q.w, q.h), HashKnobs(), TableFit::kNoPlain);
    }
    check_want("band table that does not fit", Want{1280, 720, R::kWholeLine, 0, 0, false}, packed_call(1280, 720), HashKnobs(), TableFit::kNoBand);
    check_want("band table that does not fit", Want{1950, 1096, R::kWholeLine, 0, 0, false}, packed_call(1950, 1096), HashKnobs(), TableFit::kNoBand);
    // tests/test_gpu_diff_sweep.py: HASH_SIZES, by the resize family its comment gives them
    const Want sweep[] = {{64, 64, R::kPersistentOneTile, 0, 0, false}, {64, 48, R::kPersistentOneTile, 0, 0, false}, {48, 36, R::kPersistentOneTile, 0, 0, false},
                          {32, 32, R::kPersistentOneTile, 0, 0, false}, {47, 33, R::kPersistentOneTile, 0, 0, true},  // (width off a multiple of 16: the last clip through the per-clip kernel)
                          {80, 48, R::kTiled, 2, 1, false}, {96, 64, R::kTiled, 2, 1, false}, {128, 72, R::kTiled, 2, 2, false}, {128, 128, R::kTiled, 2, 2, false},
                          {100, 60, R::kTiled, 2, 1, true}, {160, 90, R::kTiled, 3, 2, false}, {176, 144, R::kTiled, 3, 4, false},
                          {256, 128, R::kChunkStream, 0, 0, false}, {224, 126, R::kChunkStream, 0, 0, false},  // short and wide
                          {256, 144, R::kChunkStream, 0, 0, false}, {320, 180, R::kChunkStream, 0, 0, false}, {426, 240, R::kChunkStream, 0, 0, false}, {480, 270, R::kChunkStream, 0, 0, false},
                          {100, 300, R::kChunkStream, 0, 0, false},
                          {640, 360, R::kWaveStream, 8, 0, false}, {854, 480, R::kWaveStream, 8, 0, false}, {1024, 576, R::kWaveStream, 6, 0, false}, {1280, 720, R::kWaveStream, 6, 0, false},
                          {1366, 768, R::kWaveStream, 5, 0, false}, {1920, 1080, R::kWaveStream, 4, 0, false}, {1920, 64, R::kWaveStream, 4, 0, false}, {720, 576, R::kWaveStream, 8, 0, false},
                          {1440, 1080, R::kWaveStream, 5, 0, false},
                          {2560, 1440, R::kKsplit, 0, 0, false}, {3840, 2160, R::kKsplit, 0, 0, false}};
    CHECK(sizeof sweep / sizeof sweep[0] == 30, "every entry of HASH_SIZES");
    HashKnobs mode4;
    mode4.resize_mode = 4;
    for (const Want &q : sweep) {
        check_want("HASH_SIZES", q, packed_call(q.w, q.h));
        check_want("HASH_SIZES, the sweep's reference", Want{q.w, q.h, R::kWholeLine, 0, 0, false}, packed_call(q.w, q.h), mode4);
    }
    // bench.py names these kernels for its legs; the headline is the persistent <FULL> form
    check_want("bench full_hd", Want{1920, 1080, R::kWaveStream, 4, 0, false}, packed_call(1920, 1080, 1000));
    check_want("bench pitch_480x270", Want{480, 270, R::kChunkStream, 0, 0, false}, packed_call(480, 270, 4000));
    check_want("bench uhd_3840x2160", Want{3840, 2160, R::kKsplit, 0, 0, false}, packed_call(3840, 2160, 250));
    CHECK(plan_hash(packed_call(64, 64, 20000), HashKnobs()).full_tile, "64 x 64 takes the persistent <FULL> instantiation");
    // clips that repeat (clip_stride 0) or a single clip of an odd width: every clip through the careful loader
    CHECK(plan_hash(HashCall{kAligned, 47, 33, 47 * 33, 0, 100}, HashKnobs()).route == R::kPerClipFused, "clip_stride 0 at an odd width");
    CHECK(plan_hash(packed_call(47, 33, 1), HashKnobs()).route == R::kPerClipFused, "one clip of an odd width");
    // the letterbox entry
    HashKnobs k;
    LetterboxPlan lb = plan_letterbox(packed_call(64, 64, 1000), k);
    CHECK(lb.small_frames && lb.one_tile && lb.n_tail == 1, "letterbox 64 x 64: fused kernel, the last clip apart");
    lb = plan_letterbox(HashCall{kAligned, 8, 4, 32, 32, 1000}, k);
    CHECK(lb.one_tile && lb.n_tail == 2, "letterbox: every clip within 64 bytes of the end goes apart");
    lb = plan_letterbox(HashCall{kAligned, 64, 64, 4096, 0, 1000}, k);
    CHECK(lb.one_tile && lb.n_tail == 1000, "letterbox: clip_stride 0, all clips apart");
    lb = plan_letterbox(packed_call(128, 96, 1000), k);
    CHECK(lb.small_frames && !lb.one_tile && lb.n_tail == 1000, "letterbox 128 x 96: device boxes, no fused kernel");
    lb = plan_letterbox(packed_call(256, 128, 1000), k);
    CHECK(lb.small_frames && !lb.one_tile, "letterbox 256 x 128: device boxes");
    CHECK(!plan_letterbox(packed_call(1920, 1080, 1000), k).small_frames && !plan_letterbox(packed_call(256, 129, 1000), k).small_frames, "letterbox: larger frames plan on the host");
    k.no_lb_fused = true;
    lb = plan_letterbox(packed_call(64, 64, 1000), k);
    CHECK(lb.small_frames && !lb.one_tile && lb.n_tail == 1000, "VDF_NO_LB_FUSED");
    k = HashKnobs();
    k.lb_host_plan = true;
    CHECK(!plan_letterbox(packed_call(64, 64, 1000), k).small_frames, "VDF_LB_HOST_PLAN");
}

// every clip in exactly one part, and each part's kernel accepts its boxes
static void check_crop_plan(const char *what, const CropPlan &p, const HashCall &c, const HashKnobs &k, const std::vector<uint32_t> &crops)
{
    const uint32_t w = c.w, h = c.h;
    if (p.kind == CropPlan::kSmall) {
        CHECK(h <= 128 && w <= 256 && k.resize_mode == 0 && !k.no_smallcrop, "%s %ux%u: small-frame route", what, w, h);
        return;
    }
    CHECK(p.kind == CropPlan::kParts, "%s %ux%u: valid boxes must plan", what, w, h);
    std::vector<int> seen(c.n_clips, 0);
    for (uint32_t i : p.rows) seen[i]++;
    for (const CropBoxGroup &g : p.groups)
        for (uint32_t i : g.ids) seen[i]++;
    for (uint32_t i : p.rest) seen[i]++;
    size_t once = 0;
    for (int s : seen) once += s == 1;
    CHECK(once == c.n_clips, "%s %ux%u: %zu of %zu clips in exactly one part", what, w, h, once, c.n_clips);
    const bool ends16 = ((uint64_t)w * h) % 16 == 0, base16 = ((uintptr_t)c.base | c.frame_stride | c.clip_stride) % 16 == 0;
    CHECK(p.rows.empty() == (p.rows_kernel.route == HashRoute::kRefused), "%s %ux%u: a ROWCROP launch has a kernel and clips", what, w, h);
    if (!p.rows.empty()) {
        CHECK(p.rows_kernel.route == HashRoute::kWaveStream || p.rows_kernel.route == HashRoute::kChunkStream || p.rows_kernel.route == HashRoute::kKsplit, "%s %ux%u: ROWCROP kernel", what, w, h);
        check_stream_route(p.rows_kernel, c, k, what);
        CHECK(k.resize_mode == 0 && !k.no_rowcrop && h > 128 && (resize_rowcrop_streams(w) || k.rowcrop_all), "%s %ux%u: ROWCROP launch against the knobs", what, w, h);
        for (uint32_t i : p.rows) CHECK(crops[4 * i] == 0 && crops[4 * i + 1] == 0, "%s %ux%u: a box with side bars on the ROWCROP launch", what, w, h);
    }
    CHECK(p.groups.size() <= kMaxCropBoxGroups, "%s %ux%u: at most 16 column-range launches", what, w, h);
    if (!p.groups.empty()) CHECK(k.resize_mode == 0 && !k.no_rowcrop && !k.no_boxstream && h > 128 && ends16 && base16, "%s %ux%u: box launches against the knobs", what, w, h);
    std::set<uint64_t> ranges;
    for (const CropBoxGroup &g : p.groups) {
        CHECK(g.ids.size() >= kMinCropBoxGroupClips && g.waves != 0 && g.waves == resize_wavestream_waves_box(w, g.x0, g.box_w, k.wavestream_knob) && g.box_w < w && g.x0 + g.box_w <= w,
              "%s %ux%u: column range (%u, %u) with %zu clips and %d waves", what, w, h, g.x0, g.box_w, g.ids.size(), g.waves);
        CHECK(ranges.insert(crop_range_key(g.x0, g.box_w)).second, "%s %ux%u: one launch per column range", what, w, h);
        for (uint32_t i : g.ids) CHECK(crops[4 * i] == g.x0 && w - crops[4 * i] - crops[4 * i + 1] == g.box_w, "%s %ux%u: a box outside its launch's column range", what, w, h);
    }
    if (p.rest_gather) {
        int cls = 0;
        CHECK(!p.rest.empty() && (k.resize_mode == 0 || k.resize_mode == 5) && h > 128 && ends16 && ((uintptr_t)c.base | c.frame_stride | c.clip_stride) % 4 == 0 &&
              resize_cropped_stream_class(w, &cls) && cls == p.gather_cls, "%s %ux%u: gather stream kernel on an ineligible call", what, w, h);
        bool shift = w % 4 != 0;
        for (uint32_t i : p.rest) {
            uint32_t wp = 0;
            const uint32_t x0 = crops[4 * i], bw = w - x0 - crops[4 * i + 1], bh = h - crops[4 * i + 2] - crops[4 * i + 3];
            const uint32_t nb = resize_cropped_stream_blocks(bw, x0, w, p.gather_cls, &wp);
            CHECK(nb >= 1 && (nb >= 2 || bh <= 16), "%s %ux%u: box %u wide at %u does not fit the gather kernel's chunks", what, w, h, bw, x0);
            shift = shift || x0 % 4 != 0;
        }
        CHECK(shift == p.gather_shift, "%s %ux%u: operand shift", what, w, h);
    }
}

static void check_cropped_plans()
{
    const uint32_t sizes[][2] = {{64, 48}, {128, 96}, {256, 128}, {426, 240}, {640, 360}, {720, 576}, {854, 480}, {1024, 576}, {1280, 720}, {1366, 768}, {1920, 1080}, {2560, 1440}};  // CROP_SIZES
    const std::vector<KnobCase> knobs = knob_cases();
    uint32_t seed = 12345;
    const auto rnd = [&](uint32_t n) { seed = seed * 1664525u + 1013904223u; return (seed >> 8) % n; };
    for (const auto &wh : sizes) {
        const uint32_t w = wh[0], h = wh[1];
        const size_t n = 200;
        // top / bottom only; side bars, one shared range; side bars, unique ranges; mixed (a pool of boxes and no box, as the sweep's per_clip kind); 40 ranges of 5 clips
        for (int kind = 0; kind < 5; kind++) {
            std::vector<uint32_t> crops(4 * n, 0);
            const uint32_t pool[4][4] = {{0, 0, h / 8, h / 8}, {w / 8, w / 8, 0, 0}, {w / 5 + 1, w / 7, h / 9, 3}, {0, 0, 0, h - 20}};
            for (size_t i = 0; i < n; i++) {
                uint32_t *b = &crops[4 * i];
                if (kind == 0) { b[2] = rnd(h / 2); b[3] = rnd(h / 2 - 1) + (b[2] == 0); }
                if (kind == 1) { b[0] = w / 8; b[1] = w / 8; b[2] = rnd(h / 3); }
                if (kind == 2) { b[0] = 1 + (uint32_t)i % (w / 3); b[1] = rnd(w / 3); b[3] = rnd(h / 2); }
                if (kind == 3 && rnd(5) != 0) for (int q = 0, s = (int)rnd(4); q < 4; q++) b[q] = pool[s][q];
                if (kind == 4) { b[0] = 1 + (uint32_t)(i / 5); b[1] = 2; }
            }
            if (kind == 3) crops[0] = 1;  // (not all zero)
            for (const KnobCase &kc : knobs)
                for (int geom = 0; geom < 2; geom++) {
                    const HashCall c = packed_call(w, h, n, kAligned + 4 * geom);
                    const CropPlan p = plan_cropped(c, kc.k, crops.data());
                    check_crop_plan(kc.name, p, c, kc.k, crops);
                    if (p.kind != CropPlan::kParts) continue;
                    const HashKnobs &k = kc.k;
                    if (k.no_rowcrop || k.resize_mode != 0) CHECK(p.rows.empty() && p.groups.empty() && p.rest.size() == n, "%s %ux%u: everything through one general kernel", kc.name, w, h);
                    if (k.no_boxstream) CHECK(p.groups.empty(), "%s %ux%u: VDF_NO_BOXSTREAM", kc.name, w, h);
                    if (k.resize_mode == 4 || geom == 1) CHECK(!p.rest_gather || geom == 1, "%s %ux%u: mode 4 is the whole-line cropped kernel", kc.name, w, h);
                    if (k.resize_mode == 5 && geom == 0 && ((uint64_t)w * h) % 16 == 0 && kind != 2 && h > 128 && w <= 1984) CHECK(p.rest_gather, "%s %ux%u: mode 5 is the gather stream kernel", kc.name, w, h);
                    if (geom == 1) CHECK(p.rows.empty() && p.groups.empty(), "%s %ux%u: a base off 16 bytes streams nowhere", kc.name, w, h);
                    // the documented default routes
                    if (k.resize_mode == 0 && !k.no_rowcrop && !k.no_boxstream && geom == 0 && k.wavestream_knob == 0) {
                        if (kind == 0 && h > 128) CHECK(p.rows.size() == n && p.rest.empty(), "%s %ux%u: top / bottom bars stream as shorter frames", kc.name, w, h);
                        if (kind == 1 && w - w / 8 * 2 >= 513) CHECK(p.groups.size() == 1 && p.groups[0].ids.size() == n, "%s %ux%u: a shared column range is one box launch", kc.name, w, h);
                        if (kind == 2 && w / 3 >= 200) CHECK(p.groups.empty() && p.rest.size() == n, "%s %ux%u: unique column ranges go to the general kernel", kc.name, w, h);
                        if (kind == 4 && w >= 640 && w <= 1920) CHECK(p.groups.size() == kMaxCropBoxGroups && p.rest.size() == n - 5 * kMaxCropBoxGroups, "%s %ux%u: the ranges beyond sixteen go to the general kernel", kc.name, w, h);
                    }
                    // what the tables may show: each fact moves its clips, and only them
                    CropTableFit fit;
                    fit.rows_table = false;
                    CropPlan q = plan_cropped(c, kc.k, crops.data(), fit);
                    check_crop_plan("no rows table", q, c, kc.k, crops);
                    CHECK(q.rows.empty() && q.groups.size() == p.groups.size(), "%s %ux%u: without the rows table the full-width boxes take the general kernel", kc.name, w, h);
                    fit = CropTableFit();
                    fit.height_tables = false;
                    q = plan_cropped(c, kc.k, crops.data(), fit);
                    check_crop_plan("no height table", q, c, kc.k, crops);
                    CHECK(q.rows.empty() && q.groups.empty() && q.rest.size() == n, "%s %ux%u: a box height without a table sends the whole call through one general kernel", kc.name, w, h);
                    fit = CropTableFit();
                    fit.gather_tables = false;
                    q = plan_cropped(c, kc.k, crops.data(), fit);
                    check_crop_plan("no gather tables", q, c, kc.k, crops);
                    CHECK(!q.rest_gather && q.rows.size() == p.rows.size() && q.groups.size() == p.groups.size(), "%s %ux%u: without its tables the rest takes the whole-line kernel", kc.name, w, h);
                    if (!p.groups.empty()) {
                        fit = CropTableFit();
                        fit.ranges_without_table.push_back(crop_range_key(p.groups[0].x0, p.groups[0].box_w));
                        q = plan_cropped(c, kc.k, crops.data(), fit);
                        check_crop_plan("range without table", q, c, kc.k, crops);
                        for (const CropBoxGroup &g : q.groups) CHECK(crop_range_key(g.x0, g.box_w) != fit.ranges_without_table[0], "%s %ux%u: a range without a band table has no launch", kc.name, w, h);
                        CHECK(q.rest.size() >= p.groups[0].ids.size(), "%s %ux%u: ... its clips take the general kernel", kc.name, w, h);
                    }
                }
        }
        std::vector<uint32_t> bad(4 * n, 0);
        bad[4 * 7 + 0] = w / 2; bad[4 * 7 + 1] = w - w / 2;
        if (h > 128) CHECK(plan_cropped(packed_call(w, h, n), HashKnobs(), bad.data()).kind == CropPlan::kBadBox, "%ux%u: a box that leaves no pixels", w, h);
    }
}

int main()
{
    check_plain_plans();
    check_documented_routes();
    check_cropped_plans();
    const uint8_t *aligned = reinterpret_cast<const uint8_t *>(uintptr_t(0x10000));
    for (uint32_t w = 1; w <= 4200; w++) {
        // ---- stream kernel
        const uint32_t wp = stream_pitch(w);
        CHECK(wp % 16 == 0 && wp >= w, "pitch %u -> %u", w, wp);
        if (w % 16 != 0) {
            CHECK((wp / 16) % 2 == 1, "re-pitched rows must fall in 16 different bank groups: %u -> %u", w, wp);
            CHECK(wp >= w + (w % 4 ? 3u : 0u) && wp < w + 48, "pitch holds the row and the dword-alignment slack: %u -> %u", w, wp);
        } else if (w % 256 == 0 && w >= 768) {
            CHECK(wp == w + 16, "multiples of 256 are re-pitched: %u -> %u", w, wp);
        } else {
            CHECK(wp == w, "other multiples of 16 keep their pitch: %u -> %u", w, wp);
        }
        uint32_t nb = 0;
        const int cls = stream_class(w, &nb);
        const int n_kt = (int)((w + 63) / 64);
        if (cls) {
            const int buf = cls == 1 ? kStreamBufS : kStreamBufM;
            CHECK(nb >= (cls == 1 ? 4u : 2u) && nb <= 4, "blocks per chunk w=%u cls=%d nb=%u", w, cls, nb);
            // every DMA instruction fills a whole KB of LDS, and the last operand read may run 64 + 16 + 3 bytes past the chunk
            CHECK(((16 * nb * wp + 1023) & ~1023u) + 128 <= (uint32_t)buf, "chunk fits its buffer w=%u cls=%d nb=%u wp=%u", w, cls, nb, wp);
            CHECK(cls == 3 ? n_kt > kStreamTabM : n_kt <= (cls == 1 ? kStreamTabS : kStreamTabM), "table class w=%u cls=%d n_kt=%d", w, cls, n_kt);
            CHECK(resize_stream_wants_band(w) == resize_wavestream_applies(w), "band flag w=%u", w);
        }
        for (uint32_t h : {129u, 270u, 1080u, 1088u}) {
            const size_t fs = (size_t)w * h;
            const bool e = resize_stream_eligible(aligned, w, h, (fs + 15) & ~size_t(15), 16 * ((fs + 15) & ~size_t(15)));
            if (e) CHECK((cls == 1 || resize_wavestream_applies(w)) && w >= 64, "eligible implies a kernel w=%u", w);
            if ((cls == 1 || resize_wavestream_applies(w)) && w >= 64 && ((uint64_t)w * h) % 16 == 0) CHECK(e, "every width of the chunk or per-wave form streams w=%u", w);
            if (cls != 1 && !resize_wavestream_applies(w)) CHECK(!e, "widths beyond the per-wave buffers (pitch > 2368) do not stream w=%u", w);
            if (((uint64_t)w * h) % 16 != 0) CHECK(!e, "frames that do not end on a 16-byte boundary must not stream w=%u h=%u", w, h);
            CHECK(!resize_stream_eligible(aligned + 4, w, h, fs, 16 * fs), "misaligned base must not stream w=%u", w);
        }
        // ---- K-split kernel
        if (w % 16 == 0 && w >= 1024 && w <= 4096) {
            uint32_t kp = 0;
            const uint32_t knb = ksplit_geometry(w, &kp);
            CHECK(kp % 16 == 0 && (kp / 16) % 2 == 1 && kp >= w && kp <= w + 16, "k-split pitch %u -> %u", w, kp);
            CHECK(knb >= 1 && knb <= 4 && ((16 * knb * kp + 1023) & ~1023u) + 128 <= (uint32_t)kKsplitBuf, "k-split chunk w=%u nb=%u", w, knb);
            CHECK(n_kt <= 64, "k-split tiles per wave w=%u", w);
            CHECK(resize_ksplit_eligible(aligned, w, 1080, (size_t)w * 1080, (size_t)w * 1080 * 16), "k-split eligible w=%u", w);
        } else {
            CHECK(!resize_ksplit_eligible(aligned, w, 1080, (size_t)w * 1080, (size_t)w * 1080 * 16), "k-split must refuse w=%u", w);
        }
        // ---- cropped stream kernel: every crop box of an eligible pitch must fit with at least one block
        int ccls = 0;
        if (resize_cropped_stream_class(w, &ccls)) {
            CHECK(ccls == 1 || ccls == 2, "cropped class pitch=%u", w);
            for (uint32_t cw : {1u, 17u, w / 3 + 1, w - 1, w}) {
                for (uint32_t x0 : {0u, 1u, 5u}) {
                    if (cw == 0 || x0 + cw > w) continue;
                    uint32_t cp = 0;
                    const uint32_t cnb = resize_cropped_stream_blocks(cw, x0, w, ccls, &cp);
                    const bool linear = x0 == 0 && cw == w && w % 16 == 0 && w % 256 != 0;
                    CHECK(cp % 16 == 0 && (linear ? cp == w : (cp >= cw + 3 && (cp / 16) % 2 == 1)), "crop pitch pitch=%u cw=%u x0=%u -> %u", w, cw, x0, cp);
                    CHECK(cnb >= 1 && ((16 * cnb * cp + 1023) & ~1023u) + 128 <= (uint32_t)(ccls == 1 ? kStreamBufS : kStreamBufM),
                          "crop chunk pitch=%u cw=%u nb=%u cp=%u", w, cw, cnb, cp);
                }
            }
        }
    }
    // the sizes DESIGN.md names
    struct { uint32_t w; int cls; uint32_t nb; } want[] = {{480, 1, 4}, {426, 1, 4}, {854, 2, 4}, {960, 2, 4}, {640, 2, 4}, {768, 2, 4}, {1024, 2, 3},
                                                            {1280, 3, 3}, {1440, 3, 2}, {1920, 3, 2}, {1366, 3, 2}};
    for (auto &q : want) {
        uint32_t nb = 0;
        const int cls = stream_class(q.w, &nb);
        CHECK(cls == q.cls && nb == q.nb, "w=%u: class %d nb %u, expected %d %u", q.w, cls, nb, q.cls, q.nb);
    }
    for (uint32_t w : {480u, 854u, 640u, 768u, 1024u, 1280u, 1920u, 720u, 1440u, 240u, 160u, 128u, 1536u, 1792u})  // 1536 / 1792: per-wave block streams (round 3)
        CHECK(resize_stream_eligible(aligned, w, 1080, (size_t)w * 1080, (size_t)w * 1080 * 16), "%u wide should stream by default", w);
    for (uint32_t w : {2048u, 2560u, 3840u, 48u, 63u})
        CHECK(!resize_stream_eligible(aligned, w, 1080, (size_t)w * 1080, (size_t)w * 1080 * 16), "%u wide should not stream by default", w);
    // short frames (at most 128 rows: the fused kernel's range): the wide ones stream (round 5, measured)
    struct { uint32_t w, h; bool stream; } shorts[] = {{64, 64, false}, {128, 128, false}, {160, 90, false}, {128, 96, false}, {192, 80, false}, {512, 64, false},
                                                       {160, 120, false}, {192, 108, false}, {208, 112, false}, {208, 117, true}, {192, 128, true}, {200, 112, true}, {224, 126, true},
                                                       {256, 128, true}, {320, 96, true}, {480, 128, true},
                                                       {640, 120, true}, {854, 128, true}, {1920, 128, true}, {1920, 64, true}, {1920, 48, false}, {1920, 129, false}};
    for (auto &q : shorts) CHECK(resize_short_prefers_stream(q.w, q.h) == q.stream, "short frame %u x %u: stream %d", q.w, q.h, (int)q.stream);
    struct { uint32_t w, h; bool tiled; } talls[] = {{64, 160, true}, {64, 256, true}, {128, 256, true}, {176, 144, true}, {160, 200, true}, {16, 200, true}, {176, 208, false},
                                                     {192, 144, false}, {240, 160, false}, {64, 257, false}, {64, 128, false}, {100, 200, true}, {90, 250, true}, {144, 256, false}};
    for (auto &q : talls) CHECK(resize_tall_prefers_tiled(q.w, q.h) == q.tiled, "tall frame %u x %u: tiled %d", q.w, q.h, (int)q.tiled);
    // the per-wave block streams: every M-class width (from 462 columns) whose pitch is at most 1920, with as many waves as block buffers fit; the (whole-KB) block
    // fits the wave's buffer, the workgroup fits the CU's LDS, and the width's band table fits the table array of that wave count
    for (uint32_t w = 1; w <= 4200; w++) {
        uint32_t nb = 0;
        const int cls = stream_class(w, &nb);
        const int nw = resize_wavestream_waves(w);
        CHECK(resize_wavestream_applies(w) == (nw != 0), "applies <-> waves w=%u", w);
        if (nw) {
            CHECK(cls != 1 && w >= 256 && stream_pitch(w) <= 2368, "wave-stream width w=%u cls=%d nb=%u", w, cls, nb);
            CHECK(nw == 3 || nw == 4 || nw == 5 || nw == 6 || nw == 8, "wave count w=%u nw=%d", w, nw);
            CHECK((nw == 3) == (stream_pitch(w) > 1920) && (nw != 3 || w % 16 != 0), "three waves beyond the four-wave buffers, widths the K-split form cannot take w=%u nw=%d", w, nw);
            const int buf = nw == 3 ? kWaveStreamBuf3 : nw == 4 ? kWaveStreamBuf : nw == 5 ? kWaveStreamBuf5 : nw == 6 ? kWaveStreamBuf6 : kWaveStreamBuf8;
            const int tab = nw <= 4 ? kWaveStreamTabBytes : nw == 5 ? kWaveStreamTabMid : kWaveStreamTabSmall;
            CHECK(((16 * stream_pitch(w) + 1023) & ~1023u) + 128 <= (uint32_t)buf, "wave-stream block fits w=%u nw=%d", w, nw);
            CHECK(nw * buf + tab + 2 * (nw - 1) * 1024 <= kLdsPerCu, "wave-stream workgroup fits the LDS w=%u nw=%d", w, nw);
            MfmaAxisTable t;
            build_mfma_axis_table(w, kMfmaLayoutHorizontalBand, t);
            CHECK(t.ok && 16 * t.band_stride + 128 <= tab, "band table fits w=%u nw=%d: %d bytes of %d", w, nw, 16 * t.band_stride + 128, tab);
        } else if (w >= 256 && stream_pitch(w) <= 2368) {
            CHECK(cls == 1 || (w % 16 == 0 && w > 1920), "every width beyond the S class with a pitch up to 2368 takes the per-wave streams or the K-split form w=%u cls=%d", w, cls);
        }
    }
    for (uint32_t w : {528u, 640u, 854u, 1024u, 1280u, 1360u, 1366u, 1440u, 1536u, 1600u, 1680u, 1792u, 1904u, 1920u}) CHECK(resize_wavestream_applies(w), "%u wide takes the per-wave streams", w);
    for (uint32_t w : {480u, 320u, 1936u, 2048u, 2353u, 2560u, 3840u}) CHECK(!resize_wavestream_applies(w), "%u wide must not take the per-wave streams", w);
    CHECK(resize_wavestream_waves(640) == 8 && resize_wavestream_waves(1152) == 6 && resize_wavestream_waves(1366) == 5 && resize_wavestream_waves(1920) == 4 &&
          resize_wavestream_waves(1950) == 3 && resize_wavestream_waves(2340) == 3 && resize_wavestream_waves(2000) == 0 && resize_wavestream_waves(1915) == 3, "documented wave counts");
    // full-width crop boxes: the ROWCROP stream kernels everywhere but 2048 columns (measured)
    for (uint32_t w : {64u, 426u, 640u, 768u, 854u, 1024u, 1280u, 1366u, 1536u, 1600u, 1792u, 1920u, 2560u, 3840u, 4096u}) CHECK(resize_rowcrop_streams(w), "%u wide: row-cropped stream kernels", w);
    CHECK(!resize_rowcrop_streams(2048), "2048 wide: general cropped kernels");
    // crop boxes that share their column range, through the per-wave kernel: the LDS pitch holds the box and the up to 3 bytes in front of a
    // row that starts off a dword, is an odd multiple of 16, and the (whole-KB) block fits the buffer of the chosen wave count
    for (uint32_t fw : {640u, 854u, 1280u, 1366u, 1920u, 1921u, 2048u, 3840u})
        for (uint32_t x0 : {0u, 1u, 3u, 4u, 16u, 240u, 241u})
            for (uint32_t bw = 500; x0 + bw <= fw; bw += 37) {
                int mode = -1;
                const uint32_t wp = box_stream_pitch(fw, x0, bw, &mode);
                const bool whole = x0 == 0 && bw == fw, shifted = fw % 4 != 0 || x0 % 4 != 0;
                if (!whole) {
                    CHECK(mode == (shifted ? 2 : 1) && wp % 16 == 0 && (wp / 16) % 2 == 1 && wp >= bw + (shifted ? 3u : 0u) && wp < bw + 48,
                          "box pitch fw=%u x0=%u bw=%u -> %u mode %d", fw, x0, bw, wp, mode);
                }
                const int nw = resize_wavestream_waves_box(fw, x0, bw);
                if (nw && !whole) {
                    const int buf = nw == 3 ? kWaveStreamBuf3 : nw == 4 ? kWaveStreamBuf : nw == 5 ? kWaveStreamBuf5 : nw == 6 ? kWaveStreamBuf6 : kWaveStreamBuf8;
                    CHECK(bw >= 513 && ((16 * wp + 1023) & ~1023u) + 128 <= (uint32_t)buf, "box block fits fw=%u x0=%u bw=%u nw=%d", fw, x0, bw, nw);
                }
                if (!whole && bw >= 513 && wp <= 2368) CHECK(nw != 0, "boxes up to pitch 2368 take the per-wave kernel fw=%u x0=%u bw=%u", fw, x0, bw);
            }
    uint32_t kp = 0;
    CHECK(ksplit_geometry(3840, &kp) == 1 && kp == 3856, "4K: one 16-row block per chunk at pitch 3856");
    CHECK(ksplit_geometry(2048, &kp) == 2 && kp == 2064, "2048 wide: two blocks per chunk");
    if (fails == 0) std::printf("resize dispatch ok\n");
    return fails ? 1 : 0;
}
