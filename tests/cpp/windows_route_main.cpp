// Host-only front end of the windows calls' resize planning for tests/test_hash_windows_routes.py: the pseudo-clip runs of a call
// (csrc/windows_plan.h: plan_windows_resize, windows_resize_runs) and, for each run, the route plan_resize_only (csrc/resize_dispatch.cpp) gives it -
// exactly what api.cpp's hash_windows_locked launches.  stdin: one call per line, "w h mode knob no_persistent base_offset frame_pad clip_pad F n_clips";
// stdout: one line per call, "layout=<kPacked|kByClip|kByChunk> runs=<n> routes=<route of run 0>,<route of run 1>,...".
#include <cstdint>
#include <cstdio>

#include "resize_dispatch.h"
#include "windows_plan.h"

using namespace vdf;

static const char *route_name(HashRoute r)
{
    switch (r) {
    case HashRoute::kRefused: return "kRefused";
    case HashRoute::kDirect16: return "kDirect16";
    case HashRoute::kPersistentOneTile: return "kPersistentOneTile";
    case HashRoute::kTiled: return "kTiled";
    case HashRoute::kPerClipFused: return "kPerClipFused";
    case HashRoute::kChunkStream: return "kChunkStream";
    case HashRoute::kWaveStream: return "kWaveStream";
    case HashRoute::kKsplit: return "kKsplit";
    case HashRoute::kWholeLine: return "kWholeLine";
    case HashRoute::kScalar: return "kScalar";
    }
    return "?";
}

int main()
{
    unsigned w, h, F;
    int mode, knob, no_persistent;
    unsigned long base_offset, frame_pad, clip_pad, n_clips;
    while (std::scanf("%u %u %d %d %d %lu %lu %lu %u %lu", &w, &h, &mode, &knob, &no_persistent, &base_offset, &frame_pad, &clip_pad, &F, &n_clips) == 10) {
        HashKnobs k;
        k.resize_mode = mode;
        k.wavestream_knob = knob;
        k.hash_no_persistent = no_persistent != 0;
        const size_t fs = (size_t)w * h + frame_pad, cs = (size_t)F * fs + clip_pad;
        const uint8_t *base = reinterpret_cast<const uint8_t *>(uintptr_t(0x10000) + base_offset);
        const WindowsResizePlan rp = plan_windows_resize(n_clips, F, fs, cs);
        const auto runs = windows_resize_runs(rp, n_clips, F, fs, cs);
        std::printf("layout=%s runs=%zu routes=", rp.layout == WindowsResizePlan::kPacked ? "kPacked" : rp.layout == WindowsResizePlan::kByClip ? "kByClip" : "kByChunk",
                    runs.size());
        for (size_t i = 0; i < runs.size(); i++) {
            const HashCall c{base + runs[i].src_offset, w, h, fs, runs[i].step, runs[i].n};
            // both table answers a launch can meet: the plan itself, and the plan after a plain table did not fit - neither may fuse the DCT
            const HashPlan p = plan_resize_only(c, k), q = plan_resize_only(c, k, TableFit::kNoPlain);
            const bool fused = p.route == HashRoute::kPersistentOneTile || p.route == HashRoute::kTiled || p.route == HashRoute::kPerClipFused || p.route == HashRoute::kDirect16;
            if (fused || (q.route != HashRoute::kScalar && q.route != HashRoute::kRefused)) { std::printf("\nFAILED: a fused route, or kNoPlain not answered by kScalar / kRefused\n"); return 1; }
            if (p.route == HashRoute::kWholeLine && p.layout_v != kMfmaLayoutVerticalWide) { std::printf("\nFAILED: whole-line without the wide vertical layout\n"); return 1; }
            std::printf("%s%s", i ? "," : "", route_name(p.route));
        }
        std::printf("\n");
    }
    return 0;
}
