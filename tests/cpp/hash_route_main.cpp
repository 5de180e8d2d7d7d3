// Host-only front end of the hash planner (csrc/resize_dispatch.cpp: plan_hash) for tests/test_hash_route_table.py: which kernel, and which
// instantiation of it, a frame size takes under a set of knobs.  Reads lines of
//     w h resize_mode wavestream_knob no_persistent
// (the HashKnobs fields VDF_RESIZE_MODE, VDF_WAVESTREAM_NW / VDF_NO_WAVESTREAM = -1 and VDF_HASH_NO_PERSISTENT set) and prints, for a packed call of
// 1000 clips on a 16-byte-aligned base, one line of key=value fields: the route's name, the plan's values and the LDS row pitch of the stream
// forms (shift = rows that start off a dword: the operands are shifted by 0..3 bytes).  With the argument "crop": plan_cropped, see crop_mode().
// Built with g++ (no HIP).
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../vid_dup_finder_lib_amd/csrc/resize_dispatch.h"

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

// "crop" mode: lines of  w h resize_mode n_clips  followed by n_clips x (left right top bottom); prints plan_cropped's parts for a packed, aligned call
static int crop_mode()
{
    unsigned w, h, n;
    int mode;
    while (std::scanf("%u %u %d %u", &w, &h, &mode, &n) == 4) {
        std::vector<uint32_t> crops(4 * (size_t)n);
        for (uint32_t &v : crops)
            if (std::scanf("%u", &v) != 1) return 1;
        HashKnobs k;
        k.resize_mode = mode;
        const HashCall c{reinterpret_cast<const uint8_t *>(uintptr_t(0x10000)), w, h, (size_t)w * h, (size_t)w * h * 16, n};
        const CropPlan p = plan_cropped(c, k, crops.data());
        size_t group_clips = 0;
        for (const CropBoxGroup &g : p.groups) group_clips += g.ids.size();
        std::printf("w=%u h=%u kind=%s rows_route=%s rows_waves=%d rows=%zu groups=%zu group_clips=%zu group_waves=%d rest=%zu rest_gather=%d gather_shift=%d\n", w, h,
                    p.kind == CropPlan::kBadBox ? "kBadBox" : p.kind == CropPlan::kSmall ? "kSmall" : "kParts", route_name(p.rows_kernel.route), p.rows_kernel.waves, p.rows.size(),
                    p.groups.size(), group_clips, p.groups.empty() ? 0 : p.groups[0].waves, p.rest.size(), (int)p.rest_gather, (int)(p.rest_gather && p.gather_shift));
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "crop") == 0) return crop_mode();
    // every HashRoute, for the test's "every route but kRefused and kDirect16": the enum's values from its first to its last, kScalar (a route
    // appended behind kScalar has to move this bound; -Wswitch makes it enter route_name)
    std::printf("routes");
    for (int r = (int)HashRoute::kRefused; r <= (int)HashRoute::kScalar; r++) std::printf(" %s", route_name((HashRoute)r));
    std::printf("\ntiled");  // every <NKT, NRG> with an instantiation (kTiledWaves != 0)
    for (int nkt = 1; nkt <= 4; nkt++)
        for (int nrg : {1, 2, 4})
            if (tiled_waves(nkt, nrg)) std::printf(" %d,%d", nkt, nrg);
    std::printf("\n");
    unsigned w, h;
    int mode, knob, no_persistent;
    while (std::scanf("%u %u %d %d %d", &w, &h, &mode, &knob, &no_persistent) == 5) {
        HashKnobs k;
        k.resize_mode = mode;
        k.wavestream_knob = knob;
        k.hash_no_persistent = no_persistent != 0;
        const HashCall c{reinterpret_cast<const uint8_t *>(uintptr_t(0x10000)), w, h, (size_t)w * h, (size_t)w * h * 16, 1000};
        const HashPlan p = plan_hash(c, k);
        uint32_t pitch = 0;
        if (p.route == HashRoute::kChunkStream || p.route == HashRoute::kWaveStream) pitch = stream_pitch(w);
        if (p.route == HashRoute::kKsplit) ksplit_geometry(w, &pitch);
        std::printf("w=%u h=%u route=%s waves=%d tiled_nrg=%d n_kt=%d nb=%u full_tile=%d last_clip_apart=%d pitch=%u shift=%d\n", w, h, route_name(p.route), p.waves,
                    p.tiled_nrg, p.n_kt, p.nb, (int)p.full_tile, (int)p.last_clip_apart, pitch, (int)(pitch != 0 && w % 4 != 0));
    }
    return 0;
}
