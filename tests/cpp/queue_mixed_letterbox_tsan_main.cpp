// The mixed-size batching queue with Cropdetect::Letterbox (csrc/hash_queue_mixed.cpp: vdf_hash_queue_create_mixed_letterbox, vdf_hash_queue_mixed_submit_crop)
// under ThreadSanitizer, the pattern of queue_mixed_tsan_main.cpp: the GPU behind the queue is replaced by stand-ins for BOTH batch calls.  A letterbox queue and
// a plain queue are alive together and 48 callers with five clip sizes submit to both; every clip's "hash" is a checksum of its bytes and its "crop" a function
// of that checksum, so a wrong hand-over - another caller's hash or box, a box from the plain call, a batch sent to the wrong call - is a wrong value.  Thread 0
// also submits clips larger than the staging, refused while others are in flight.  A lost wake-up is a hang (the test's timeout), an unlocked access a TSan
// report.  Built by tests/test_hash_queue_mixed_letterbox_tsan.py - no GPU, no libvdf_hip.so.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "../../vid_dup_finder_lib_amd/csrc/vdf_ctx.h"

vdf_ctx::~vdf_ctx() {}  // (api.cpp's releases device objects; the stand-in contexts own none)

static std::atomic<int> g_plain_calls{0}, g_letterbox_calls{0}, g_bad_batches{0};
static std::atomic<size_t> g_limit_bytes{0};
static std::atomic<uint32_t> g_limit_clips{0};

static uint64_t checksum(const uint8_t *p, size_t n)
{
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}
static void crop_of(uint64_t sum, uint32_t crop[4])
{
    for (int k = 0; k < 4; k++) crop[k] = (uint32_t)((sum >> (13 * k)) & 0x3FFu) + 1u;  // never all zero: a plain queue's zeros cannot pass for it
}

// the batch as the queue must build it: descriptors inside the buffer, in order, 64-byte aligned, whole frames, no caller-supplied box
static bool batch_ok(const vdf_clip *clips, size_t n, size_t buf_bytes, uint32_t frames_per_clip)
{
    bool ok = frames_per_clip == 16 && n >= 1 && n <= g_limit_clips.load() && buf_bytes <= ((g_limit_bytes.load() + 63) & ~(size_t)63);
    uint64_t end = 0;
    for (size_t i = 0; i < n && ok; i++) {
        const size_t bytes = (size_t)clips[i].w * clips[i].h * 16;
        ok = clips[i].offset >= end && clips[i].offset % 64 == 0 && clips[i].offset + bytes <= buf_bytes && clips[i].frame_stride == (uint64_t)clips[i].w * clips[i].h &&
             (clips[i].crop_left | clips[i].crop_right | clips[i].crop_top | clips[i].crop_bottom) == 0;
        end = clips[i].offset + bytes;
    }
    return ok;
}

extern "C" {
int vdf_ctx_create(int device_id, vdf_ctx **out) { *out = new vdf_ctx(); (*out)->device = device_id; return VDF_OK; }
void vdf_ctx_destroy(vdf_ctx *ctx) { delete ctx; }
int vdf_ctx_device_count(const vdf_ctx *) { return 1; }
int vdf_ctx_device_at(const vdf_ctx *, int) { return 0; }
int vdf_hash_clips_u8(vdf_ctx *, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, size_t n, uint32_t frames_per_clip, uint64_t *out, uint32_t *)
{
    g_plain_calls++;
    std::this_thread::sleep_for(std::chrono::microseconds(150 + 20 * n));
    const bool ok = batch_ok(clips, n, buf_bytes, frames_per_clip);
    for (size_t i = 0; i < n && ok; i++)
        for (int w = 0; w < VDF_HASH_WORDS; w++) out[i * VDF_HASH_WORDS + w] = checksum(buf + clips[i].offset, (size_t)clips[i].w * clips[i].h * 16) + (uint64_t)w;
    if (!ok) g_bad_batches++;
    return ok ? VDF_OK : VDF_E_INVAL;
}
int vdf_hash_clips_u8_letterbox(vdf_ctx *, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, size_t n, uint32_t frames_per_clip, uint64_t *out,
                                uint32_t *out_crops, uint32_t *)
{
    g_letterbox_calls++;
    std::this_thread::sleep_for(std::chrono::microseconds(200 + 25 * n));
    const bool ok = batch_ok(clips, n, buf_bytes, frames_per_clip) && out_crops != nullptr;
    for (size_t i = 0; i < n && ok; i++) {
        const uint64_t sum = checksum(buf + clips[i].offset, (size_t)clips[i].w * clips[i].h * 16);
        for (int w = 0; w < VDF_HASH_WORDS; w++) out[i * VDF_HASH_WORDS + w] = ~sum + (uint64_t)w;  // (not the plain call's words)
        crop_of(sum, out_crops + 4 * i);
    }
    if (!ok) g_bad_batches++;
    return ok ? VDF_OK : VDF_E_INVAL;
}
}

static const uint32_t kSizes[5][2] = {{8, 4}, {7, 5}, {16, 16}, {33, 9}, {40, 24}};  // 512 ... 15360 bytes per clip

static int run(int threads, size_t staging, uint32_t max_batch, uint32_t wait_us, int per_thread, uint32_t slots)
{
    g_limit_bytes = staging; g_limit_clips = max_batch; g_bad_batches = 0; g_plain_calls = 0; g_letterbox_calls = 0;
    vdf_ctx *ctx = nullptr;
    vdf_ctx_create(0, &ctx);
    vdf_hash_queue_mixed *ql = nullptr, *qp = nullptr;
    if (vdf_hash_queue_create_mixed_letterbox(ctx, staging, max_batch, wait_us, slots, &ql) != VDF_OK) return 1;
    if (vdf_hash_queue_create_mixed(ctx, staging, max_batch, wait_us, slots, &qp) != VDF_OK) return 1;
    std::atomic<int> wrong{0}, refused{0};
    std::atomic<uint64_t> to_letterbox{0}, to_plain{0};
    std::vector<std::thread> th;
    for (int t = 0; t < threads; t++)
        th.emplace_back([&, t] {
            std::mt19937 rng(500 + t);
            std::vector<uint8_t> c;
            for (int k = 0; k < per_thread; k++) {
                uint32_t w = kSizes[(t + k) % 5][0], h = kSizes[(t + k) % 5][1];
                const bool big = t == 0 && k % 7 == 3;
                if (big) { w = 64; h = (uint32_t)(staging / (64 * 16)) + 1; }
                c.resize((size_t)w * h * 16);
                for (auto &b : c) b = (uint8_t)rng();
                const int mode = (int)(rng() % 3);  // 0: letterbox queue with the box, 1: letterbox queue through the plain submit, 2: plain queue with a box asked for
                uint64_t out[VDF_HASH_WORDS];
                uint32_t crop[4] = {9999, 9999, 9999, 9999};
                const int rc = mode == 0   ? vdf_hash_queue_mixed_submit_crop(ql, c.data(), w, h, out, crop)
                               : mode == 1 ? vdf_hash_queue_mixed_submit(ql, c.data(), w, h, out)
                                           : vdf_hash_queue_mixed_submit_crop(qp, c.data(), w, h, out, crop);
                if (big) {
                    if (rc != VDF_E_INVAL) wrong++;
                    refused++;
                    continue;
                }
                if (rc != VDF_OK) { wrong++; return; }
                (mode == 2 ? to_plain : to_letterbox)++;
                const uint64_t sum = checksum(c.data(), c.size());
                uint32_t want_crop[4] = {0, 0, 0, 0};
                if (mode == 0) crop_of(sum, want_crop);
                if (mode == 1) std::fill(want_crop, want_crop + 4, 9999u);  // untouched: the plain submit drops the box
                for (int i = 0; i < VDF_HASH_WORDS; i++) if (out[i] != (mode == 2 ? sum : ~sum) + (uint64_t)i) wrong++;
                for (int i = 0; i < 4; i++) if (crop[i] != want_crop[i]) wrong++;
                if (rng() % 7 == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 300));
            }
        });
    for (auto &x : th) x.join();
    uint64_t nbl = 0, ncl = 0, nbp = 0, ncp = 0;
    vdf_hash_queue_mixed_stats(ql, &nbl, &ncl);
    vdf_hash_queue_mixed_stats(qp, &nbp, &ncp);
    const bool ok = wrong == 0 && g_bad_batches == 0 && ncl == to_letterbox.load() && ncp == to_plain.load() && refused.load() > 0 &&
                    ncl + ncp == (uint64_t)threads * per_thread - (uint64_t)refused.load() && nbl == (uint64_t)g_letterbox_calls.load() && nbp == (uint64_t)g_plain_calls.load() &&
                    nbl > 0 && nbp > 0;
    std::printf("threads %d staging %zu max_batch %u wait %u us: letterbox queue %llu clips in %llu batches, plain queue %llu in %llu, %d refused, %d wrong%s\n", threads,
                staging, max_batch, wait_us, (unsigned long long)ncl, (unsigned long long)nbl, (unsigned long long)ncp, (unsigned long long)nbp, refused.load(), wrong.load(),
                ok ? "" : "  <-- FAILED");
    vdf_hash_queue_mixed_destroy(ql);
    vdf_hash_queue_mixed_destroy(qp);
    vdf_ctx_destroy(ctx);
    return ok ? 0 : 1;
}

int main()
{
    int bad = 0;
    bad += run(48, 1 << 20, 4, 200, 60, 0);    // 48 callers, five clip sizes, batches of 4: most sleep for a free slot
    bad += run(48, 20000, 64, 2000, 40, 0);    // a byte budget closes batches before count or deadline
    bad += run(33, 1 << 16, 8, 2000, 50, 3);   // three slots
    // arguments
    vdf_ctx *ctx = nullptr;
    vdf_ctx_create(0, &ctx);
    vdf_hash_queue_mixed *q = nullptr;
    uint64_t out[VDF_HASH_WORDS];
    uint32_t crop[4];
    uint8_t px[16] = {0};
    bad += vdf_hash_queue_create_mixed_letterbox(ctx, 0, 4, 0, 0, &q) != VDF_E_INVAL;
    bad += vdf_hash_queue_create_mixed_letterbox(ctx, 4096, 0, 0, 0, &q) != VDF_E_INVAL;
    bad += vdf_hash_queue_create_mixed_letterbox(ctx, 4096, 4, 0, 17, &q) != VDF_E_INVAL;
    bad += vdf_hash_queue_create_mixed_letterbox(nullptr, 4096, 4, 0, 1, &q) != VDF_E_INVAL;
    bad += vdf_hash_queue_create_mixed_letterbox(ctx, 16, 4, 0, 1, &q) != VDF_OK;
    bad += vdf_hash_queue_mixed_submit_crop(nullptr, px, 1, 1, out, crop) != VDF_E_INVAL;
    bad += vdf_hash_queue_mixed_submit_crop(q, px, 0, 1, out, crop) != VDF_E_INVAL;
    bad += vdf_hash_queue_mixed_submit_crop(q, px, 1, 2, out, crop) != VDF_E_INVAL;  // 32 bytes into 16
    g_limit_bytes = 16; g_limit_clips = 4;
    bad += vdf_hash_queue_mixed_submit_crop(q, px, 1, 1, out, nullptr) != VDF_OK;    // the box is optional
    bad += vdf_hash_queue_mixed_submit_crop(q, px, 1, 1, out, crop) != VDF_OK || crop[0] == 0;
    vdf_hash_queue_mixed_destroy(q);
    vdf_ctx_destroy(ctx);
    std::puts(bad ? "queue mixed letterbox tsan FAILED" : "queue mixed letterbox tsan ok");
    return bad ? 1 : 0;
}
