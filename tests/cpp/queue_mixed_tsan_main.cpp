// The mixed-size batching queue's host logic (csrc/hash_queue_mixed.cpp) under ThreadSanitizer, with the GPU behind it replaced by stand-ins, as
// queue_tsan_main.cpp does for hash_queue.cpp: vdf_ctx_create hands out an empty context, vdf_hash_clips_u8 "hashes" each clip of the batch to a
// checksum of its bytes (found through the batch's descriptors) after a short sleep, and checks the batch it is given: descriptors inside the
// buffer, no overlap, no more clips or bytes than the queue was made for.  A lost wake-up shows as a hang (the test's timeout), a wrong
// hand-over as a wrong checksum, an unlocked access as a TSan report.  Built by tests/test_hash_queue_mixed_tsan.py - no GPU, no libvdf_hip.so.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "../../vid_dup_finder_lib_amd/csrc/vdf_ctx.h"

vdf_ctx::~vdf_ctx() {}  // (api.cpp's releases device objects; the stand-in contexts own none)

static std::atomic<int> g_calls{0}, g_concurrent{0}, g_concurrent_max{0}, g_bad_batches{0}, g_batches_closed_by_bytes{0};
static std::atomic<size_t> g_limit_bytes{0};
static std::atomic<uint32_t> g_limit_clips{0};

static uint64_t checksum(const uint8_t *p, size_t n)
{
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

extern "C" {
int vdf_ctx_create(int device_id, vdf_ctx **out) { *out = new vdf_ctx(); (*out)->device = device_id; return VDF_OK; }
void vdf_ctx_destroy(vdf_ctx *ctx) { delete ctx; }
int vdf_ctx_device_count(const vdf_ctx *) { return 1; }
int vdf_ctx_device_at(const vdf_ctx *, int) { return 0; }
int vdf_hash_clips_u8(vdf_ctx *, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, size_t n, uint32_t frames_per_clip, uint64_t *out, uint32_t *)
{
    const int c = ++g_concurrent;
    int m = g_concurrent_max.load();
    while (c > m && !g_concurrent_max.compare_exchange_weak(m, c)) {}
    g_calls++;
    std::this_thread::sleep_for(std::chrono::microseconds(150 + 20 * n));
    bool ok = frames_per_clip == 16 && n >= 1 && n <= g_limit_clips.load() && buf_bytes <= ((g_limit_bytes.load() + 63) & ~(size_t)63);
    uint64_t end = 0;
    for (size_t i = 0; i < n; i++) {
        const size_t bytes = (size_t)clips[i].w * clips[i].h * 16;
        ok = ok && clips[i].offset >= end && clips[i].offset % 64 == 0 && clips[i].offset + bytes <= buf_bytes && clips[i].frame_stride == (uint64_t)clips[i].w * clips[i].h;
        end = clips[i].offset + bytes;
        if (!ok) break;
        for (int w = 0; w < VDF_HASH_WORDS; w++) out[i * VDF_HASH_WORDS + w] = checksum(buf + clips[i].offset, bytes) + (uint64_t)w;
    }
    if (n < g_limit_clips.load()) g_batches_closed_by_bytes++;  // (or by the deadline: the byte-budget run has none to speak of)
    if (!ok) g_bad_batches++;
    --g_concurrent;
    return ok ? VDF_OK : VDF_E_INVAL;
}
}

static const uint32_t kSizes[5][2] = {{8, 4}, {7, 5}, {16, 16}, {33, 9}, {40, 24}};  // 512 ... 15360 bytes per clip

// oversize: every seventh submission of thread 0 is a clip larger than the staging: refused at once, the others go on
static int run(int threads, size_t staging, uint32_t max_batch, uint32_t wait_us, int per_thread, uint32_t slots, bool oversize, bool expect_byte_cuts)
{
    g_limit_bytes = staging; g_limit_clips = max_batch; g_concurrent_max = 0; g_bad_batches = 0; g_batches_closed_by_bytes = 0;
    vdf_ctx *ctx = nullptr;
    vdf_ctx_create(0, &ctx);
    vdf_hash_queue_mixed *q = nullptr;
    if (vdf_hash_queue_create_mixed(ctx, staging, max_batch, wait_us, slots, &q) != VDF_OK) return 1;
    std::atomic<int> wrong{0}, refused{0};
    std::atomic<uint64_t> accepted{0};
    std::vector<std::thread> th;
    for (int t = 0; t < threads; t++)
        th.emplace_back([&, t] {
            std::mt19937 rng(100 + t);
            std::vector<uint8_t> c;
            for (int k = 0; k < per_thread; k++) {
                uint32_t w = kSizes[(t + k) % 5][0], h = kSizes[(t + k) % 5][1];
                const bool big = oversize && t == 0 && k % 7 == 3;
                if (big) { w = 64; h = (uint32_t)(staging / (64 * 16)) + 1; }
                c.resize((size_t)w * h * 16);
                for (auto &b : c) b = (uint8_t)rng();
                uint64_t out[VDF_HASH_WORDS];
                const int rc = vdf_hash_queue_mixed_submit(q, c.data(), w, h, out);
                if (big) {
                    if (rc != VDF_E_INVAL) wrong++;
                    refused++;
                    continue;
                }
                if (rc != VDF_OK) { wrong++; return; }
                accepted++;
                const uint64_t want = checksum(c.data(), c.size());
                for (int i = 0; i < VDF_HASH_WORDS; i++) if (out[i] != want + (uint64_t)i) wrong++;
                if (rng() % 7 == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 300));
            }
        });
    for (auto &x : th) x.join();
    uint64_t nb = 0, nc = 0;
    vdf_hash_queue_mixed_stats(q, &nb, &nc);
    uint32_t infl = 0;
    vdf_hash_queue_mixed_in_flight_max(q, &infl);
    const uint32_t n_slots = slots ? slots : 2u;
    bool ok = wrong == 0 && g_bad_batches == 0 && nc == accepted.load() && nc == (uint64_t)threads * per_thread - (uint64_t)refused.load() && infl <= n_slots &&
              (uint32_t)g_concurrent_max.load() <= n_slots && nb == (uint64_t)g_calls.exchange(0);
    if (expect_byte_cuts) ok = ok && g_batches_closed_by_bytes.load() > 0;
    if (oversize) ok = ok && refused.load() > 0;
    std::printf("threads %d staging %zu max_batch %u wait %u us slots %u: %llu clips in %llu batches (%d short of max_batch), %d refused, at most %u in flight, %d wrong%s\n",
                threads, staging, max_batch, wait_us, n_slots, (unsigned long long)nc, (unsigned long long)nb, g_batches_closed_by_bytes.load(), refused.load(), infl,
                wrong.load(), ok ? "" : "  <-- FAILED");
    vdf_hash_queue_mixed_destroy(q);
    vdf_ctx_destroy(ctx);
    return ok ? 0 : 1;
}

int main()
{
    int bad = 0;
    bad += run(48, 1 << 20, 4, 200, 60, 0, false, false);    // 48 callers, five clip sizes, batches of 4: most sleep for a free slot
    bad += run(48, 20000, 64, 100000, 40, 0, false, true);   // a byte budget (one 15 KB clip and a few small ones) closes batches long before count or deadline
    bad += run(16, 1 << 20, 64, 300, 80, 4, false, false);   // batches that never fill: every leader runs into its deadline
    bad += run(33, 1 << 16, 8, 2000, 50, 3, true, false);    // an oversize clip refused while others are in flight
    bad += run(1, 15360, 16, 50, 30, 1, false, false);       // a single caller, staging of exactly the largest clip
    // arguments
    vdf_ctx *ctx = nullptr;
    vdf_ctx_create(0, &ctx);
    vdf_hash_queue_mixed *q = nullptr;
    uint64_t out[VDF_HASH_WORDS];
    uint8_t px[16] = {0};
    bad += vdf_hash_queue_create_mixed(ctx, 0, 4, 0, 0, &q) != VDF_E_INVAL;
    bad += vdf_hash_queue_create_mixed(ctx, 4096, 0, 0, 0, &q) != VDF_E_INVAL;
    bad += vdf_hash_queue_create_mixed(ctx, 4096, 4, 0, 17, &q) != VDF_E_INVAL;
    bad += vdf_hash_queue_create_mixed(ctx, 16, 4, 0, 1, &q) != VDF_OK;
    bad += vdf_hash_queue_mixed_submit(q, px, 0, 1, out) != VDF_E_INVAL;
    bad += vdf_hash_queue_mixed_submit(q, px, 1, 2, out) != VDF_E_INVAL;  // 32 bytes into 16
    g_limit_bytes = 16; g_limit_clips = 4;
    bad += vdf_hash_queue_mixed_submit(q, px, 1, 1, out) != VDF_OK;
    vdf_hash_queue_mixed_destroy(q);
    vdf_ctx_destroy(ctx);
    std::puts(bad ? "queue mixed tsan FAILED" : "queue mixed tsan ok");
    return bad ? 1 : 0;
}
