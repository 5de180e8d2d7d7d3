// The batching queue (hash_queue.cpp) for clips of ANY frame size: one queue serves a whole library, whatever resolutions its files have.
//
// The protocol is hash_queue.cpp's - slots per GPU with a private context each, COLLECTING -> RUNNING -> DRAINING, one mutex, arrivals on
// cv_free, a slot's leader on cv_leader, its joiners on cv_done, the copies outside the lock - with two differences:
//   * a slot is full when max_batch clips OR staging_bytes of pinned memory are reached: a clip that does not fit what is left of the
//     collecting slot closes that batch (its leader need not wait for its deadline) and moves on to the next slot that collects;
//   * a clip of more than staging_bytes is refused (VDF_E_INVAL) without touching a slot.
// The leader hashes its batch with ONE vdf_hash_clips_u8 call on the slot's context: the clips sit in the slot's staging one after the
// other, each on a 64-byte boundary.  The slots per GPU are a parameter of the create call; this file reads no environment variable.
// A letterbox queue (vdf_hash_queue_create_mixed_letterbox) hashes its batches with vdf_hash_clips_u8_letterbox instead and hands every
// caller its clip's box as well.
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include <hip/hip_runtime.h>

#include "vdf_ctx.h"

// Weak: only a letterbox queue reaches it, so a program that never makes one (the plain queue's stand-alone test) links without a definition.
extern "C" int vdf_hash_clips_u8_letterbox(vdf_ctx *ctx, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips, uint32_t frames_per_clip,
                                           uint64_t *out_hashes, uint32_t *out_crops, uint32_t *out_dontcare) __attribute__((weak));

namespace {

#ifdef VDF_QUEUE_SYSTEM_CLOCK  // (ThreadSanitizer builds: see hash_queue.cpp)
using QueueClock = std::chrono::system_clock;
#else
using QueueClock = std::chrono::steady_clock;
#endif

struct Slot {
    vdf_ctx *ctx = nullptr;      // private context of this slot
    uint8_t *staging = nullptr;  // pinned host memory, staging_bytes
    bool pinned = false;
    std::vector<uint64_t> hashes;
    std::vector<uint32_t> crops;  // a letterbox queue: the batch's boxes
    std::vector<vdf_clip> clips;
    enum { COLLECTING, RUNNING, DRAINING } state = COLLECTING;
    uint32_t count = 0, ready = 0, remaining = 0;
    size_t used = 0;  // bytes of staging the joined clips take
    bool closed = false;  // an arrival did not fit: the leader closes the batch without waiting for its deadline
    uint64_t gen = 0, done_gen = ~0ull;
    int batch_rc = VDF_OK;
    std::condition_variable cv_leader;  // the leader: the batch is full / every joined copy has finished
    std::condition_variable cv_done;    // the joiners: the batch's results are in
};

constexpr size_t kAlign = 64;
size_t aligned_clip_bytes(uint32_t w, uint32_t h) { return ((size_t)w * h * VDF_DCT_SIZE + kAlign - 1) & ~(kAlign - 1); }

}  // namespace

struct vdf_hash_queue_mixed {
    size_t staging_bytes = 0, largest_clip = 0;  // the slots' staging (a multiple of 64); the caller's limit as given
    uint32_t max_batch = 0, max_wait_us = 0;
    bool letterbox = false;
    std::vector<Slot> slots;
    size_t cur = 0;  // the slot new arrivals join
    std::mutex mu;
    std::condition_variable cv_free;  // arrivals: some slot collects again
    uint32_t waiting_free = 0;        // ... how many sleep there
    uint64_t n_batches = 0, n_clips = 0;
    uint32_t in_flight = 0, in_flight_max = 0;
};

extern "C" {

void vdf_hash_queue_mixed_destroy(vdf_hash_queue_mixed *q)
{
    if (!q) return;
    for (Slot &s : q->slots) {
        if (s.staging) { if (s.pinned) (void)hipHostFree(s.staging); else std::free(s.staging); }
        if (s.ctx) vdf_ctx_destroy(s.ctx);
    }
    delete q;
}

static int create_queue(vdf_ctx *ctx, size_t staging_bytes, uint32_t max_batch, uint32_t max_wait_us, uint32_t slots_per_gpu, bool letterbox,
                        vdf_hash_queue_mixed **out)
{
    if (!ctx || !out || staging_bytes == 0 || max_batch == 0 || slots_per_gpu > 16) return VDF_E_INVAL;
    *out = nullptr;
    if (letterbox && !vdf_hash_clips_u8_letterbox) return VDF_E_INVAL;  // (a program linked without the letterbox call)
    vdf_hash_queue_mixed *q = new (std::nothrow) vdf_hash_queue_mixed();
    if (!q) return VDF_E_OOM;
    q->letterbox = letterbox;
    q->staging_bytes = (staging_bytes + kAlign - 1) & ~(kAlign - 1);
    q->largest_clip = staging_bytes;
    q->max_batch = max_batch; q->max_wait_us = max_wait_us;
    const int n_dev = vdf_ctx_device_count(ctx);
    const int per_gpu = slots_per_gpu ? (int)slots_per_gpu : 2;
    q->slots = std::vector<Slot>((size_t)(per_gpu * n_dev));
    vdf_impl::DeviceGuard restore_device;  // the loop below visits every device of the context on the caller's thread
    for (size_t k = 0; k < q->slots.size(); k++) {
        Slot &s = q->slots[k];
        const int dev = vdf_ctx_device_at(ctx, (int)(k % (size_t)n_dev));
        int rc = vdf_ctx_create(dev, &s.ctx);
        if (rc) { vdf_hash_queue_mixed_destroy(q); return rc; }
        s.ctx->one_stream = true;  // one stream per slot (vdf_ctx.h)
        (void)hipSetDevice(dev);
        if (hipHostMalloc((void **)&s.staging, q->staging_bytes, hipHostMallocDefault) == hipSuccess) {
            s.pinned = true;
        } else {
            (void)hipGetLastError();
            s.staging = (uint8_t *)std::malloc(q->staging_bytes);
            if (!s.staging) { vdf_hash_queue_mixed_destroy(q); return VDF_E_OOM; }
        }
        s.hashes.resize((size_t)max_batch * VDF_HASH_WORDS);
        s.clips.resize(max_batch);
        if (letterbox) s.crops.resize((size_t)max_batch * 4);
    }
    *out = q;
    return VDF_OK;
}

int vdf_hash_queue_create_mixed(vdf_ctx *ctx, size_t staging_bytes, uint32_t max_batch, uint32_t max_wait_us, uint32_t slots_per_gpu,
                                vdf_hash_queue_mixed **out)
{
    return create_queue(ctx, staging_bytes, max_batch, max_wait_us, slots_per_gpu, false, out);
}

int vdf_hash_queue_create_mixed_letterbox(vdf_ctx *ctx, size_t staging_bytes, uint32_t max_batch, uint32_t max_wait_us, uint32_t slots_per_gpu,
                                          vdf_hash_queue_mixed **out)
{
    return create_queue(ctx, staging_bytes, max_batch, max_wait_us, slots_per_gpu, true, out);
}

// frames: 16 gray frames of w x h, tightly packed.  Blocks until hashed.  out_crop (nullable): the clip's box, zeros from a plain queue.
int vdf_hash_queue_mixed_submit_crop(vdf_hash_queue_mixed *q, const uint8_t *frames, uint32_t w, uint32_t h, uint64_t *out_hash, uint32_t *out_crop)
{
    if (!q || !frames || !out_hash || w == 0 || h == 0) return VDF_E_INVAL;
    const size_t clip_bytes = (size_t)w * h * VDF_DCT_SIZE, need = aligned_clip_bytes(w, h);
    if (clip_bytes > q->largest_clip) return VDF_E_INVAL;  // no slot could ever take it
    std::unique_lock<std::mutex> lk(q->mu);
    // join the collecting slot; one that has no room for this clip closes (its batch goes as it is) and the next collecting slot takes over
    auto collecting = [&]() -> Slot * {
        for (size_t i = 0; i < q->slots.size(); i++) {
            const size_t k = (q->cur + i) % q->slots.size();
            Slot &c = q->slots[k];
            if (c.state != Slot::COLLECTING || c.closed || c.count >= q->max_batch) continue;
            if (c.used + need > q->staging_bytes) {  // (count > 0: an empty slot takes any clip that passed the check above)
                c.closed = true;
                c.cv_leader.notify_one();
                continue;
            }
            q->cur = k;
            return &c;
        }
        return nullptr;
    };
    Slot *sp = collecting();
    while (!sp) {
        q->waiting_free++;
        q->cv_free.wait(lk);
        q->waiting_free--;
        sp = collecting();
    }
    Slot &s = *sp;
    const uint32_t my = s.count++;
    const size_t my_at = s.used;
    s.used += need;
    s.clips[my] = vdf_clip{(uint64_t)my_at, (uint64_t)w * h, w, h, 0, 0, 0, 0};
    const uint64_t my_gen = s.gen;
    const auto deadline = QueueClock::now() + std::chrono::microseconds(q->max_wait_us);
    if (my != 0 && s.count == q->max_batch) s.cv_leader.notify_one();  // this join fills the batch
    lk.unlock();
    std::memcpy(s.staging + my_at, frames, clip_bytes);  // outside the lock: callers copy in parallel
    lk.lock();
    s.ready++;
    if (my == 0) {
        // leader: give others until the deadline (counted from the first arrival), until the batch is full or until a clip did not fit
        while (s.count < q->max_batch && !s.closed && s.cv_leader.wait_until(lk, deadline) != std::cv_status::timeout) {}
        s.state = Slot::RUNNING;                         // no more joins here; arrivals move on to the next slot
        while (s.ready < s.count) s.cv_leader.wait(lk);  // every joined caller has finished its copy
        const uint32_t n = s.count;
        const size_t used = s.used;
        q->in_flight++;
        if (q->in_flight > q->in_flight_max) q->in_flight_max = q->in_flight;
        lk.unlock();
        const int rc = q->letterbox ? vdf_hash_clips_u8_letterbox(s.ctx, s.staging, used, s.clips.data(), n, VDF_DCT_SIZE, s.hashes.data(), s.crops.data(), nullptr)
                                    : vdf_hash_clips_u8(s.ctx, s.staging, used, s.clips.data(), n, VDF_DCT_SIZE, s.hashes.data(), nullptr);
        lk.lock();
        q->in_flight--;
        s.batch_rc = rc;
        s.done_gen = my_gen;
        s.remaining = n;
        s.state = Slot::DRAINING;
        q->n_batches++;
        q->n_clips += n;
        s.cv_done.notify_all();
    } else {
        if (s.state == Slot::RUNNING && s.ready == s.count) s.cv_leader.notify_one();  // the closed batch was waiting for this copy
        while (!(s.done_gen == my_gen && s.state == Slot::DRAINING)) s.cv_done.wait(lk);
    }
    const int rc = s.batch_rc;
    if (rc == VDF_OK) std::memcpy(out_hash, s.hashes.data() + (size_t)my * VDF_HASH_WORDS, VDF_HASH_WORDS * 8);
    if (rc == VDF_OK && out_crop) {
        if (q->letterbox) std::memcpy(out_crop, s.crops.data() + (size_t)my * 4, 16);
        else std::memset(out_crop, 0, 16);
    }
    if (--s.remaining == 0) {  // last one out reopens the slot
        s.count = 0;
        s.ready = 0;
        s.used = 0;
        s.closed = false;
        s.gen++;
        s.state = Slot::COLLECTING;
        const uint32_t wake = q->waiting_free < q->max_batch ? q->waiting_free : q->max_batch;
        if (wake >= q->waiting_free) q->cv_free.notify_all();
        else
            for (uint32_t i = 0; i < wake; i++) q->cv_free.notify_one();
    }
    return rc;
}

int vdf_hash_queue_mixed_submit(vdf_hash_queue_mixed *q, const uint8_t *frames, uint32_t w, uint32_t h, uint64_t *out_hash)
{
    return vdf_hash_queue_mixed_submit_crop(q, frames, w, h, out_hash, nullptr);
}

int vdf_hash_queue_mixed_stats(vdf_hash_queue_mixed *q, uint64_t *n_batches, uint64_t *n_clips)
{
    if (!q) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(q->mu);
    if (n_batches) *n_batches = q->n_batches;
    if (n_clips) *n_clips = q->n_clips;
    return VDF_OK;
}

int vdf_hash_queue_mixed_in_flight_max(vdf_hash_queue_mixed *q, uint32_t *out)
{
    if (!q || !out) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(q->mu);
    *out = q->in_flight_max;
    return VDF_OK;
}

}  // extern "C"
