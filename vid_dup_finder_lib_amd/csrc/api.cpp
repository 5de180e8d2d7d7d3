// C-ABI layer (include/vdf.h): context, device scratch, launch orchestration, the hit-buffer
// overflow protocol and the host-level convenience calls.  Compiled with hipcc; the kernels live
// in hamming.hip and dct_hash.hip.  There is deliberately NO CPU fallback for the compute path:
// without a usable GPU every compute entry point fails with VDF_E_HIP.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>

#include "align_seed_rates_plan.h"
#include "host_sort.h"
#include "vdf_ctx.h"
#include "window_class_layout.h"

namespace {
thread_local std::string g_create_error;
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}

vdf_ctx::~vdf_ctx()
{
    if (!subs.empty() || !workers.empty()) vdf_impl::destroy_multi(this);
    if (copy_pool) vdf_impl::destroy_copy_pool(this);
    for (auto &kv : axis_tables) {
        kv.second->start.release(); kv.second->size.release(); kv.second->w.release();
        delete kv.second;
    }
    for (auto &kv : mfma_tables) {
        kv.second->operand.release(); kv.second->bias.release(); kv.second->meta.release();
        delete kv.second;
    }
    for (auto &kv : box_tables) {
        kv.second->blob.release(); kv.second->entries.release();
        delete kv.second;
    }
    DevBuf *all[] = {&row_lo, &row_hi, &tile_lo, &tile_hi, &tile_first, &tile_count, &tile_offset, &counters,
                     &hits, &perm, &matched, &exp_cols, &exp_rows, &pop_cols, &pop_rows, &cand, &group_cmin, &group_offset, &group_blocks, &up_hashes,
                     &up_dur, &up_ref_hashes, &up_ref_dur, &small, &frames, &frames2, &out_hashes, &out_hashes2, &out_dc,
                     &out_dc2, &cos_table, &crops, &crop_desc, &crop_tables, &crop_desc2, &crop_tables2, &crop_work, &sort_scratch, &sort_scratch_pub, &hits2, &hit_bitmaps, &bitmap_gather,
                     &out_zero, &out_zero2, &up_zero, &variant_hashes, &align_plan, &align_scratch, &align_up, &seed_bitmap, &seed_plan, &seed_out, &seed_classes};
    for (DevBuf *b : all) b->release();
    for (PinBuf &b : pin) b.release();
    for (PinBuf &b : pin_out) b.release();
    pin_small.release();
    pin_ctrl.release();
    pin_crops.release();
    pin_desc.release();
    host_hits.buf.release();
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (ev_mid) (void)hipEventDestroy(ev_mid);
    if (ev_wait) (void)hipEventDestroy(ev_wait);
    for (hipEvent_t e : ev_copy) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_done) if (e) (void)hipEventDestroy(e);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    if (stream) (void)hipStreamDestroy(stream);
}

namespace vdf_impl {

void set_create_error(const std::string &msg) { g_create_error = msg; }

int fail(vdf_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

int fail_hip(vdf_ctx *ctx, hipError_t e, const char *what)
{
    std::string msg = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return fail(ctx, e == hipErrorOutOfMemory ? VDF_E_OOM : VDF_E_HIP, msg);
}

bool is_sorted_u32(const uint32_t *d, size_t n)
{
    for (size_t i = 1; i < n; i++)
        if (d[i] < d[i - 1]) return false;
    return true;
}

// Shared core of both searches: windows + tiles, distance kernel, hit download (sorted by (row, col)).
constexpr size_t kPinSmallBytes = 4u << 20;
constexpr uint64_t kDeviceSortHits = 1u << 17;
constexpr uint32_t kRefsMinWorkgroups = 2048;  // a reference search with fewer (tile, chunk) workgroups than this narrows its chunks
constexpr uint64_t kSpecSortHits = 1u << 14;    // hit lists expected to be at least this long are sorted on the device speculatively
constexpr uint64_t kFilterHits = 1u << 16;      // from this many hits on, a replay-only launch drops the rows that cannot become targets  // hit lists from this length on are sorted on the device

int search_core(vdf_ctx *ctx, int mode, const uint64_t *d_col_hashes, const uint32_t *d_col_dur, size_t n_cols,
                const uint64_t *d_row_hashes, const uint32_t *d_row_dur, const uint32_t *d_row_perm, size_t n_rows,
                uint32_t tol_int, uint32_t shard_index, uint32_t shard_count, uint32_t row_begin, uint32_t row_end,
                const uint32_t *d_matched, uint32_t row_index_base, vdf_hit *hits, uint64_t capacity,
                uint64_t *n_hits_out, uint32_t *overflow_row_out, hipStream_t stream, bool replay_only, vdf_ctx::HostHits *staging,
                ShardExchange *fx)
{
    *n_hits_out = 0;
    *overflow_row_out = 0xFFFFFFFFu;
    if (n_rows == 0 || n_cols == 0) return VDF_OK;
    if (n_rows >= 0xFFFFFFFFull || n_cols >= 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "more than 2^32-1 hashes");
    if (shard_count == 0 || shard_index >= shard_count) return fail(ctx, VDF_E_INVAL, "bad shard index/count");
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    const double t_enter = now_ms();

    vdf::SearchLaunch L{};
    const bool mfma = ctx->search_backend == 1;
    // MFMA kernel: 512-row workgroups for search(); reference searches may take 256-row ones (a tile's candidate range is the
    // union of its rows' duration windows: fewer rows, narrower union)
    L.tile_rows = mfma ? (mode == 1 ? ctx->mfma_refs_rows : ctx->mfma_self_rows) : ctx->tile_rows;
    L.chunk_cols = mfma ? ctx->mfma_chunk_cols : ctx->chunk_cols;
    L.n_row_tiles = (uint32_t)((n_rows + L.tile_rows - 1) / L.tile_rows);
    if (mfma && L.chunk_cols == 0) {
        // Long chunks amortise a workgroup's target loads (65536 columns measured best at 1 M hashes), but a small search
        // must still be cut into enough workgroups to fill and balance 256 CUs: halve (down to 4096) until there are >= 8192 of them
        // (swept at 10 k .. 1 M hashes, tools/sweep_sizes.py).
        L.chunk_cols = 65536;
        while (L.chunk_cols > 4096 && (uint64_t)L.n_row_tiles * ((n_cols + L.chunk_cols - 1) / L.chunk_cols) < ctx->mfma_min_wgs) L.chunk_cols /= 2;
    }
    // (row tile, chunk) workgroups are numbered with 32 bits: widen the chunks rather than refuse very large inputs
    while ((uint64_t)L.n_row_tiles * ((n_cols + L.chunk_cols - 1) / L.chunk_cols) >= 0x40000000ull && L.chunk_cols < (1u << 22))
        L.chunk_cols *= 2;
    const size_t padded_rows = (size_t)L.n_row_tiles * L.tile_rows;
    VDF_HIP(ctx, ctx->row_lo.reserve(padded_rows * 4));
    VDF_HIP(ctx, ctx->row_hi.reserve(padded_rows * 4));
    VDF_HIP(ctx, ctx->tile_lo.reserve((size_t)L.n_row_tiles * 4));
    VDF_HIP(ctx, ctx->tile_hi.reserve((size_t)L.n_row_tiles * 4));
    VDF_HIP(ctx, ctx->tile_first.reserve((size_t)L.n_row_tiles * 4));
    VDF_HIP(ctx, ctx->tile_count.reserve((size_t)L.n_row_tiles * 4));
    VDF_HIP(ctx, ctx->tile_offset.reserve(((size_t)L.n_row_tiles + 1) * 4));
    VDF_HIP(ctx, ctx->counters.reserve(64));
    const uint64_t dev_cap = std::max<uint64_t>(capacity, 1);
    VDF_HIP(ctx, ctx->hits.reserve(dev_cap * sizeof(vdf_hit)));

    L.row_hashes = reinterpret_cast<const uint32_t *>(d_row_hashes);
    L.row_perm = d_row_perm;
    L.n_rows = (uint32_t)n_rows;
    L.row_index_base = row_index_base;
    L.col_hashes = reinterpret_cast<const uint32_t *>(d_col_hashes);
    L.n_cols = (uint32_t)n_cols;
    L.row_lo = ctx->row_lo.as<uint32_t>();
    L.row_hi = ctx->row_hi.as<uint32_t>();
    L.tile_lo = ctx->tile_lo.as<uint32_t>();
    L.tile_hi = ctx->tile_hi.as<uint32_t>();
    L.tile_first = ctx->tile_first.as<uint32_t>();
    L.tile_count = ctx->tile_count.as<uint32_t>();
    L.tile_offset = ctx->tile_offset.as<uint32_t>();
    L.tol = tol_int;
    L.matched = d_matched;
    L.self_mode = (mode == 0);
    L.shard_index = shard_index;
    L.shard_count = shard_count;
    L.hits = ctx->hits.as<vdf_hit>();
    L.capacity = capacity;
    L.counters = ctx->counters.as<unsigned long long>();
    L.overflow_row = reinterpret_cast<uint32_t *>(ctx->counters.as<unsigned long long>() + 4);

    // Early-exit step (both backends): the first 64-bit k-step after which unrelated hashes (partial distance bits / 2 +-
    // sqrt(bits) / 2) are, 4 sigma down, still more than tol apart - then nearly every block stops there.  Exact whatever is
    // picked.  Kernels are instantiated for steps 6, 8, 10, 11, 12, 13, 14 (MFMA) / 6, 10, 12 (VALU): round up; 16 = no test.
    // (tolerance 350 -> step 12 = 832 bits; up to 387 -> 13; up to 417 -> 14 = 960 bits; beyond that unrelated hashes are no longer
    // 4 sigma away from the tolerance after any prefix and the stream runs all 16 steps)
    L.prune_step = 16;
    if (ctx->mfma_prune_step >= 0) {
        L.prune_step = ctx->mfma_prune_step;
    } else {
        for (int st = 6; st <= 14; st++) {
            const double bits = 64.0 * (st + 1);
            if (bits / 2 - 2.0 * std::sqrt(bits) >= (double)tol_int + 1) { L.prune_step = st; break; }
        }
    }
    if (mfma) L.prune_step = L.prune_step <= 6 ? 6 : L.prune_step <= 8 ? 8 : L.prune_step <= 10 ? 10 : L.prune_step <= 14 ? L.prune_step : 16;
    else L.prune_step = L.prune_step <= 6 ? 6 : L.prune_step <= 10 ? 10 : L.prune_step <= 12 ? 12 : 16;
    if (mfma) {
        L.group_size = std::min<uint32_t>(ctx->mfma_group, L.n_row_tiles);
        L.n_groups = (L.n_row_tiles + L.group_size - 1) / L.group_size;
        if (L.n_groups > 1024) return fail(ctx, VDF_E_INVAL, "too many row-tile groups");
        VDF_HIP(ctx, ctx->group_cmin.reserve((size_t)L.n_groups * 4));
        VDF_HIP(ctx, ctx->group_offset.reserve(((size_t)L.n_groups + 1) * 4));
        VDF_HIP(ctx, ctx->group_blocks.reserve((size_t)L.n_groups * 4));
        L.group_blocks = ctx->group_blocks.as<uint32_t>();
        L.group_cmin = ctx->group_cmin.as<uint32_t>();
        L.group_offset = ctx->group_offset.as<uint32_t>();
        // expand both operands to {0, 1} fp4 nibbles (512 B per hash) plus popcount arrays; rows share the column copy in self mode
        const uint32_t k_steps = (uint32_t)(L.prune_step < 15 ? L.prune_step + 1 : 16);  // k-steps of the tested prefix
        const uint32_t col_pad = (uint32_t)((n_cols + vdf::kMfmaRowPad - 1) / vdf::kMfmaRowPad * vdf::kMfmaRowPad) + vdf::kMfmaColPad;
        VDF_HIP(ctx, ctx->exp_cols.reserve((size_t)col_pad * 512));
        VDF_HIP(ctx, ctx->pop_cols.reserve((size_t)col_pad * 12));
        // A database the caller has pinned (vdf_ctx_pin_database: "these bytes will not change") keeps its expansion between
        // searches: 0.15 ms per million hashes that a reference search of 0.9 ms need not pay again.
        const ExpOwner want_owner{d_col_hashes, n_cols, k_steps, ctx->exp_cols.p};
        const bool reuse = ctx->pinned_db == d_col_hashes && ctx->pinned_n == n_cols && ctx->exp_owner == want_owner;
        if (!reuse) {
            ctx->exp_owner = ExpOwner{};
            VDF_HIP(ctx, vdf::launch_expand_fp4(L.col_hashes, (uint32_t)n_cols, col_pad, ctx->exp_cols.p, k_steps,
                                                ctx->pop_cols.as<float>(), stream));
            ctx->exp_owner = want_owner;
        }
        L.col_exp = ctx->exp_cols.p;
        L.col_pop3 = ctx->pop_cols.as<float>();
        L.col_pad = col_pad;
        if (d_row_hashes == d_col_hashes) {
            L.row_exp = ctx->exp_cols.p;
            L.row_pop3 = L.col_pop3;
            L.row_pad = col_pad;
        } else {
            const uint32_t row_pad = (uint32_t)((padded_rows + 127) / 128 * 128);
            VDF_HIP(ctx, ctx->exp_rows.reserve((size_t)row_pad * 512));
            VDF_HIP(ctx, ctx->pop_rows.reserve((size_t)row_pad * 12));
            VDF_HIP(ctx, vdf::launch_expand_fp4(L.row_hashes, (uint32_t)n_rows, row_pad, ctx->exp_rows.p, k_steps,
                                                ctx->pop_rows.as<float>(), stream));
            L.row_exp = ctx->exp_rows.p;
            L.row_pop3 = ctx->pop_rows.as<float>();
            L.row_pad = row_pad;
        }
    }
    // counters[0..2] = 0, overflow_row = UINT32_MAX
    const unsigned long long init[8] = {0, 0, 0, 0, 0xFFFFFFFFull, 0, 0, 0};
    // How much of the hit list is fetched together with the counters (one synchronisation instead of two): about what the
    // previous call produced.  From 16 k pairs on that head is also put into (row, col) order on the device BEFORE its
    // length is known: the slots are pre-filled with 0xFF (sorts last), so if the list fits the head the host receives it
    // sorted - the host radix sort of a 50 k-pair list cost 0.2 ms of a 1.5 ms reference search.
    const bool pin_ok = ctx->pin_small.reserve(kPinSmallBytes) && ctx->pin_small.pinned;
    uint64_t spec = std::min<uint64_t>(capacity, std::max<uint64_t>(ctx->hits_guess + ctx->hits_guess / 4 + 1024, 8192));
    if (!pin_ok || spec * sizeof(vdf_hit) > kPinSmallBytes) spec = 0;  // long lists go straight to the caller's buffer, once their length is known
    const bool spec_sort = spec && ctx->hits_guess >= kSpecSortHits;
    if (spec_sort) VDF_HIP(ctx, hipMemsetAsync(ctx->hits.p, 0xFF, (size_t)spec * sizeof(vdf_hit), stream));
    // A reference search's workgroups are (256-row tile, chunk of its rows' united +-5 % windows): how many there are is only known
    // once the windows are.  With the chunk width picked for a full rectangle the BASELINE configs[4] shape ends up with ~600
    // workgroups of very different lengths for 512 resident slots (kernel 0.88 ms); 8192-column chunks give ~2500 and 0.73 ms
    // (gpurun_out/r03m).  So: if the first pass yields too few, the chunks are halved until there would be enough and the windows /
    // tile kernels run once more (60 us); the width is remembered for the next search of the same shape.  search() keeps its long
    // chunks: its 512-row workgroups pay 208 KB of target loads each, and narrower chunks measured slower at every width.
    const bool adapt_refs = mode == 1 && mfma && ctx->mfma_chunk_cols == 0;
    if (adapt_refs && ctx->refs_hint_cols == n_cols && ctx->refs_hint_rows == n_rows && ctx->refs_hint_chunk) L.chunk_cols = ctx->refs_hint_chunk;
    if (!ctx->pin_ctrl.reserve(256)) return fail(ctx, VDF_E_OOM, "pinned staging");
    unsigned long long *pre = ctx->pin_ctrl.as<unsigned long long>() + 8;
    uint32_t total_tiles = 0;
    unsigned long long unsorted = 0, admitted = 0;
    for (int pass = 0;; pass++) {
        VDF_HIP(ctx, hipMemcpyAsync(ctx->counters.p, init, sizeof init, hipMemcpyHostToDevice, stream));
        VDF_HIP(ctx, vdf::launch_windows_tiles(mode, d_col_dur, (uint32_t)n_cols, d_row_dur, d_row_perm, (uint32_t)n_rows,
                                               row_begin, row_end, shard_index, shard_count, L, stream));
        // workgroup count, sortedness flag and admitted pairs come back through pinned memory (a pageable destination would
        // make each of the copies a blocking round trip of its own)
        VDF_HIP(ctx, hipMemcpyAsync(pre, L.counters, 64, hipMemcpyDeviceToHost, stream));
        VDF_HIP(ctx, hipMemcpyAsync(pre + 8, mfma ? L.group_offset + L.n_groups : L.tile_offset + L.n_row_tiles, 4,
                                    hipMemcpyDeviceToHost, stream));
        // (the grouped grid of the matrix-core backend counts every (tile, chunk) of a group's rectangle; the workgroups that
        // have work are the sum of the tiles' own chunk counts)
        VDF_HIP(ctx, hipMemcpyAsync(pre + 9, L.tile_offset + L.n_row_tiles, 4, hipMemcpyDeviceToHost, stream));
        VDF_HIP(ctx, hipStreamSynchronize(stream));
        total_tiles = *reinterpret_cast<const uint32_t *>(pre + 8);
        const uint32_t busy_tiles = *reinterpret_cast<const uint32_t *>(pre + 9);
        unsorted = pre[5];
        admitted = pre[2];
        if (!adapt_refs || pass > 0 || unsorted || busy_tiles == 0 || busy_tiles >= kRefsMinWorkgroups || L.chunk_cols <= 4096) break;
        uint64_t est = busy_tiles;
        while (L.chunk_cols > 4096 && est < kRefsMinWorkgroups) { L.chunk_cols /= 2; est *= 2; }
    }
    if (adapt_refs) { ctx->refs_hint_cols = n_cols; ctx->refs_hint_rows = n_rows; ctx->refs_hint_chunk = L.chunk_cols; }
    // the windows are binary searches over the candidate durations (search_algorithm.rs:93-117,173-185 rely on Search::sort)
    if (unsorted) return fail(ctx, VDF_E_INVAL, "durations are not ascending: pass the arrays in Search::sort order");
    if (total_tiles >= 0x7FFFFFFFu) return fail(ctx, VDF_E_INVAL, "tile count exceeds the grid limit");
    if (mfma) {
        // Queue of suspect pairs the stream cannot rule out (16-byte entries).  Unrelated hashes put ~2.3e-6 of the admitted
        // pairs there at the 4-sigma test point; slots are handed out in chunks of 8 per wave, so every wave may strand
        // a few.  Sized generously from the admitted pairs; if it still overflows, the hit-buffer overflow protocol takes
        // over (rows below the smallest row that lost a suspect are complete).
        const uint64_t want = ((uint64_t)((double)admitted * 6e-6) + (uint64_t)total_tiles * 8 * 8 + std::max<uint64_t>(capacity, 1ull << 20)) * ctx->cand_scale;
        L.cand_capacity = (uint32_t)std::min<uint64_t>(want, 0x40000000ull);
        if (ctx->cand_capacity_override)  // VDF_CAND_CAPACITY (tests: forces the overflow path)
            L.cand_capacity = (uint32_t)std::min<uint64_t>((uint64_t)ctx->cand_capacity_override * ctx->cand_scale, 0x40000000ull);
        // (a buffer that grows is freed and allocated again, and the allocator may hand the old address back: the capacity tells, the pointer does not)
        const size_t cap_before = ctx->cand.cap;
        VDF_HIP(ctx, ctx->cand.reserve((size_t)L.cand_capacity * 16));
        if (ctx->cand.cap != cap_before) ctx->cand_dirty = SIZE_MAX;  // fresh allocation: fill all of it
        // Only the slots earlier launches may have touched need the empty pattern (0xFF) again - ALL of them, whatever this
        // launch's capacity is: a launch with a smaller queue (after an overflow retry's x4, or a smaller search) must not
        // leave the slots beyond its own capacity stale for a later, larger launch to read as suspects.
        const size_t slots = ctx->cand.cap / 16;
        const size_t fill = (ctx->cand_dirty == SIZE_MAX ? slots : std::min<size_t>(slots, ctx->cand_dirty)) * 16;
        if (fill) VDF_HIP(ctx, hipMemsetAsync(ctx->cand.p, 0xFF, fill, stream));
        ctx->cand_dirty = L.cand_capacity;  // until the launch reports how far it got (an error return below keeps this bound)
        L.cand = ctx->cand.p;
        L.cand_head = ctx->counters.as<unsigned long long>() + 6;
    }

    ctx->timing.prep_ms += (float)(now_ms() - t_enter);
    VDF_HIP(ctx, hipEventRecord(ctx->ev0, stream));
    if (mfma) {
        VDF_HIP(ctx, vdf::launch_hamming_tiles_mfma2(L, total_tiles, stream));
        VDF_HIP(ctx, hipEventRecord(ctx->ev_mid, stream));
        if (total_tiles) VDF_HIP(ctx, vdf::launch_resolve_candidates(L, stream));
    } else {
        VDF_HIP(ctx, vdf::launch_hamming_tiles(L, total_tiles, stream));
        VDF_HIP(ctx, hipEventRecord(ctx->ev_mid, stream));
    }
    VDF_HIP(ctx, hipEventRecord(ctx->ev1, stream));
    // Counters and - speculatively - the head of the hit list come back behind ONE synchronisation: the list is usually
    // about as long as the previous call's, and a second round trip costs more than copying a few KB too many.
    if (!ctx->pin_ctrl.reserve(256)) return fail(ctx, VDF_E_OOM, "pinned staging");
    unsigned long long *fin = ctx->pin_ctrl.as<unsigned long long>();
    VDF_HIP(ctx, hipMemcpyAsync(fin, ctx->counters.p, 64, hipMemcpyDeviceToHost, stream));
    unsigned row_bits = 1;
    while (row_bits < 32 && ((uint64_t)row_index_base + n_rows) >> row_bits) row_bits++;
    unsigned col_bits = 1;  // columns are candidate indices below n_cols: the hit sort skips the bytes above them
    while (col_bits < 32 && ((uint64_t)n_cols >> col_bits)) col_bits++;
    if (spec_sort) {
        VDF_HIP(ctx, ctx->sort_scratch.reserve(vdf::sort_hits_scratch_bytes((size_t)spec)));
        VDF_HIP(ctx, vdf::launch_sort_hits(ctx->hits.as<vdf_hit>(), (size_t)spec, row_bits, ctx->sort_scratch.p, ctx->sort_scratch.cap, stream, col_bits));
    }
    if (spec) VDF_HIP(ctx, hipMemcpyAsync(ctx->pin_small.p, ctx->hits.p, (size_t)spec * sizeof(vdf_hit), hipMemcpyDeviceToHost, stream));
    VDF_HIP(ctx, hipStreamSynchronize(stream));
    const double t_synced = now_ms();
    float ms = 0.f, ms_stream = 0.f;
    VDF_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    VDF_HIP(ctx, hipEventElapsedTime(&ms_stream, ctx->ev0, ctx->ev_mid));
    ctx->timing.stream_ms += ms_stream;
    ctx->timing.resolve_ms += ms - ms_stream;
    if (mfma) { ctx->timing.suspects += fin[6]; ctx->timing.suspect_capacity = L.cand_capacity; }

    if (mfma) ctx->cand_dirty = (size_t)std::min<uint64_t>(fin[6], L.cand_capacity);  // slots this launch used
    const uint64_t produced = fin[0];
    uint64_t stored = std::min<uint64_t>(produced, capacity);
    ctx->hits_guess = stored;
    uint64_t n_out = produced;
    vdf_hit *d_list = ctx->hits.as<vdf_hit>();
    uint64_t have = std::min(stored, spec);
    // Dense near-duplicates: most of the thresholded pairs belong to rows the greedy replay never uses as targets
    // (hamming.hip: launch_filter_*).  With the COMPLETE hit set of the launch in hand they are dropped here, before the
    // sort, the download and the host replay - a cluster of s mutual duplicates sends down s - 1 pairs instead of
    // s (s - 1) / 2.  A sharded launch has the complete set spread over its shards: they agree that nobody overflowed, and OR
    // the two bitmaps (1 bit per entry: 125 KB per million) between the steps.  EVERY shard takes part, also one without hits.
    bool filter = false;
    if (replay_only && mode == 0 && !ctx->no_hit_filter) {
        bool complete = produced <= capacity && (uint32_t)fin[4] == 0xFFFFFFFFu;
        uint64_t total = produced;
        if (fx) {
            const int r = fx->agree(shard_index, ctx, &complete, &total);
            if (r) return r;
        } else if (shard_count != 1) {
            complete = false;
        }
        filter = complete && total >= kFilterHits;
    }
    if (filter) {
        const size_t words = ((size_t)n_cols + 31) / 32;
        VDF_HIP(ctx, ctx->hits2.reserve((size_t)std::max<uint64_t>(stored, 1) * sizeof(vdf_hit)));
        VDF_HIP(ctx, ctx->hit_bitmaps.reserve(2 * words * 4 + 16));
        uint32_t *bm = ctx->hit_bitmaps.as<uint32_t>();
        VDF_HIP(ctx, vdf::launch_filter_mark_incoming(d_list, stored, (uint32_t)n_cols, bm, stream));
        // (an exchange that could not be carried out says so on every shard alike - kExchangeOff: the launch goes on unfiltered)
        if (fx) { const int r = fx->or_bitmap(shard_index, ctx, bm, words, stream); if (r < 0) return r; if (r == vdf_impl::kExchangeOff) filter = false; }
        if (filter) {
            VDF_HIP(ctx, vdf::launch_filter_mark_covered(d_list, stored, (uint32_t)n_cols, bm, stream));
            if (fx) { const int r = fx->or_bitmap(shard_index, ctx, bm + words, words, stream); if (r < 0) return r; if (r == vdf_impl::kExchangeOff) filter = false; }
        }
    }
    if (filter) {
        uint32_t *bm = ctx->hit_bitmaps.as<uint32_t>();
        VDF_HIP(ctx, vdf::launch_filter_compact(d_list, stored, (uint32_t)n_cols, bm, ctx->hits2.as<vdf_hit>(), L.counters + 7, stream));
        VDF_HIP(ctx, hipMemcpyAsync(fin + 7, L.counters + 7, 8, hipMemcpyDeviceToHost, stream));
        VDF_HIP(ctx, hipStreamSynchronize(stream));
        d_list = ctx->hits2.as<vdf_hit>();
        stored = fin[7];
        n_out = stored;
        have = 0;  // the speculative copy held unfiltered pairs
        ctx->timing.hits_filtered += produced - stored;
    }
    if (stored) {
        if (staging) {  // the library's own staging grows to the list (host-level calls)
            const size_t need = std::max<size_t>((size_t)stored, 1u << 16);
            if (staging->size() < need && !staging->resize(need + need / 4)) return fail(ctx, VDF_E_OOM, "hit staging");
            hits = staging->data();
        }
        if (have) std::memcpy(hits, ctx->pin_small.p, (size_t)have * sizeof(vdf_hit));
        if (stored > have) {
            // Long list: it is put into (row, col) order on the device before it comes down - a host radix sort of 1e7
            // pairs costs about as much as the search kernel.
            const bool dev_sort = stored >= (d_list == ctx->hits.as<vdf_hit>() ? kDeviceSortHits : kDeviceSortHits / 16);  // after the filter nothing of the list is on the host yet
            if (dev_sort) {
                VDF_HIP(ctx, ctx->sort_scratch.reserve(vdf::sort_hits_scratch_bytes((size_t)stored)));
                VDF_HIP(ctx, vdf::launch_sort_hits(d_list, (size_t)stored, row_bits, ctx->sort_scratch.p, ctx->sort_scratch.cap, stream, col_bits));
                VDF_HIP(ctx, hipMemcpyAsync(hits, d_list, (size_t)stored * sizeof(vdf_hit), hipMemcpyDeviceToHost, stream));
            } else {
                VDF_HIP(ctx, hipMemcpyAsync(hits + have, d_list + have, (size_t)(stored - have) * sizeof(vdf_hit), hipMemcpyDeviceToHost, stream));
            }
            VDF_HIP(ctx, hipStreamSynchronize(stream));
            if (!dev_sort) sort_hits(hits, (size_t)stored);
        } else if (!spec_sort) {
            sort_hits(hits, (size_t)stored);
        }
    }
    ctx->timing.download_ms += (float)(now_ms() - t_synced);
    *n_hits_out = n_out;
    *overflow_row_out = (uint32_t)fin[4];
    ctx->stats.pairs += fin[2];
    ctx->stats.pairs_computed += fin[1];
    ctx->stats.n_hits += produced;
    ctx->stats.n_tiles += total_tiles;
    ctx->stats.n_launches += 1;
    ctx->stats.kernel_ms += ms;
    ctx->stats.pairs_early_exit += fin[3];
    ctx->stats.early_exit_bits = L.prune_step < 15 ? 64u * (uint32_t)(L.prune_step + 1) : 0u;
    return VDF_OK;
}

int upload(vdf_ctx *ctx, DevBuf &buf, const void *src, size_t bytes, hipStream_t stream)
{
    VDF_HIP(ctx, buf.reserve(std::max<size_t>(bytes, 16)));
    if (bytes) VDF_HIP(ctx, hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, stream));
    return VDF_OK;
}

std::mutex &link_mutex(int device)
{
    static std::mutex m[64];
    return m[(unsigned)device % 64u];
}

int wait_event(vdf_ctx *ctx, hipEvent_t ev)
{
    if (!ctx->spin_wait) {
        const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(50);
        do {
            const hipError_t q = hipEventQuery(ev);
            if (q == hipSuccess) return VDF_OK;
            if (q != hipErrorNotReady) return fail_hip(ctx, q, "hipEventQuery");
        } while (std::chrono::steady_clock::now() < until);
    }
    VDF_HIP(ctx, hipEventSynchronize(ev));
    return VDF_OK;
}

DeviceAxisTable *axis_table(vdf_ctx *ctx, uint32_t in_size, hipStream_t stream, int *rc)
{
    auto it = ctx->axis_tables.find(in_size);
    if (it != ctx->axis_tables.end()) { *rc = VDF_OK; return it->second; }
    DeviceAxisTable *t = new DeviceAxisTable();
    if (!vdf::build_axis_table(in_size, VDF_DCT_SIZE, t->host)) {
        delete t;
        *rc = fail(ctx, VDF_E_BAD_DIMS, "cannot build resize table");
        return nullptr;
    }
    int r = upload(ctx, t->start, t->host.start.data(), t->host.start.size() * 4, stream);
    if (r == VDF_OK) r = upload(ctx, t->size, t->host.size.data(), t->host.size.size() * 4, stream);
    if (r == VDF_OK) r = upload(ctx, t->w, t->host.w.data(), t->host.w.size() * 2, stream);
    if (r == VDF_OK && hipStreamSynchronize(stream) != hipSuccess) r = fail(ctx, VDF_E_HIP, "table upload failed");
    if (r != VDF_OK) {
        t->start.release(); t->size.release(); t->w.release();
        delete t;
        *rc = r;
        return nullptr;
    }
    ctx->axis_tables[in_size] = t;
    *rc = VDF_OK;
    return t;
}

DeviceMfmaTable *mfma_table(vdf_ctx *ctx, uint32_t in_size, int layout, hipStream_t stream, int *rc)
{
    const uint64_t key = (uint64_t)in_size * 4 + (uint64_t)layout;
    auto it = ctx->mfma_tables.find(key);
    if (it != ctx->mfma_tables.end()) { *rc = VDF_OK; return it->second; }
    DeviceMfmaTable *t = new DeviceMfmaTable();
    if (!vdf::build_mfma_axis_table(in_size, layout, t->host)) {
        delete t;
        *rc = fail(ctx, VDF_E_BAD_DIMS, "cannot build resize table");
        return nullptr;
    }
    int r = VDF_OK;
    if (t->host.ok) {
        r = upload(ctx, t->operand, t->host.operand.data(), t->host.operand.size(), stream);
        if (r == VDF_OK) r = upload(ctx, t->bias, t->host.bias.data(), t->host.bias.size() * 4, stream);
        if (r == VDF_OK && !t->host.band_meta.empty())
            r = upload(ctx, t->meta, t->host.band_meta.data(), t->host.band_meta.size() * 4, stream);
        if (r == VDF_OK && hipStreamSynchronize(stream) != hipSuccess) r = fail(ctx, VDF_E_HIP, "table upload failed");
    }
    if (r != VDF_OK) {
        t->operand.release(); t->bias.release(); t->meta.release();
        delete t;
        *rc = r;
        return nullptr;
    }
    ctx->mfma_tables[key] = t;
    *rc = VDF_OK;
    return t;
}

// The tables of EVERY crop-box size of a w x h frame (vdf_ctx.h: BoxTableSet), built and uploaded once per context and frame size.
BoxTableSet *box_table_set(vdf_ctx *ctx, uint32_t w, uint32_t h, hipStream_t stream, int *rc)
{
    const uint64_t key = ((uint64_t)w << 32) | h;
    auto it = ctx->box_tables.find(key);
    if (it != ctx->box_tables.end()) { *rc = VDF_OK; return it->second; }
    BoxTableSet *set = new BoxTableSet();
    set->one_tile = w <= 64 && h <= 64;
    const size_t n_idx = (size_t)w + h + 2;
    std::vector<vdf::CropTableEntry> entries(n_idx, vdf::CropTableEntry{nullptr, nullptr, 0, 0});
    std::vector<size_t> offset(n_idx, 0);
    std::vector<uint8_t> blob;
    bool usable = true;
    for (size_t idx = 0; idx < n_idx && usable; idx++) {
        const bool vertical = idx > w;
        const uint32_t size = (uint32_t)(vertical ? idx - w - 1 : idx);
        offset[idx] = blob.size();
        if (size == 0) {  // no such box; the one-tile form keeps the stride
            if (set->one_tile) blob.resize(blob.size() + vdf::kSmallBoxTableStride, 0);
            continue;
        }
        vdf::MfmaAxisTable t;
        if (!vdf::build_mfma_axis_table(size, vertical ? vdf::kMfmaLayoutVertical : vdf::kMfmaLayoutHorizontal, t) || !t.ok) { usable = false; break; }
        const size_t at = blob.size();
        blob.resize(at + t.operand.size() + 128, 0);
        std::memcpy(blob.data() + at, t.operand.data(), t.operand.size());
        std::memcpy(blob.data() + at + t.operand.size(), t.bias.data(), 64);
        const int32_t tail[2] = {t.precision, t.n_tiles};
        std::memcpy(blob.data() + at + t.operand.size() + 64, tail, sizeof tail);
        entries[idx].n_tiles = t.n_tiles;
        entries[idx].precision = t.precision;
        if (set->one_tile && blob.size() - at != vdf::kSmallBoxTableStride) usable = false;  // (cannot happen: sizes <= 64 are one tile)
    }
    int r = VDF_OK;
    if (usable) {
        r = upload(ctx, set->blob, blob.data(), blob.size(), stream);
        if (r == VDF_OK) {
            for (size_t idx = 0; idx < n_idx; idx++) {
                if (!entries[idx].n_tiles) continue;
                entries[idx].operand = set->blob.as<uint8_t>() + offset[idx];
                entries[idx].bias = reinterpret_cast<const int32_t *>(set->blob.as<uint8_t>() + offset[idx] + (size_t)entries[idx].n_tiles * 2048);
            }
            r = upload(ctx, set->entries, entries.data(), entries.size() * sizeof(vdf::CropTableEntry), stream);
        }
        // (pageable sources: both copies have left the host buffers when hipMemcpyAsync returns, but the one-time wait keeps this like mfma_table)
        if (r == VDF_OK && hipStreamSynchronize(stream) != hipSuccess) r = fail(ctx, VDF_E_HIP, "table upload failed");
    }
    if (r != VDF_OK) {
        set->blob.release(); set->entries.release();
        delete set;
        *rc = r;
        return nullptr;
    }
    set->usable = usable;
    ctx->box_tables[key] = set;
    *rc = VDF_OK;
    return set;
}

vdf::ResizeAxisTable dev_view(const DeviceAxisTable *t)
{
    vdf::ResizeAxisTable v{};
    if (t) {
        v.start = t->start.as<int32_t>();
        v.size = t->size.as<int32_t>();
        v.w = t->w.as<int16_t>();
        v.window = t->host.window;
        v.precision = t->host.precision;
    }
    return v;
}

int ensure_cos_table(vdf_ctx *ctx, hipStream_t stream)
{
    if (ctx->cos_table.p) return VDF_OK;
    // [k][n] cosine matrix (kept for reference kernels), then the constants of the split-radix DCT-16 in the order
    // dct_hash.hip reads them: 4 + 2 + 1 twiddles (cos, sin) and sqrt(1/2).  Computed exactly as rustdct does
    // (twiddles::single_twiddle(i, len).conj(): angle = (-2 pi / len) * i) so that they equal the oracle's bit for bit.
    double tab[16 * 16 + 17];
    for (int k = 0; k < 16; k++)
        for (int n = 0; n < 16; n++) tab[k * 16 + n] = std::cos(M_PI * (double)k * ((double)n + 0.5) / 16.0);
    int at = 256;
    auto twiddle = [&](int i, int fft_len) {
        const double angle_constant = M_PI * -2.0 / (double)fft_len;
        const double angle = angle_constant * (double)i;
        tab[at++] = std::cos(angle);
        tab[at++] = -std::sin(angle);
    };
    for (int i = 0; i < 4; i++) twiddle(2 * i + 1, 64);
    for (int i = 0; i < 2; i++) twiddle(2 * i + 1, 32);
    twiddle(1, 16);
    tab[at++] = M_SQRT1_2;
    tab[at++] = 0.0; tab[at++] = 0.0;
    int rc = upload(ctx, ctx->cos_table, tab, sizeof tab, stream);
    if (rc) return rc;
    VDF_HIP(ctx, hipStreamSynchronize(stream));
    return VDF_OK;
}

using vdf::kMaxClipsPerLaunch;  // (resize_dispatch.h: the mixed planner cuts its parts by it too)

// One launch's worth of a hash call: at most kMaxClipsPerLaunch clips of it.
struct HashJob {
    const uint8_t *d_frames;
    size_t n_clips;
    uint32_t w, h;
    size_t frame_stride, clip_stride;
    uint64_t *d_out;
    uint32_t *d_dc;
    hipStream_t stream;
    uint64_t *d_zero = nullptr;  // the zero planes, or none
    vdf::HashCall call() const { return vdf::HashCall{d_frames, w, h, frame_stride, clip_stride, n_clips}; }
    const uint8_t *buf_end() const { return d_frames + (n_clips - 1) * clip_stride + (VDF_DCT_SIZE - 1) * frame_stride + (size_t)w * h; }
    HashJob clips(size_t c0, size_t n) const
    {
        return HashJob{d_frames + c0 * clip_stride, n, w, h, frame_stride, clip_stride, d_out + c0 * VDF_HASH_WORDS, d_dc ? d_dc + c0 : nullptr, stream,
                       d_zero ? d_zero + c0 * VDF_HASH_WORDS : nullptr};
    }
};

// Every hash entry: the argument checks, in the order their error codes are reported, then the call as launches of at most
// kMaxClipsPerLaunch clips: one(first clip, clips)
template <class One> int checked_launches(vdf_ctx *ctx, const HashJob &j, uint32_t frames_per_clip, One one)
{
    if (frames_per_clip < VDF_DCT_SIZE) return fail(ctx, VDF_E_NOT_ENOUGH_FRAMES, "fewer than 16 frames per clip");
    if (j.w == 0 || j.h == 0) return fail(ctx, VDF_E_BAD_DIMS, "zero frame dimension");
    if (j.frame_stride < (size_t)j.w * j.h) return fail(ctx, VDF_E_INVAL, "frame_stride smaller than a frame");
    if (j.n_clips == 0) return VDF_OK;
    if (!j.d_frames || !j.d_out) return fail(ctx, VDF_E_INVAL, "null pointer");
    for (size_t c0 = 0; c0 < j.n_clips; c0 += kMaxClipsPerLaunch)
        if (int rc = one(c0, std::min(kMaxClipsPerLaunch, j.n_clips - c0))) return rc;
    return VDF_OK;
}

vdf::HashKnobs hash_knobs(const vdf_ctx *ctx)
{
    return vdf::HashKnobs{ctx->resize_mode, ctx->wavestream_knob, ctx->hash_no_persistent != 0, ctx->no_rowcrop, ctx->rowcrop_all, ctx->no_boxstream,
                          ctx->no_smallcrop, ctx->lb_host_plan, ctx->no_lb_fused};
}

// mv null: the launch's clips name their vertical tables themselves (ROWCROP and box launches)
vdf::MfmaResizeArgs resize_args(const vdf_ctx *ctx, const DeviceMfmaTable *mh, const DeviceMfmaTable *mv)
{
    vdf::MfmaResizeArgs a{};
    a.bh = mh->operand.p;
    a.bias_h = mh->bias.as<int32_t>();
    a.prec_h = mh->host.precision;
    a.n_kt = mh->host.n_tiles;
    if (!mh->host.band_meta.empty()) {
        a.band_meta = mh->meta.as<int32_t>();
        a.band_stride = mh->host.band_stride;
    }
    if (mv) {
        a.av = mv->operand.p;
        a.bias_v = mv->bias.as<int32_t>();
        a.prec_v = mv->host.precision;
        a.n_rg = mv->host.n_tiles;
    }
    a.persistent_wgs_per_cu = ctx->hash_wgs_per_cu;
    return a;
}

int dct_hash_of_small(vdf_ctx *ctx, const HashJob &j)
{
    VDF_HIP(ctx, vdf::launch_dct_hash(ctx->small.as<uint8_t>(), 4096, 256, j.n_clips, ctx->cos_table.as<double>(), j.d_out, j.d_dc, j.stream, j.d_zero));
    return VDF_OK;
}

// Fetch the MFMA tables a plan names; a table that does not fit is what the plan could not know: plan again (plan_of(fit)) with that fact - the
// second plan ends in kScalar or kRefused.  *plan: the plan that stands; *mh, *mv: its tables (none for kDirect16, kScalar, kRefused).
template <class PlanOf>
int settle_plan(vdf_ctx *ctx, const HashJob &j, PlanOf plan_of, vdf::HashPlan *plan, DeviceMfmaTable **mh, DeviceMfmaTable **mv)
{
    using vdf::HashRoute;
    int rc = VDF_OK;
    *plan = plan_of(vdf::TableFit::kAll);
    *mh = *mv = nullptr;
    while (plan->route != HashRoute::kDirect16 && plan->route != HashRoute::kScalar && plan->route != HashRoute::kRefused) {
        *mh = mfma_table(ctx, j.w, plan->layout_h, j.stream, &rc);
        if (rc) return rc;
        if (!(*mh)->host.ok && plan->layout_h == vdf::kMfmaLayoutHorizontalBand) { *plan = plan_of(vdf::TableFit::kNoBand); continue; }
        *mv = mfma_table(ctx, j.h, plan->layout_v, j.stream, &rc);
        if (rc) return rc;
        if ((*mh)->host.ok && (*mv)->host.ok) break;
        *plan = plan_of(vdf::TableFit::kNoPlain);
    }
    return VDF_OK;
}

// The routes that resize apart from the DCT (chunk stream, wave stream, K-split, whole-line, scalar): frame f of clip c of the job to
// small + 4096 c + 256 f.  The plain call's second half (dct_hash_of_small follows) and the whole resize stage of the windows calls.
int resize_into_small(vdf_ctx *ctx, const HashJob &j, const vdf::HashPlan &plan, const DeviceMfmaTable *mh, const DeviceMfmaTable *mv, uint8_t *small)
{
    using vdf::HashRoute;
    switch (plan.route) {
    case HashRoute::kChunkStream:
    case HashRoute::kWaveStream:
        VDF_HIP(ctx, vdf::launch_resize_mfma_frames_stream(j.d_frames, j.n_clips, j.w, j.h, j.frame_stride, j.clip_stride, resize_args(ctx, mh, mv), plan, small, j.stream));
        return VDF_OK;
    case HashRoute::kKsplit:
        VDF_HIP(ctx, vdf::launch_resize_mfma_frames_ksplit(j.d_frames, j.n_clips, j.w, j.h, j.frame_stride, j.clip_stride, resize_args(ctx, mh, mv), plan, small, j.stream));
        return VDF_OK;
    case HashRoute::kWholeLine:
        VDF_HIP(ctx, vdf::launch_resize_mfma_frames(j.d_frames, j.n_clips, j.w, j.h, j.frame_stride, j.clip_stride, j.buf_end(), resize_args(ctx, mh, mv), small, j.stream));
        return VDF_OK;
    case HashRoute::kScalar: {  // scalar fixed-point resize (any coefficient range)
        const int need_h = (j.w != VDF_DCT_SIZE), need_v = (j.h != VDF_DCT_SIZE);
        int rc = VDF_OK;
        DeviceAxisTable *th = need_h ? axis_table(ctx, j.w, j.stream, &rc) : nullptr;
        if (rc) return rc;
        DeviceAxisTable *tv = need_v ? axis_table(ctx, j.h, j.stream, &rc) : nullptr;
        if (rc) return rc;
        int32_t y_first = 0, tmp_rows = VDF_DCT_SIZE;
        if (need_v) {
            y_first = tv->host.start[0];
            tmp_rows = tv->host.start[VDF_DCT_SIZE - 1] + tv->host.size[VDF_DCT_SIZE - 1] - y_first;
        }
        if ((size_t)tmp_rows * 16 > 64 * 1024) return fail(ctx, VDF_E_BAD_DIMS, "frame height above 4096 is not supported by the scalar resize kernel");
        VDF_HIP(ctx, vdf::launch_resize_generic(j.d_frames, j.n_clips, j.w, j.h, j.frame_stride, j.clip_stride, dev_view(th), dev_view(tv), need_h, need_v,
                                                y_first, tmp_rows, small, j.stream));
        return VDF_OK;
    }
    case HashRoute::kRefused: return fail(ctx, VDF_E_BAD_DIMS, "coefficients do not fit the i8 split");
    case HashRoute::kDirect16:
    case HashRoute::kPersistentOneTile:
    case HashRoute::kTiled:
    case HashRoute::kPerClipFused: break;
    }
    return fail(ctx, VDF_E_INVAL, "internal: a route that does not resize into the 16 x 16 buffer");
}

// Plan (resize_dispatch.h: plan_hash), fetch the tables the plan names, launch its route.
int hash_launch(vdf_ctx *ctx, const HashJob &j)
{
    using vdf::HashRoute;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure_cos_table(ctx, j.stream);
    if (rc) return rc;
    const vdf::HashKnobs knobs = hash_knobs(ctx);
    vdf::HashPlan plan;
    DeviceMfmaTable *mh = nullptr, *mv = nullptr;
    if ((rc = settle_plan(ctx, j, [&](vdf::TableFit fit) { return vdf::plan_hash(j.call(), knobs, fit); }, &plan, &mh, &mv))) return rc;
    switch (plan.route) {
    case HashRoute::kRefused: return fail(ctx, VDF_E_BAD_DIMS, "coefficients do not fit the i8 split");
    case HashRoute::kDirect16:
        VDF_HIP(ctx, vdf::launch_dct_hash(j.d_frames, j.clip_stride, j.frame_stride, j.n_clips, ctx->cos_table.as<double>(), j.d_out, j.d_dc, j.stream, j.d_zero));
        return VDF_OK;
    case HashRoute::kPersistentOneTile:
    case HashRoute::kTiled:
    case HashRoute::kPerClipFused:
        VDF_HIP(ctx, vdf::launch_resize_dct_fused(j.d_frames, j.n_clips, j.w, j.h, j.frame_stride, j.clip_stride, j.buf_end(), resize_args(ctx, mh, mv), plan,
                                                  ctx->cos_table.as<double>(), j.d_out, j.d_dc, j.stream, j.d_zero));
        return VDF_OK;
    default: break;
    }
    VDF_HIP(ctx, ctx->small.reserve(j.n_clips * 4096));
    if ((rc = resize_into_small(ctx, j, plan, mh, mv, ctx->small.as<uint8_t>()))) return rc;
    return dct_hash_of_small(ctx, j);
}

int hash_device_locked(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w,
                       uint32_t h, size_t frame_stride, size_t clip_stride, uint64_t *d_out, uint32_t *d_dc,
                       hipStream_t stream, uint64_t *d_zero)
{
    const HashJob all{d_frames, n_clips, w, h, frame_stride, clip_stride, d_out, d_dc, stream, d_zero};
    return checked_launches(ctx, all, frames_per_clip, [&](size_t c0, size_t n) { return hash_launch(ctx, all.clips(c0, n)); });
}

// ---- every 16-frame window of a clip (include/vdf.h: vdf_hash_windows_u8[_device]) ----------------------------------------------
// The resize stage of one run of 16-frame pseudo-clips (windows_plan.h): planned by plan_resize_only (resize_dispatch.h: the plain call's plan, with the
// routes that fuse the DCT sent to the whole-line or the scalar kernel), the plain call's tables and launchers, pseudo-clip i to small + 4096 i.
int windows_resize_run(vdf_ctx *ctx, const HashJob &j, uint8_t *small)
{
    const vdf::HashKnobs knobs = hash_knobs(ctx);
    vdf::HashPlan plan;
    DeviceMfmaTable *mh = nullptr, *mv = nullptr;
    if (int rc = settle_plan(ctx, j, [&](vdf::TableFit fit) { return vdf::plan_resize_only(j.call(), knobs, fit); }, &plan, &mh, &mv)) return rc;
    return resize_into_small(ctx, j, plan, mh, mv, small);
}

// the argument checks of the windows calls, in the order their codes are reported; *run: there is something to hash
int windows_checks(vdf_ctx *ctx, const void *frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h, size_t frame_stride,
                   uint32_t window_stride, const void *out_hashes, bool *run)
{
    *run = false;
    if (frames_per_clip < VDF_DCT_SIZE) return fail(ctx, VDF_E_NOT_ENOUGH_FRAMES, "fewer than 16 frames per clip");
    if (w == 0 || h == 0) return fail(ctx, VDF_E_BAD_DIMS, "zero frame dimension");
    if (frame_stride < (size_t)w * h) return fail(ctx, VDF_E_INVAL, "frame_stride smaller than a frame");
    if (window_stride == 0) return fail(ctx, VDF_E_INVAL, "window_stride of zero");
    const size_t n_win = vdf::window_count(frames_per_clip, window_stride);
    // (frame counts within 64 of 2^32 are refused with the same code: the kernel's frame arithmetic is 32-bit)
    if (frames_per_clip > 0xFFFFFFC0u || (n_clips && n_win > 0xFFFFFFFFull / n_clips)) return fail(ctx, VDF_E_INVAL, "2^32 windows or more in one call");
    if (n_clips == 0) return VDF_OK;
    if (!frames || !out_hashes) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "the windows calls take a single-device context");
    *run = true;
    return VDF_OK;
}

// windows_checks has passed.  The resize stage of every windows launch - plain, retimed, several rates - run once: the cosine table, then the
// clips' frames as 16 x 16 bytes, *out saying where they are (the caller's own buffer if they are 16 x 16 already).
int windows_frames_locked(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h, size_t frame_stride,
                          size_t clip_stride, hipStream_t stream, vdf::WindowsFrames *out)
{
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ensure_cos_table(ctx, stream)) return rc;
    vdf::WindowsFrames wf{};
    if (w == VDF_DCT_SIZE && h == VDF_DCT_SIZE) {  // the resize is a copy: the kernel reads the caller's frames
        wf.base = wf.tail = d_frames;
        wf.clip_stride = clip_stride;
        wf.chunk_stride = 16 * frame_stride;
        wf.frame_stride = frame_stride;
        wf.main_frames = frames_per_clip;
        wf.dwords = (((uintptr_t)d_frames | frame_stride | clip_stride) & 3u) == 0;
    } else {
        const vdf::WindowsResizePlan rp = vdf::plan_windows_resize(n_clips, frames_per_clip, frame_stride, clip_stride);
        VDF_HIP(ctx, ctx->small.reserve(rp.small_bytes));
        uint8_t *small = ctx->small.as<uint8_t>();
        for (const vdf::WindowsResizeRun &r : vdf::windows_resize_runs(rp, n_clips, frames_per_clip, frame_stride, clip_stride))
            for (size_t c0 = 0; c0 < r.n; c0 += kMaxClipsPerLaunch) {  // launches of at most kMaxClipsPerLaunch pseudo-clips
                const HashJob j{d_frames + r.src_offset + c0 * r.step, std::min(kMaxClipsPerLaunch, r.n - c0), w, h, frame_stride, r.step, nullptr, nullptr, stream};
                if (int rc = windows_resize_run(ctx, j, small + r.dst_offset + c0 * 4096)) return rc;
            }
        wf.base = small;
        wf.tail = small + rp.tail_offset;
        wf.clip_stride = rp.clip_step;
        wf.chunk_stride = rp.chunk_step;
        wf.frame_stride = 256;
        wf.tail_clip_stride = 4096;
        wf.main_frames = 16 * rp.n_chunks;
        wf.tail_first = frames_per_clip - 16;
        wf.dwords = true;
    }
    *out = wf;
    return VDF_OK;
}

// windows_checks has passed.  d_zero (nullable): the windows' zero planes as well - the same resize runs and routes, the kernel's PLANES form
// retimed (nullable; d_zero is null then): the retimed windows of that plan (windows_retimed_plan.h) - the same resize stage, the retimed kernel
int hash_windows_locked(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h, size_t frame_stride,
                        size_t clip_stride, uint32_t window_stride, uint64_t *d_out, uint32_t *d_dc, hipStream_t stream, uint64_t *d_zero = nullptr,
                        const vdf::WindowsRetimedPlan *retimed = nullptr)
{
    vdf::WindowsFrames wf{};
    if (int rc = windows_frames_locked(ctx, d_frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride, stream, &wf)) return rc;
    const vdf::WindowsPlan plan = vdf::plan_windows(frames_per_clip, window_stride);
    if (retimed) VDF_HIP(ctx, vdf::launch_dct_hash_windows_retimed(wf, n_clips, *retimed, ctx->cos_table.as<double>(), d_out, d_dc, stream));
    else VDF_HIP(ctx, vdf::launch_dct_hash_windows(wf, n_clips, plan, ctx->cos_table.as<double>(), d_out, d_dc, stream, d_zero));
    return VDF_OK;
}

// the rate checks of the retimed windows calls, behind windows_checks' (whose window count is the plain one: an upper bound of the retimed one)
int windows_retimed_checks(vdf_ctx *ctx, uint32_t frames_per_clip, uint32_t rate_num, uint32_t rate_den)
{
    if (!vdf::retimed_rate_ok(rate_num, rate_den)) return fail(ctx, VDF_E_INVAL, "rate outside 1 <= den <= num <= 2 den, num <= 65535");
    if (frames_per_clip < vdf::retimed_span(rate_num, rate_den)) return fail(ctx, VDF_E_NOT_ENOUGH_FRAMES, "fewer frames per clip than a retimed window spans");
    return VDF_OK;
}

// The tables that the descriptors of one launch name, by (box size, axis): each is fetched, and gets its entry, where a box first asks for it.
// Arrays over the sizes, not a map: 20 000 clips were 0.19 ms of host time through a map, with the GPU idle behind the wait for the boxes;
// w + 1 and h + 1 slots are small at every supported size.
struct LaunchTables {
    int layout_h, layout_v;
    std::vector<int32_t> at_h, at_v;            // [size] -> entry, -1 = not asked for yet
    std::vector<const DeviceMfmaTable *> used;  // [entry]
    LaunchTables(uint32_t w, uint32_t h, int lh, int lv) : layout_h(lh), layout_v(lv), at_h(w + 1, -1), at_v(h + 1, -1) {}
    // -1: *rc is set, or (*rc == VDF_OK) the table does not fit the i8 split
    int32_t entry(vdf_ctx *ctx, uint32_t size, bool vertical, hipStream_t stream, int *rc)
    {
        int32_t &at = (vertical ? at_v : at_h)[size];
        if (at >= 0) return at;
        const DeviceMfmaTable *t = mfma_table(ctx, size, vertical ? layout_v : layout_h, stream, rc);
        if (*rc || !t->host.ok) return -1;
        used.push_back(t);
        return at = (int32_t)used.size() - 1;
    }
    vdf::CropTableEntry crop_entry(size_t i) const { return vdf::CropTableEntry{used[i]->operand.p, used[i]->bias.as<int32_t>(), used[i]->host.n_tiles, used[i]->host.precision}; }
    vdf::CropStreamTable stream_entry(size_t i) const
    {
        const DeviceMfmaTable *t = used[i];
        return vdf::CropStreamTable{t->operand.p, t->bias.as<int32_t>(), t->host.band_meta.empty() ? nullptr : t->meta.as<int32_t>(), t->host.n_tiles,
                                    t->host.precision, t->host.band_stride, 0};
    }
};

int no_split_table(vdf_ctx *ctx) { return fail(ctx, VDF_E_BAD_DIMS, "crop box size whose coefficients do not fit the i8 split"); }

// Small frames: ONE pass over the boxes - check, table entries by box size, descriptors written straight into the pinned staging - then one
// upload and one launch that resizes, transforms and hashes (resize_dct_hash_cropped_small_kernel).
int hash_cropped_small(vdf_ctx *ctx, const HashJob &j, const uint32_t *crops)
{
    const uint32_t w = j.w, h = j.h;
    const size_t nd = j.n_clips * sizeof(vdf::CropClipDesc), off = (nd + 63) & ~size_t(63);
    if (!ctx->pin_desc.reserve(off + ((size_t)w + h + 2) * sizeof(vdf::CropTableEntry))) return fail(ctx, VDF_E_OOM, "host staging for the crop descriptors");
    vdf::CropClipDesc *dsc = ctx->pin_desc.as<vdf::CropClipDesc>();
    vdf::CropTableEntry *ent = reinterpret_cast<vdf::CropTableEntry *>(ctx->pin_desc.as<char>() + off);
    LaunchTables tabs(w, h, vdf::kMfmaLayoutHorizontal, vdf::kMfmaLayoutVertical);
    int rc = VDF_OK;
    for (size_t c = 0; c < j.n_clips; c++) {
        const uint32_t l = crops[4 * c], r = crops[4 * c + 1], t = crops[4 * c + 2], b = crops[4 * c + 3];
        if ((uint64_t)l + r >= w || (uint64_t)t + b >= h) return fail(ctx, VDF_E_INVAL, "crop box leaves no pixels");  // crop.rs:21-22
        const uint32_t bw = w - l - r, bh = h - t - b;
        const int32_t ih = tabs.entry(ctx, bw, false, j.stream, &rc), iv = ih < 0 ? -1 : tabs.entry(ctx, bh, true, j.stream, &rc);
        if (iv < 0) return rc ? rc : no_split_table(ctx);
        dsc[c] = vdf::CropClipDesc{l, t, bw, bh, (uint32_t)ih, (uint32_t)iv, (uint32_t)c, 0u};
    }
    for (size_t i = 0; i < tabs.used.size(); i++) ent[i] = tabs.crop_entry(i);
    if ((rc = upload(ctx, ctx->crop_desc2, dsc, nd, j.stream))) return rc;
    if ((rc = upload(ctx, ctx->crop_tables2, ent, std::max<size_t>(tabs.used.size(), 1) * sizeof(vdf::CropTableEntry), j.stream))) return rc;
    VDF_HIP(ctx, hipEventRecord(ctx->ev_mid, j.stream));
    VDF_HIP(ctx, vdf::launch_resize_dct_cropped_small(j.d_frames, j.n_clips, w, j.frame_stride, j.clip_stride, j.buf_end(), ctx->crop_desc2.as<vdf::CropClipDesc>(),
                                                      ctx->crop_tables2.as<vdf::CropTableEntry>(), ctx->cos_table.as<double>(), j.d_out, j.d_dc, j.stream, j.d_zero));
    // the staging is read by the two copies: they must have run before the next call on this context rewrites it (the kernel stays queued)
    VDF_HIP(ctx, hipEventSynchronize(ctx->ev_mid));
    return VDF_OK;
}

// The host descriptors of a planned cropped call (resize_dispatch.h: CropPlan), part by part.
struct CropDescs {
    const DeviceMfmaTable *rows_mh = nullptr;      // the ROWCROP launch's horizontal table
    std::vector<const DeviceMfmaTable *> group_mh;  // each box launch's band table
    std::vector<size_t> group_first;                // ... and its first entry of row_clips
    std::vector<vdf::CropStreamClip> row_clips, gather_clips;  // the ROWCROP launch's clips, then every box launch's; the gather stream kernel's
    std::vector<vdf::CropStreamTable> row_tables, gather_tables;
    std::vector<vdf::CropClipDesc> line_clips;  // the whole-line cropped kernel's
    std::vector<vdf::CropTableEntry> line_tables;
};

vdf::CropStreamClip stream_clip(const HashJob &j, const uint32_t *crops, uint32_t c)
{
    vdf::CropStreamClip q{};
    q.x0 = crops[4 * c]; q.y0 = crops[4 * c + 2]; q.w = j.w - q.x0 - crops[4 * c + 1]; q.h = j.h - q.y0 - crops[4 * c + 3]; q.src_clip = c;
    return q;
}

// Fetches the tables and builds the descriptors of every part.  *again: a table does not fit - what the plan could not know is noted in *fit,
// and the caller plans again.
int build_crop_descs(vdf_ctx *ctx, const HashJob &j, const uint32_t *crops, const vdf::CropPlan &plan, vdf::CropTableFit *fit, CropDescs *d, bool *again)
{
    int rc = VDF_OK;
    *d = CropDescs();
    *again = true;
    if (plan.rows_kernel.route != vdf::HashRoute::kRefused) {
        d->rows_mh = mfma_table(ctx, j.w, plan.rows_kernel.layout_h, j.stream, &rc);
        if (rc) return rc;
        if (!d->rows_mh->host.ok) { fit->rows_table = false; return VDF_OK; }
    }
    for (const vdf::CropBoxGroup &g : plan.groups) {
        const DeviceMfmaTable *mh = mfma_table(ctx, g.box_w, vdf::kMfmaLayoutHorizontalBand, j.stream, &rc);
        if (rc) return rc;
        if (!mh->host.ok || !vdf::resize_wavestream_table_fits(g.waves, mh->host.band_stride)) { fit->ranges_without_table.push_back(vdf::crop_range_key(g.x0, g.box_w)); return VDF_OK; }
        d->group_mh.push_back(mh);
    }
    // full-width boxes and the boxes of a column range: rows y0 .. y0 + h at the frame's pitch, a vertical table per box height
    LaunchTables row_tabs(j.w, j.h, vdf::kMfmaLayoutHorizontal, vdf::kMfmaLayoutVertical);
    const auto append_rows = [&](const std::vector<uint32_t> &ids) -> bool {
        for (uint32_t c : ids) {
            vdf::CropStreamClip q = stream_clip(j, crops, c);
            q.wp = j.w;
            const int32_t iv = row_tabs.entry(ctx, q.h, true, j.stream, &rc);
            if (iv < 0) return false;
            q.v_table = (uint32_t)iv;
            d->row_clips.push_back(q);
        }
        return true;
    };
    bool rows_ok = append_rows(plan.rows);
    for (const vdf::CropBoxGroup &g : plan.groups) {
        d->group_first.push_back(d->row_clips.size());
        rows_ok = rows_ok && append_rows(g.ids);
    }
    if (rc) return rc;
    if (!rows_ok) { fit->height_tables = false; return VDF_OK; }
    for (size_t i = 0; i < row_tabs.used.size(); i++) d->row_tables.push_back(row_tabs.stream_entry(i));
    if (plan.rest_gather) {  // gathered boxes: LDS pitch and chunk geometry per box, the horizontal table in band form
        LaunchTables tabs(j.w, j.h, vdf::kMfmaLayoutHorizontalBand, vdf::kMfmaLayoutVertical);
        for (uint32_t c : plan.rest) {
            vdf::CropStreamClip q = stream_clip(j, crops, c);
            q.nb = vdf::resize_cropped_stream_blocks(q.w, q.x0, j.w, plan.gather_cls, &q.wp);
            q.step_rows = 4096u / q.wp;
            q.step_x = 4096u - q.step_rows * q.wp;
            q.n_chunks = (q.h + 16 * q.nb - 1) / (16 * q.nb);
            const int32_t ih = tabs.entry(ctx, q.w, false, j.stream, &rc), iv = ih < 0 ? -1 : tabs.entry(ctx, q.h, true, j.stream, &rc);
            if (rc) return rc;
            if (iv < 0) { fit->gather_tables = false; return VDF_OK; }
            q.h_table = (uint32_t)ih; q.v_table = (uint32_t)iv;
            d->gather_clips.push_back(q);
        }
        for (size_t i = 0; i < tabs.used.size(); i++) d->gather_tables.push_back(tabs.stream_entry(i));
    } else {  // frames at least 1.5 windows wide read whole 128-byte lines (resize_row_quads)
        LaunchTables tabs(j.w, j.h, vdf::kMfmaLayoutHorizontal, j.w >= 192 ? vdf::kMfmaLayoutVerticalWide : vdf::kMfmaLayoutVertical);
        for (uint32_t c : plan.rest) {
            const vdf::CropStreamClip q = stream_clip(j, crops, c);
            const int32_t ih = tabs.entry(ctx, q.w, false, j.stream, &rc), iv = ih < 0 ? -1 : tabs.entry(ctx, q.h, true, j.stream, &rc);
            if (iv < 0) return rc ? rc : no_split_table(ctx);
            d->line_clips.push_back(vdf::CropClipDesc{q.x0, q.y0, q.w, q.h, (uint32_t)ih, (uint32_t)iv, c, 0u});
        }
        for (size_t i = 0; i < tabs.used.size(); i++) d->line_tables.push_back(tabs.crop_entry(i));
    }
    *again = false;
    return VDF_OK;
}

template <class Clip, class Table>
int upload_descs(vdf_ctx *ctx, const std::vector<Clip> &clips, const std::vector<Table> &tables, DevBuf &bd, DevBuf &bt, hipStream_t stream)
{
    int rc = upload(ctx, bd, clips.data(), clips.size() * sizeof(Clip), stream);
    return rc ? rc : upload(ctx, bt, tables.data(), tables.size() * sizeof(Table), stream);
}

// Uploads the descriptors, launches every part, then dct_hash over the whole batch.
int launch_crop_parts(vdf_ctx *ctx, const HashJob &j, const vdf::CropPlan &plan, const CropDescs &d)
{
    int rc = VDF_OK;
    if (!d.row_clips.empty() && (rc = upload_descs(ctx, d.row_clips, d.row_tables, ctx->crop_desc, ctx->crop_tables, j.stream))) return rc;
    if (plan.rest_gather) {
        if ((rc = upload_descs(ctx, d.gather_clips, d.gather_tables, ctx->crop_desc2, ctx->crop_tables2, j.stream))) return rc;
    } else if (!plan.rest.empty()) {
        // through pinned staging (consumed by the time of the wait below): a descriptor per clip is 0.6 MB for 20 000 small clips
        const size_t nd = d.line_clips.size() * sizeof(vdf::CropClipDesc), nt = d.line_tables.size() * sizeof(vdf::CropTableEntry), off = (nd + 63) & ~size_t(63);
        if (!ctx->pin_desc.reserve(off + nt)) return fail(ctx, VDF_E_OOM, "host staging for the crop descriptors");
        std::memcpy(ctx->pin_desc.p, d.line_clips.data(), nd);
        std::memcpy(ctx->pin_desc.as<char>() + off, d.line_tables.data(), nt);
        if ((rc = upload(ctx, ctx->crop_desc2, ctx->pin_desc.p, nd, j.stream))) return rc;
        if ((rc = upload(ctx, ctx->crop_tables2, ctx->pin_desc.as<char>() + off, nt, j.stream))) return rc;
    }
    VDF_HIP(ctx, hipStreamSynchronize(j.stream));  // the host vectors go out of scope with this call
    VDF_HIP(ctx, ctx->small.reserve(j.n_clips * 4096));
    uint8_t *small = ctx->small.as<uint8_t>();
    const vdf::CropStreamClip *row_clips = ctx->crop_desc.as<vdf::CropStreamClip>();
    const vdf::CropStreamTable *row_tables = ctx->crop_tables.as<vdf::CropStreamTable>();
    if (plan.rows_kernel.route == vdf::HashRoute::kKsplit)
        VDF_HIP(ctx, vdf::launch_resize_mfma_frames_ksplit(j.d_frames, plan.rows.size(), j.w, j.h, j.frame_stride, j.clip_stride, resize_args(ctx, d.rows_mh, nullptr),
                                                           plan.rows_kernel, small, j.stream, row_clips, row_tables));
    else if (!plan.rows.empty())
        VDF_HIP(ctx, vdf::launch_resize_mfma_frames_stream(j.d_frames, plan.rows.size(), j.w, j.h, j.frame_stride, j.clip_stride, resize_args(ctx, d.rows_mh, nullptr),
                                                           plan.rows_kernel, small, j.stream, row_clips, row_tables));
    for (size_t i = 0; i < plan.groups.size(); i++) {
        const vdf::CropBoxGroup &g = plan.groups[i];
        VDF_HIP(ctx, vdf::launch_resize_mfma_box_wavestream(j.d_frames, g.ids.size(), j.w, j.h, j.frame_stride, j.clip_stride, resize_args(ctx, d.group_mh[i], nullptr),
                                                            g.x0, g.box_w, g.waves, row_clips + d.group_first[i], row_tables, small, j.stream));
    }
    if (plan.rest_gather)
        VDF_HIP(ctx, vdf::launch_resize_mfma_cropped_stream(j.d_frames, plan.rest.size(), j.w, j.h, j.frame_stride, j.clip_stride, ctx->crop_desc2.as<vdf::CropStreamClip>(),
                                                            ctx->crop_tables2.as<vdf::CropStreamTable>(), plan.gather_cls, plan.gather_shift, small, j.stream));
    else if (!plan.rest.empty())
        VDF_HIP(ctx, vdf::launch_resize_mfma_cropped(j.d_frames, plan.rest.size(), j.w, j.frame_stride, j.clip_stride, j.buf_end(), ctx->crop_desc2.as<vdf::CropClipDesc>(),
                                                     ctx->crop_tables2.as<vdf::CropTableEntry>(), small, j.w >= 192, j.stream));
    return dct_hash_of_small(ctx, j);
}

int hash_cropped_launch(vdf_ctx *ctx, const HashJob &j, const uint32_t *crops)
{
    bool any = false;
    if (crops)
        for (size_t i = 0; i < j.n_clips * 4 && !any; i++) any = crops[i] != 0;
    if (!any) return hash_launch(ctx, j);  // the common case, before any planning: the fused / persistent kernels
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure_cos_table(ctx, j.stream);
    if (rc) return rc;
    const vdf::HashKnobs knobs = hash_knobs(ctx);
    vdf::CropTableFit fit;
    vdf::CropPlan plan;
    CropDescs descs;
    for (bool again = true; again;) {  // (every further round has one more fact in `fit`, and there are finitely many)
        plan = vdf::plan_cropped(j.call(), knobs, crops, fit);
        if (plan.kind == vdf::CropPlan::kBadBox) return fail(ctx, VDF_E_INVAL, "crop box leaves no pixels");
        if (plan.kind == vdf::CropPlan::kSmall) return hash_cropped_small(ctx, j, crops);
        if ((rc = build_crop_descs(ctx, j, crops, plan, &fit, &descs, &again))) return rc;
    }
    return launch_crop_parts(ctx, j, plan, descs);
}

// Hash clips whose crop boxes (HOST array [n_clips][4] = left, right, top, bottom; null = no crop) are read in place.
int hash_cropped_locked(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w,
                        uint32_t h, size_t frame_stride, size_t clip_stride, const uint32_t *crops, uint64_t *d_out,
                        uint32_t *d_dc, hipStream_t stream)
{
    const HashJob all{d_frames, n_clips, w, h, frame_stride, clip_stride, d_out, d_dc, stream};
    return checked_launches(ctx, all, frames_per_clip, [&](size_t c0, size_t n) { return hash_cropped_launch(ctx, all.clips(c0, n), crops ? crops + 4 * c0 : nullptr); });
}

// ---- clips of different frame sizes in one call (include/vdf.h: vdf_hash_clips_u8[_device]) ------------------------------------------------------
static_assert(sizeof(vdf_clip) == sizeof(vdf::MixedClip) && offsetof(vdf_clip, offset) == offsetof(vdf::MixedClip, offset) &&
              offsetof(vdf_clip, frame_stride) == offsetof(vdf::MixedClip, frame_stride) && offsetof(vdf_clip, w) == offsetof(vdf::MixedClip, w) &&
              offsetof(vdf_clip, h) == offsetof(vdf::MixedClip, h) && offsetof(vdf_clip, crop_left) == offsetof(vdf::MixedClip, crop) &&
              offsetof(vdf_clip, crop_bottom) == offsetof(vdf::MixedClip, crop) + 12, "the planner reads vdf_clip as vdf::MixedClip");

int mixed_check_failed(vdf_ctx *ctx, const vdf::MixedCheck &c)
{
    const std::string at = " (clip " + std::to_string(c.clip) + ")";
    switch (c.error) {
    case vdf::MixedError::kNotEnoughFrames: return fail(ctx, VDF_E_NOT_ENOUGH_FRAMES, "fewer than 16 frames per clip");
    case vdf::MixedError::kZeroDim: return fail(ctx, VDF_E_BAD_DIMS, "zero frame dimension" + at);
    case vdf::MixedError::kStrideBelowFrame: return fail(ctx, VDF_E_INVAL, "frame_stride smaller than a frame" + at);
    case vdf::MixedError::kEmptyBox: return fail(ctx, VDF_E_INVAL, "crop box leaves no pixels" + at);
    case vdf::MixedError::kOutOfBuffer: return fail(ctx, VDF_E_INVAL, "clip reaches past the end of the buffer" + at);
    case vdf::MixedError::kCropGiven: return fail(ctx, VDF_E_INVAL, "caller-supplied crop box in a letterbox call" + at);
    case vdf::MixedError::kNone: break;
    }
    return VDF_OK;
}

// The mixed parts: table entries by box size, every descriptor through the pinned staging in ONE upload for the whole call (so no launch of
// the call rewrites staging another launch's upload still reads), then the launches of the plan and the DCT of the per-frame parts.
int hash_mixed_launch(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf::MixedPlan &plan, uint64_t *d_out, uint32_t *d_dc, hipStream_t stream,
                      uint64_t *d_zero)
{
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure_cos_table(ctx, stream);
    if (rc) return rc;
    const size_t n = plan.descs.size(), nd = n * sizeof(vdf::MixedClipDesc), off = (nd + 63) & ~size_t(63);
    const size_t max_entries = 2 * ((size_t)plan.max_w + plan.max_h + 2);
    if (!ctx->pin_desc.reserve(off + max_entries * sizeof(vdf::CropTableEntry))) return fail(ctx, VDF_E_OOM, "host staging for the clip descriptors");
    vdf::MixedClipDesc *dsc = ctx->pin_desc.as<vdf::MixedClipDesc>();
    vdf::CropTableEntry *ent = reinterpret_cast<vdf::CropTableEntry *>(ctx->pin_desc.as<char>() + off);
    // two sets: the whole-line part reads its vertical tables in another k order
    LaunchTables plain(plan.max_w, plan.max_h, vdf::kMfmaLayoutHorizontal, vdf::kMfmaLayoutVertical), wide(plan.max_w, plan.max_h, vdf::kMfmaLayoutHorizontal, vdf::kMfmaLayoutVerticalWide);
    for (const vdf::MixedLaunch &l : plan.launches) {
        LaunchTables &tabs = l.part == vdf::MixedPart::kWideLines ? wide : plain;
        for (size_t i = l.first; i < l.first + l.count; i++) {
            vdf::MixedClipDesc d = plan.descs[i];
            const int32_t ih = tabs.entry(ctx, d.bw, false, stream, &rc), iv = ih < 0 ? -1 : tabs.entry(ctx, d.bh, true, stream, &rc);
            if (iv < 0) return rc ? rc : fail(ctx, VDF_E_BAD_DIMS, "box size whose coefficients do not fit the i8 split (clip " + std::to_string(d.out_index) + ")");
            d.h_table = (uint32_t)ih; d.v_table = (uint32_t)iv;
            dsc[i] = d;
        }
    }
    const size_t n_plain = plain.used.size(), n_entries = n_plain + wide.used.size();
    if (n_entries > max_entries) return fail(ctx, VDF_E_INVAL, "table index of a mixed call outgrew its staging");  // (cannot happen: one entry per size and axis)
    for (size_t i = 0; i < n_plain; i++) ent[i] = plain.crop_entry(i);
    for (size_t i = n_plain; i < n_entries; i++) ent[i] = wide.crop_entry(i - n_plain);
    for (const vdf::MixedLaunch &l : plan.launches)
        for (size_t i = l.first; i < l.first + l.count; i++) {
            if (l.part == vdf::MixedPart::kWideLines) { dsc[i].h_table += (uint32_t)n_plain; dsc[i].v_table += (uint32_t)n_plain; }
            if (dsc[i].h_table >= n_entries || dsc[i].v_table >= n_entries || dsc[i].out_index >= n) return fail(ctx, VDF_E_INVAL, "descriptor names a table or an output that is not there");
        }
    const size_t n_frames_part = n - plan.n_small;
    VDF_HIP(ctx, ctx->small.reserve(std::max<size_t>(n_frames_part, 1) * 4096));
    if ((rc = upload(ctx, ctx->crop_desc2, dsc, nd, stream))) return rc;
    if ((rc = upload(ctx, ctx->crop_tables2, ent, n_entries * sizeof(vdf::CropTableEntry), stream))) return rc;
    VDF_HIP(ctx, hipEventRecord(ctx->ev_mid, stream));
    const vdf::MixedClipDesc *d_desc = ctx->crop_desc2.as<vdf::MixedClipDesc>();
    const vdf::CropTableEntry *d_tab = ctx->crop_tables2.as<vdf::CropTableEntry>();
    const uint8_t *buf_end = d_buf + buf_bytes;
    uint8_t *small = ctx->small.as<uint8_t>();
    hipError_t e = hipSuccess;
    for (const vdf::MixedLaunch &l : plan.launches) {
        if (e != hipSuccess) break;
        if (l.part == vdf::MixedPart::kSmall) {
            e = vdf::launch_mixed_small(d_buf, buf_end, d_desc + l.first, l.count, d_tab, ctx->cos_table.as<double>(), d_out, d_dc, stream, d_zero);
        } else {
            uint8_t *slot0 = small + (l.first - plan.n_small) * 4096;
            e = vdf::launch_mixed_frames(d_buf, buf_end, d_desc + l.first, l.count, d_tab, l.part == vdf::MixedPart::kWideLines, slot0, stream);
            if (e == hipSuccess) e = vdf::launch_dct_hash_indexed(slot0, d_desc + l.first, l.count, ctx->cos_table.as<double>(), d_out, d_dc, stream, d_zero);
        }
    }
    // the staging is read by the two copies: they must have run before the next call on this context rewrites it (the kernels stay queued)
    const hipError_t ew = hipEventSynchronize(ctx->ev_mid);
    if (e != hipSuccess) return fail_hip(ctx, e, "mixed hash launch");
    VDF_HIP(ctx, ew);
    return VDF_OK;
}

int hash_clips_locked(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips, uint32_t frames_per_clip,
                      uint64_t *d_out, uint32_t *d_dc, hipStream_t stream, uint64_t *d_zero)
{
    if (n_clips && !clips) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (n_clips > 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "more than 2^32 - 1 clips in one call");
    const vdf::MixedClip *mc = reinterpret_cast<const vdf::MixedClip *>(clips);
    const vdf::MixedCheck chk = vdf::check_mixed(mc, n_clips, frames_per_clip, buf_bytes);
    if (chk.error != vdf::MixedError::kNone) return mixed_check_failed(ctx, chk);
    if (n_clips == 0) return VDF_OK;
    if (!d_buf || !d_out) return fail(ctx, VDF_E_INVAL, "null pointer");
    const vdf::MixedPlan plan = vdf::plan_mixed(mc, n_clips, hash_knobs(ctx));
    if (plan.kind == vdf::MixedPlan::kUniform) {  // one size, evenly spaced: exactly the uniform call
        std::vector<uint32_t> crops;
        if (plan.cropped) {
            crops.resize(n_clips * 4);
            for (size_t i = 0; i < n_clips; i++) std::memcpy(&crops[4 * i], mc[i].crop, 16);
        }
        const HashJob all{d_buf + plan.offset0, n_clips, mc[0].w, mc[0].h, (size_t)mc[0].frame_stride, (size_t)plan.clip_stride, d_out, d_dc, stream, d_zero};
        return checked_launches(ctx, all, frames_per_clip,
                                [&](size_t c0, size_t n) { return hash_cropped_launch(ctx, all.clips(c0, n), plan.cropped ? crops.data() + 4 * c0 : nullptr); });
    }
    return hash_mixed_launch(ctx, d_buf, buf_bytes, plan, d_out, d_dc, stream, d_zero);
}

// Small frames: the boxes stay on the device.  No copy to the host, no wait, no host loop over the clips between the launches; out_crops is
// filled by one copy queued behind them and waited for at the END of the call (d_out_crops: no wait at all).
int letterbox_small(vdf_ctx *ctx, const HashJob &j, uint32_t frames_per_clip, const vdf::LetterboxPlan &plan, const BoxTableSet *set, uint32_t *out_crops,
                    uint32_t *d_crops)
{
    const size_t n_fused = j.n_clips - plan.n_tail;
    if (n_fused)
        VDF_HIP(ctx, vdf::launch_letterbox_hash_small(j.d_frames, n_fused, j.w, j.h, j.frame_stride, j.clip_stride, set->blob.p, ctx->cos_table.as<double>(),
                                                      j.d_out, j.d_dc, d_crops, ctx->hash_wgs_per_cu_set ? ctx->hash_wgs_per_cu : 0, j.stream));
    if (plan.n_tail) {
        const HashJob tail = j.clips(n_fused, plan.n_tail);
        VDF_HIP(ctx, ctx->crop_work.reserve(vdf::letterbox_work_bytes(tail.n_clips, frames_per_clip)));
        VDF_HIP(ctx, vdf::launch_letterbox(tail.d_frames, tail.n_clips, frames_per_clip, j.w, j.h, j.frame_stride, j.clip_stride, d_crops + 4 * n_fused,
                                           ctx->crop_work.as<uint32_t>(), j.stream, ctx->lb_side_strips));
        VDF_HIP(ctx, vdf::launch_resize_dct_cropped_small_boxes(tail.d_frames, tail.n_clips, j.w, j.h, j.frame_stride, j.clip_stride, j.buf_end(), d_crops + 4 * n_fused,
                                                                set->entries.as<vdf::CropTableEntry>(), ctx->cos_table.as<double>(), tail.d_out, tail.d_dc, j.stream));
    }
    if (out_crops) {
        if (!ctx->pin_crops.reserve(j.n_clips * 16)) return fail(ctx, VDF_E_OOM, "host staging for the crop boxes");
        VDF_HIP(ctx, hipMemcpyAsync(ctx->pin_crops.p, d_crops, j.n_clips * 16, hipMemcpyDeviceToHost, j.stream));
        VDF_HIP(ctx, hipEventRecord(ctx->ev_mid, j.stream));
        VDF_HIP(ctx, hipEventSynchronize(ctx->ev_mid));  // everything of this call is queued: the wait costs the GPU nothing
        std::memcpy(out_crops, ctx->pin_crops.p, j.n_clips * 16);
    }
    return VDF_OK;
}

int letterbox_launch(vdf_ctx *ctx, const HashJob &j, uint32_t frames_per_clip, uint32_t *out_crops, uint32_t *d_out_crops)
{
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t *d_crops = d_out_crops;  // (the detect writes straight into the caller's d_out_crops when given)
    if (!d_crops) {
        VDF_HIP(ctx, ctx->crops.reserve(j.n_clips * 16));
        d_crops = ctx->crops.as<uint32_t>();
    }
    const vdf::LetterboxPlan plan = vdf::plan_letterbox(j.call(), hash_knobs(ctx));
    if (plan.small_frames) {  // every box size's tables are resident (box_table_set), so the kernels find a box's tables by its size
        int rc = ensure_cos_table(ctx, j.stream);
        if (rc) return rc;
        const BoxTableSet *set = box_table_set(ctx, j.w, j.h, j.stream, &rc);
        if (rc) return rc;
        if (set->usable) return letterbox_small(ctx, j, frames_per_clip, plan, set, out_crops, d_crops);
    }
    // (Cutting a large batch into chunks whose detect passes run on a second stream under the resize of the chunks before them was
    // built and measured in round 5 - profiles/r05_letterbox_ab.txt: the resize kernels fill every CU's LDS, so the walkers only got in
    // between the chunks, and three chunk boundaries cost more than the hidden detect time saved: 1000 pillarboxed 1080p clips 5.45 ms
    // against 5.32.  The detect pass was made faster instead: csrc/cropdetect.hip.)
    // Larger frames: which kernel a box takes (row-range stream, column-range stream, gather, whole-line) and the tables of its size are
    // decided per box SHAPE on the host - tables for every box size of a 1080p frame would be 50 MB and a second of host time per frame size -
    // so the boxes come down once and the call waits for the detect.
    VDF_HIP(ctx, ctx->crop_work.reserve(vdf::letterbox_work_bytes(j.n_clips, frames_per_clip)));
    VDF_HIP(ctx, vdf::launch_letterbox(j.d_frames, j.n_clips, frames_per_clip, j.w, j.h, j.frame_stride, j.clip_stride, d_crops, ctx->crop_work.as<uint32_t>(),
                                       j.stream, ctx->lb_side_strips));
    // (pinned: a pageable destination makes the copy synchronous and slow - 0.3 MB for 20 000 clips)
    if (!ctx->pin_crops.reserve(j.n_clips * 16)) return fail(ctx, VDF_E_OOM, "host staging for the crop boxes");
    uint32_t *crops = ctx->pin_crops.as<uint32_t>();
    VDF_HIP(ctx, hipMemcpyAsync(crops, d_crops, j.n_clips * 16, hipMemcpyDeviceToHost, j.stream));
    VDF_HIP(ctx, hipEventRecord(ctx->ev_wait, j.stream));
    if (int rcw = wait_event(ctx, ctx->ev_wait)) return rcw;  // (behind the frames' upload when they come from the host: milliseconds)
    if (out_crops) std::memcpy(out_crops, crops, j.n_clips * 16);
    return hash_cropped_launch(ctx, j, crops);
}

int letterbox_hash_device_locked(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                                 uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride, uint64_t *d_out,
                                 uint32_t *d_dc, uint32_t *out_crops, hipStream_t stream, uint32_t *d_out_crops)
{
    const HashJob all{d_frames, n_clips, w, h, frame_stride, clip_stride, d_out, d_dc, stream};
    return checked_launches(ctx, all, frames_per_clip, [&](size_t c0, size_t n) {
        return letterbox_launch(ctx, all.clips(c0, n), frames_per_clip, out_crops ? out_crops + 4 * c0 : nullptr, d_out_crops ? d_out_crops + 4 * c0 : nullptr);
    });
}

// ---- letterbox detection on clips of different frame sizes (include/vdf.h: vdf_cropdetect_letterbox_clips_device, vdf_hash_clips_u8_letterbox[_device]) ----
// The checks of both calls, in the order their codes are reported; *plan is valid when VDF_OK comes back and n_clips != 0.
static int letterbox_clips_plan(vdf_ctx *ctx, const void *d_buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips, uint32_t frames_per_clip, const void *out,
                                vdf::LetterboxMixedPlan *plan)
{
    if (n_clips && !clips) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (n_clips > 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "more than 2^32 - 1 clips in one call");
    const vdf::MixedClip *mc = reinterpret_cast<const vdf::MixedClip *>(clips);
    const vdf::MixedCheck chk = vdf::check_mixed(mc, n_clips, frames_per_clip, buf_bytes);
    if (chk.error != vdf::MixedError::kNone) return mixed_check_failed(ctx, chk);
    *plan = vdf::plan_letterbox_mixed(mc, n_clips, hash_knobs(ctx));
    if (plan->kind == vdf::LetterboxMixedPlan::kCropGiven) return mixed_check_failed(ctx, vdf::MixedCheck{vdf::MixedError::kCropGiven, plan->bad_clip});
    if (n_clips && (!d_buf || !out)) return fail(ctx, VDF_E_INVAL, "null pointer");
    return VDF_OK;
}

// The detect passes of a kMixed plan: descriptors through the pinned staging in one upload, then the plan's launches.  The staging is free
// again when this returns (the upload has run; the kernels stay queued).
static int letterbox_clips_detect(vdf_ctx *ctx, const uint8_t *d_buf, const vdf::LetterboxMixedPlan &plan, size_t n_clips, uint32_t *d_crops, hipStream_t stream)
{
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nd = plan.descs.size() * sizeof(vdf::LetterboxProbeDesc);
    if (plan.descs.size() != n_clips) return fail(ctx, VDF_E_INVAL, "letterbox plan does not cover the call");  // (cannot happen: one descriptor per clip)
    if (!ctx->pin_desc.reserve(nd)) return fail(ctx, VDF_E_OOM, "host staging for the clip descriptors");
    std::memcpy(ctx->pin_desc.p, plan.descs.data(), nd);
    if (int rc = upload(ctx, ctx->crop_desc, ctx->pin_desc.p, nd, stream)) return rc;
    VDF_HIP(ctx, hipEventRecord(ctx->ev_mid, stream));
    VDF_HIP(ctx, ctx->crop_work.reserve(plan.work_bytes));
    const hipError_t e = vdf::launch_letterbox_mixed(d_buf, ctx->crop_desc.as<vdf::LetterboxProbeDesc>(), plan.launches.data(), plan.launches.size(), n_clips, d_crops,
                                                     ctx->crop_work.as<uint32_t>(), stream);
    const hipError_t ew = hipEventSynchronize(ctx->ev_mid);
    if (e != hipSuccess) return fail_hip(ctx, e, "mixed letterbox launch");
    VDF_HIP(ctx, ew);
    return VDF_OK;
}

int cropdetect_clips_locked(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips, uint32_t frames_per_clip,
                            uint32_t *d_crops, hipStream_t stream)
{
    vdf::LetterboxMixedPlan plan;
    if (int rc = letterbox_clips_plan(ctx, d_buf, buf_bytes, clips, n_clips, frames_per_clip, d_crops, &plan)) return rc;
    if (n_clips == 0) return VDF_OK;
    if (plan.kind == vdf::LetterboxMixedPlan::kUniform) {  // one size, evenly spaced: exactly vdf_cropdetect_letterbox_device
        VDF_HIP(ctx, hipSetDevice(ctx->device));
        const uint8_t *base = d_buf + plan.offset0;
        VDF_HIP(ctx, ctx->crop_work.reserve(vdf::letterbox_work_bytes(std::min(kMaxClipsPerLaunch, n_clips), frames_per_clip)));
        for (size_t c0 = 0; c0 < n_clips; c0 += kMaxClipsPerLaunch)
            VDF_HIP(ctx, vdf::launch_letterbox(base + c0 * plan.clip_stride, std::min(kMaxClipsPerLaunch, n_clips - c0), frames_per_clip, clips[0].w, clips[0].h,
                                               (size_t)clips[0].frame_stride, (size_t)plan.clip_stride, d_crops + 4 * c0, ctx->crop_work.as<uint32_t>(), stream,
                                               ctx->lb_side_strips));
        return VDF_OK;
    }
    return letterbox_clips_detect(ctx, d_buf, plan, n_clips, d_crops, stream);
}

// detect, boxes down (the call waits for its detect, as the uniform call does for large frames), then the mixed hash call on the detected boxes
int letterbox_clips_locked(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips, uint32_t frames_per_clip,
                           uint64_t *d_out, uint32_t *d_dc, uint32_t *out_crops, hipStream_t stream)
{
    vdf::LetterboxMixedPlan plan;
    if (int rc = letterbox_clips_plan(ctx, d_buf, buf_bytes, clips, n_clips, frames_per_clip, d_out, &plan)) return rc;
    if (n_clips == 0) return VDF_OK;
    if (plan.kind == vdf::LetterboxMixedPlan::kUniform)  // exactly vdf_hash_frames_u8_letterbox_device
        return letterbox_hash_device_locked(ctx, d_buf + plan.offset0, n_clips, frames_per_clip, clips[0].w, clips[0].h, (size_t)clips[0].frame_stride,
                                            (size_t)plan.clip_stride, d_out, d_dc, out_crops, stream);
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    VDF_HIP(ctx, ctx->crops.reserve(n_clips * 16));
    uint32_t *d_crops = ctx->crops.as<uint32_t>();
    if (int rc = letterbox_clips_detect(ctx, d_buf, plan, n_clips, d_crops, stream)) return rc;
    if (!ctx->pin_crops.reserve(n_clips * 16)) return fail(ctx, VDF_E_OOM, "host staging for the crop boxes");
    const uint32_t *crops = ctx->pin_crops.as<uint32_t>();
    VDF_HIP(ctx, hipMemcpyAsync(ctx->pin_crops.p, d_crops, n_clips * 16, hipMemcpyDeviceToHost, stream));
    VDF_HIP(ctx, hipEventRecord(ctx->ev_wait, stream));
    if (int rcw = wait_event(ctx, ctx->ev_wait)) return rcw;
    if (out_crops) std::memcpy(out_crops, crops, n_clips * 16);
    std::vector<vdf_clip> boxed(clips, clips + n_clips);
    for (size_t i = 0; i < n_clips; i++) {
        boxed[i].crop_left = crops[4 * i]; boxed[i].crop_right = crops[4 * i + 1];
        boxed[i].crop_top = crops[4 * i + 2]; boxed[i].crop_bottom = crops[4 * i + 3];
    }
    // check_mixed + plan_mixed + hash_mixed_launch, unchanged: a detected box that leaves no pixels or a box size without an i8 table is reported here,
    // after the detect, and no hash is written
    return hash_clips_locked(ctx, d_buf, buf_bytes, boxed.data(), n_clips, frames_per_clip, d_out, d_dc, stream);
}


int search_refs_device_locked(vdf_ctx *ctx, const uint64_t *d_cand_hashes, const uint32_t *d_cand_durations,
                                     size_t n_cand, const uint64_t *d_ref_hashes, const uint32_t *d_ref_durations,
                                     size_t n_ref, uint32_t tol_int, uint32_t ref_index_base, vdf_hit *hits,
                                     uint64_t capacity, uint64_t *n_hits, hipStream_t s, vdf_ctx::HostHits *staging)
{
    ctx->stats = vdf_search_stats{};
    ctx->timing = vdf_search_timing{};
    *n_hits = 0;
    if (n_ref == 0 || n_cand == 0) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    // References arrive in the caller's order; tiles want neighbouring rows to share a duration window, so
    // rows are visited through a stable duration-sorted permutation (reported indices stay the caller's).
    // (stable, on the device: the durations never leave HBM and nothing here waits for the GPU)
    const size_t sbytes = vdf::sort_order_scratch_bytes((uint32_t)n_ref, false);
    VDF_HIP(ctx, ctx->sort_scratch.reserve(sbytes));
    VDF_HIP(ctx, ctx->perm.reserve(std::max<size_t>(n_ref * 4, 16)));
    VDF_HIP(ctx, vdf::launch_sort_order(d_ref_durations, nullptr, (uint32_t)n_ref, ctx->perm.as<uint32_t>(), ctx->sort_scratch.p,
                                        ctx->sort_scratch.cap, s));
    int rc = VDF_OK;
    // Every hit is part of the output here (consume = false).  The hit buffer is the caller's to size (VDF_E_OVERFLOW with the
    // required size); the suspect queue of the matrix-core backend is the library's: if a launch dropped suspects, run it
    // again with a larger queue.
    for (int attempt = 0;; attempt++) {
        uint32_t overflow_row = 0;
        ctx->stats = vdf_search_stats{};
        rc = search_core(ctx, 1, d_cand_hashes, d_cand_durations, n_cand, d_ref_hashes, d_ref_durations,
                         ctx->perm.as<uint32_t>(), n_ref, tol_int, 0, 1, 0, 0xFFFFFFFFu, nullptr, ref_index_base, hits,
                         capacity, n_hits, &overflow_row, s, false, staging);
        if (rc) { ctx->cand_scale = 1; return rc; }
        if (*n_hits > capacity) { ctx->cand_scale = 1; return fail(ctx, VDF_E_OVERFLOW, "hit buffer too small; *n_hits holds the required size"); }
        if (overflow_row == 0xFFFFFFFFu) break;  // complete
        if (attempt >= 12) { ctx->cand_scale = 1; return fail(ctx, VDF_E_OVERFLOW, "suspect queue overflow"); }
        ctx->cand_scale *= 4;
    }
    ctx->cand_scale = 1;
    return VDF_OK;
}

int create_single(int device_id, vdf_ctx **out, std::string *err)
{
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        *err = std::string("no usable HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count = 0");
        (void)hipGetLastError();
        return VDF_E_HIP;
    }
    if (device_id < 0 || device_id >= count) { *err = "device id out of range"; return VDF_E_INVAL; }
    vdf_ctx *ctx = new (std::nothrow) vdf_ctx();
    if (!ctx) return VDF_E_OOM;
    ctx->device = device_id;
    ctx->spin_wait = std::getenv("VDF_SPIN_WAIT") != nullptr;
    ctx->no_link_turns = std::getenv("VDF_NO_LINK_TURNS") != nullptr;
    const unsigned wait_flags = hipEventDisableTiming | (ctx->spin_wait ? 0u : (unsigned)hipEventBlockingSync);
    bool ok = hipSetDevice(device_id) == hipSuccess &&
              hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreate(&ctx->ev0) == hipSuccess && hipEventCreate(&ctx->ev1) == hipSuccess &&
              hipEventCreate(&ctx->ev_mid) == hipSuccess && hipEventCreateWithFlags(&ctx->ev_wait, wait_flags) == hipSuccess;
    for (int i = 0; ok && i < 2; i++)
        ok = hipEventCreateWithFlags(&ctx->ev_copy[i], wait_flags) == hipSuccess &&
             hipEventCreateWithFlags(&ctx->ev_done[i], wait_flags) == hipSuccess;
    if (!ok) {
        *err = std::string("context setup failed: ") + hipGetErrorString(hipGetLastError());
        delete ctx;
        return VDF_E_HIP;
    }
    if (const char *s = std::getenv("VDF_ROWS_PER_LANE")) {
        int r = std::atoi(s);
        if (r == 1 || r == 2 || r == 4) ctx->tile_rows = 256u * (uint32_t)r;
    }
    if (const char *s = std::getenv("VDF_RESIZE_MODE")) {
        int m = std::atoi(s);
        if (m >= 0 && m <= 6 && m != 2) ctx->resize_mode = m;  // 2 was the per-frame 16 x 64 B kernel, removed in round 3
    }
    if (const char *s = std::getenv("VDF_SEARCH_BACKEND")) {
        if (!std::strcmp(s, "valu")) ctx->search_backend = 0;
        else if (!std::strcmp(s, "mfma")) ctx->search_backend = 1;
    }
    if (const char *s = std::getenv("VDF_MFMA_CHUNK_COLS")) {
        long c = std::atol(s);
        if (c >= 32 && c <= (1 << 22)) ctx->mfma_chunk_cols = (uint32_t)c;
    }
    if (const char *s = std::getenv("VDF_CAND_CAPACITY")) { const long v = std::atol(s); if (v >= 8 && v <= 0x40000000l) ctx->cand_capacity_override = (uint32_t)v; }
    if (const char *s = std::getenv("VDF_MFMA_SELF_ROWS")) { const int v = std::atoi(s); if (v == 256 || v == 512) ctx->mfma_self_rows = (uint32_t)v; }
    if (const char *s = std::getenv("VDF_MFMA_REFS_ROWS")) { const int v = std::atoi(s); if (v == 256 || v == 512) ctx->mfma_refs_rows = (uint32_t)v; }
    if (const char *s = std::getenv("VDF_MFMA_PRUNE_STEP")) ctx->mfma_prune_step = std::atoi(s);
    if (const char *s = std::getenv("VDF_MFMA_MIN_WGS")) { const long v = std::atol(s); if (v >= 1 && v <= (1 << 24)) ctx->mfma_min_wgs = (uint32_t)v; }
    if (const char *s = std::getenv("VDF_MFMA_GROUP")) {
        long c = std::atol(s);
        if (c >= 1 && c <= (1 << 20)) ctx->mfma_group = (uint32_t)c;
    }
    if (const char *s = std::getenv("VDF_NO_HIT_FILTER")) ctx->no_hit_filter = std::atoi(s) != 0;
    if (std::getenv("VDF_NO_WAVESTREAM")) ctx->wavestream_knob = -1;
    else if (const char *s = std::getenv("VDF_WAVESTREAM_NW")) { const int v = std::atoi(s); if (v >= 3 && v <= 8) ctx->wavestream_knob = v; }
    ctx->no_rowcrop = std::getenv("VDF_NO_ROWCROP") != nullptr;
    ctx->rowcrop_all = std::getenv("VDF_ROWCROP_ALL") != nullptr;
    ctx->no_boxstream = std::getenv("VDF_NO_BOXSTREAM") != nullptr;
    ctx->no_smallcrop = std::getenv("VDF_NO_SMALLCROP") != nullptr;
    ctx->no_device_path_order = std::getenv("VDF_NO_DEVICE_PATH_ORDER") != nullptr;
    ctx->lb_host_plan = std::getenv("VDF_LB_HOST_PLAN") != nullptr;
    ctx->no_lb_fused = std::getenv("VDF_NO_LB_FUSED") != nullptr;
    if (std::getenv("VDF_LB_NC16")) ctx->lb_side_strips = 16;
    if (const char *s = std::getenv("VDF_COPY_THREADS")) { const int v = std::atoi(s); if (v >= 1 && v <= 64) ctx->copy_threads = v; }
    if (const char *s = std::getenv("VDF_HOST_CHUNK_MB")) { const long v = std::atol(s); if (v >= 1 && v <= 1024) ctx->host_chunk_bytes = (size_t)v << 20; }
    if (const char *s = std::getenv("VDF_HOST_DIRECT")) ctx->host_direct = std::atoi(s) != 0;
    if (const char *s = std::getenv("VDF_HASH_NO_PERSISTENT")) ctx->hash_no_persistent = std::atoi(s) != 0;
    if (const char *s = std::getenv("VDF_HASH_WGS_PER_CU")) {
        int v = std::atoi(s);
        if (v >= 1 && v <= 8) { ctx->hash_wgs_per_cu = v; ctx->hash_wgs_per_cu_set = true; }
    }
    if (const char *s = std::getenv("VDF_CHUNK_COLS")) {
        long c = std::atol(s);
        if (c >= 64 && c <= (1 << 20)) ctx->chunk_cols = (uint32_t)c;
    }
    *out = ctx;
    return VDF_OK;
}

// search() over a sorted database that is already resident on EVERY device of the context (each device's
// up_hashes / up_dur): row tiles are dealt round-robin over the devices (tile t -> device t % G), every device emits
// the thresholded pairs of its tiles, the host merges them and replays search_self's consumption ONCE
// (search_algorithm.rs:131-170) -> the same MatchGroups for every G.  Hit-buffer overflow: rows below the smallest
// row that lost a hit on any device are complete and are replayed; the consumption bitmap goes back to every device and
// the search resumes from that row.
int search_self_resident(vdf_ctx *ctx, size_t n, uint32_t tol_int, vdf_groups *out)
{
    const int G = device_count(ctx);
    uint64_t capacity = ctx->hit_capacity;
    std::vector<uint8_t> matched(n, 0);
    std::vector<uint32_t> bitmap;  // 1 bit per entry, built on the first overflow, then updated with the new members only
    bool use_bitmap = false;
    std::vector<vdf_hit> merged;
    uint32_t row_begin = 0;
    uint64_t span = n;  // rows per launch; shrinks after an overflow, grows back afterwards
    ctx->stats = vdf_search_stats{};
    const double t_call = now_ms();
    double replay_ms = 0.0;
    for (int k = 0; k < G; k++) { device_ctx(ctx, k)->stats = vdf_search_stats{}; device_ctx(ctx, k)->timing = vdf_search_timing{}; }
    while (row_begin < n) {
        const uint32_t row_end = (uint32_t)std::min<uint64_t>((uint64_t)row_begin + span, n);
        // the hits feed the replay and nothing else: rows that cannot become targets are dropped on the devices, which meet for
        // that through the context's own exchange when there are several (multi.cpp: LocalExchange)
        std::unique_ptr<ShardExchange> fx(make_local_exchange(ctx));
        int rc = for_each_device(ctx, [&](int k, vdf_ctx *d) {
            const int r = search_core(d, 0, d->up_hashes.as<uint64_t>(), d->up_dur.as<uint32_t>(), n, d->up_hashes.as<uint64_t>(),
                                      d->up_dur.as<uint32_t>(), nullptr, n, tol_int, (uint32_t)k, (uint32_t)G, row_begin, row_end,
                                      use_bitmap ? d->matched.as<uint32_t>() : nullptr, 0, nullptr, capacity,
                                      &d->r_n_hits, &d->r_overflow, d->stream, /*replay_only=*/true, &d->host_hits, fx.get());
            if (r && fx && !d->err_secondary) fx->abort(r, "device " + std::to_string(d->device) + ": " + d->err);  // the other devices must not wait for this one at the filter's meeting points
            return r;
        });
        if (rc) { vdf_groups_free(out); return rc; }
        uint32_t overflow_row = 0xFFFFFFFFu;
        for (int k = 0; k < G; k++) overflow_row = std::min(overflow_row, device_ctx(ctx, k)->r_overflow);
        const uint32_t complete_end = std::min(overflow_row, row_end);
        const vdf_hit *hp;
        uint64_t nh;
        if (G == 1) {
            hp = device_ctx(ctx, 0)->host_hits.data();
            nh = std::min(device_ctx(ctx, 0)->r_n_hits, capacity);
        } else {  // every device's list is sorted by (row, col) and the devices own disjoint rows
            merged.clear();
            for (int k = 0; k < G; k++) {
                const vdf_ctx *d = device_ctx(ctx, k);
                const vdf_hit *b = d->host_hits.data(), *e = b + std::min(d->r_n_hits, capacity);
                e = std::lower_bound(b, e, vdf_hit{complete_end, 0u}, hit_less);  // rows >= complete_end are searched again
                const size_t mid = merged.size();
                merged.insert(merged.end(), b, e);
                std::inplace_merge(merged.begin(), merged.begin() + (ptrdiff_t)mid, merged.end(), hit_less);
            }
            hp = merged.data();
            nh = merged.size();
        }
        const uint64_t old_members = out->n_groups ? out->offsets[out->n_groups] : 0;
        const double t_replay = now_ms();
        rc = vdf_replay_self(n, hp, nh, row_begin, complete_end, matched.data(), out);
        replay_ms += now_ms() - t_replay;
        if (rc) { vdf_groups_free(out); return fail(ctx, rc, "replay failed"); }
        if (overflow_row == 0xFFFFFFFFu) {
            row_begin = row_end;
            span = std::min<uint64_t>(n, span * 4);
        } else {
            const uint64_t progress = complete_end - row_begin;
            if (progress == 0) {
                // Not even one row fit: give a single row the whole buffer (its hits are < n), and a larger suspect queue
                // (a row of a dense cluster has as many suspects as the cluster has members).
                span = 1;
                if (capacity < n) capacity = n;
                for (int k = 0; k < G; k++) device_ctx(ctx, k)->cand_scale = std::min<uint64_t>(device_ctx(ctx, k)->cand_scale * 4, 1ull << 24);
            } else {
                span = std::max<uint64_t>(progress * 2, device_ctx(ctx, 0)->tile_rows);
            }
            row_begin = complete_end;
        }
        if (row_begin < n) {  // feed the consumption state back to the devices
            if (!use_bitmap) {
                bitmap.assign((n + 31) / 32, 0u);
                for (size_t i = 0; i < n; i++)
                    if (matched[i]) bitmap[i >> 5] |= 1u << (i & 31);
                use_bitmap = true;
            } else {  // entries consumed by this round = the members of the groups it appended
                const uint64_t new_members = out->n_groups ? out->offsets[out->n_groups] : 0;
                for (uint64_t q = old_members; q < new_members; q++) {
                    const uint64_t i = out->members[q];
                    bitmap[i >> 5] |= 1u << (i & 31);
                }
            }
            rc = for_each_device(ctx, [&](int, vdf_ctx *d) {
                int r = upload(d, d->matched, bitmap.data(), bitmap.size() * 4, d->stream);
                if (r) return r;
                VDF_HIP(d, hipStreamSynchronize(d->stream));  // `bitmap` is rewritten by the next round
                return (int)VDF_OK;
            });
            if (rc) { vdf_groups_free(out); return rc; }
        }
    }
    // statistics: sums over the devices; kernel time = the slowest device's
    ctx->dev_stats.assign((size_t)G, vdf_search_stats{});
    vdf_search_stats agg{};
    for (int k = 0; k < G; k++) {
        device_ctx(ctx, k)->cand_scale = 1;
        const vdf_search_stats &st = device_ctx(ctx, k)->stats;
        ctx->dev_stats[(size_t)k] = st;
        agg.pairs += st.pairs; agg.pairs_computed += st.pairs_computed; agg.n_hits += st.n_hits; agg.n_tiles += st.n_tiles;
        agg.pairs_early_exit += st.pairs_early_exit;
        agg.n_launches = std::max(agg.n_launches, st.n_launches);
        agg.kernel_ms = std::max(agg.kernel_ms, st.kernel_ms);
        agg.early_exit_bits = st.early_exit_bits;
    }
    ctx->stats = agg;
    const double t_fin = now_ms();
    const int rc_fin = vdf_groups_finish_self(out);
    vdf_search_timing tm{};
    for (int k = 0; k < G; k++) {  // device figures: the slowest device's
        const vdf_search_timing &q = device_ctx(ctx, k)->timing;
        tm.prep_ms = std::max(tm.prep_ms, q.prep_ms); tm.stream_ms = std::max(tm.stream_ms, q.stream_ms);
        tm.resolve_ms = std::max(tm.resolve_ms, q.resolve_ms); tm.download_ms = std::max(tm.download_ms, q.download_ms);
        tm.suspects += q.suspects; tm.suspect_capacity = std::max(tm.suspect_capacity, q.suspect_capacity);
        tm.hits_filtered += q.hits_filtered;
    }
    tm.replay_ms = (float)(replay_ms + now_ms() - t_fin);
    tm.total_ms = (float)(now_ms() - t_call);
    ctx->timing = tm;
    ctx->dev_timing.assign((size_t)G, vdf_search_timing{});
    for (int k = 0; k < G; k++) ctx->dev_timing[(size_t)k] = device_ctx(ctx, k)->timing;
    return rc_fin;
}

// search_with_references() with the sorted candidates resident on every device (up_hashes / up_dur) and device k holding
// the references [ref_base[k], ref_base[k] + ref_cnt[k]) of the caller's order in up_ref_hashes / up_ref_dur: every
// device searches its slice; per-device hit lists concatenate in device order = reference input order.
int search_refs_resident(vdf_ctx *ctx, size_t n_cand, const std::vector<size_t> &ref_cnt, const std::vector<size_t> &ref_base,
                         uint32_t tol_int, vdf_groups *out)
{
    const int G = device_count(ctx);
    const uint64_t capacity0 = ctx->hit_capacity;
    const double t_call = now_ms();
    int rc = for_each_device(ctx, [&](int k, vdf_ctx *d) {
        d->r_n_hits = 0;
        d->stats = vdf_search_stats{};
        d->timing = vdf_search_timing{};
        if (ref_cnt[(size_t)k] == 0) return (int)VDF_OK;
        uint64_t capacity = capacity0;
        for (int attempt = 0; attempt < 6; attempt++) {
            int r = search_refs_device_locked(d, d->up_hashes.as<uint64_t>(), d->up_dur.as<uint32_t>(), n_cand,
                                              d->up_ref_hashes.as<uint64_t>(), d->up_ref_dur.as<uint32_t>(),
                                              ref_cnt[(size_t)k], tol_int, (uint32_t)ref_base[(size_t)k], nullptr,
                                              capacity, &d->r_n_hits, d->stream, &d->host_hits);
            if (r == VDF_E_OVERFLOW && d->r_n_hits > capacity) { capacity = d->r_n_hits; continue; }  // every hit is output: size up
            return r;
        }
        return (int)VDF_E_OVERFLOW;
    });
    if (rc) return rc;
    ctx->dev_stats.assign((size_t)G, vdf_search_stats{});
    vdf_search_stats agg{};
    for (int k = 0; k < G; k++) {
        const vdf_search_stats &st = device_ctx(ctx, k)->stats;
        ctx->dev_stats[(size_t)k] = st;
        agg.pairs += st.pairs; agg.pairs_computed += st.pairs_computed; agg.n_hits += st.n_hits; agg.n_tiles += st.n_tiles;
        agg.pairs_early_exit += st.pairs_early_exit;
        agg.n_launches = std::max(agg.n_launches, st.n_launches);
        agg.kernel_ms = std::max(agg.kernel_ms, st.kernel_ms);
        agg.early_exit_bits = st.early_exit_bits;
    }
    ctx->stats = agg;
    vdf_search_timing tm{};
    for (int k = 0; k < G; k++) {
        const vdf_search_timing &q = device_ctx(ctx, k)->timing;
        tm.prep_ms = std::max(tm.prep_ms, q.prep_ms); tm.stream_ms = std::max(tm.stream_ms, q.stream_ms);
        tm.resolve_ms = std::max(tm.resolve_ms, q.resolve_ms); tm.download_ms = std::max(tm.download_ms, q.download_ms);
        tm.suspects += q.suspects; tm.suspect_capacity = std::max(tm.suspect_capacity, q.suspect_capacity);
        tm.hits_filtered += q.hits_filtered;
    }
    ctx->dev_timing.assign((size_t)G, vdf_search_timing{});
    for (int k = 0; k < G; k++) ctx->dev_timing[(size_t)k] = device_ctx(ctx, k)->timing;
    const double t_group = now_ms();
    int rcg;
    if (G == 1) {
        rcg = vdf_groups_from_ref_hits(device_ctx(ctx, 0)->host_hits.data(), device_ctx(ctx, 0)->r_n_hits, out);
    } else {
        std::vector<vdf_hit> all;
        for (int k = 0; k < G; k++) {
            const vdf_ctx *d = device_ctx(ctx, k);
            all.insert(all.end(), d->host_hits.data(), d->host_hits.data() + d->r_n_hits);
        }
        rcg = vdf_groups_from_ref_hits(all.data(), all.size(), out);
    }
    tm.replay_ms = (float)(now_ms() - t_group);
    tm.total_ms = (float)(now_ms() - t_call);
    ctx->timing = tm;
    return rcg;
}

// ---- alignment of videos on their window hashes (include/vdf.h: vdf_align_windows[_device|_host]) -------------------------------
// the argument checks all three forms share, in the order their messages are reported; first arrays on the host (null: not checked here)
int align_checks(vdf_ctx *ctx, const void *a_hashes, const uint32_t *a_first, size_t n_a, const void *b_hashes, const uint32_t *b_first, size_t n_b,
                 const void *a_first_ptr, const void *b_first_ptr, uint32_t min_run, const void *out, size_t capacity, const size_t *n_out,
                 const size_t *n_listed = nullptr,  // the *_pairs forms: the limit is on the LISTED pairs, not on n_a x n_b
                 const char *listed_what = "pairs")  // ... or "triples" (vdf_align_windows_variants_pairs*)
{
    const bool self = b_hashes == nullptr;
    if (!n_out || (n_a && (!a_hashes || !a_first_ptr)) || (!self && n_b && !b_first_ptr) || (capacity && !out)) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (min_run == 0) return fail(ctx, VDF_E_INVAL, "min_run of zero");
    const uint32_t *firsts[2] = {a_first, self ? nullptr : b_first};
    const size_t counts[2] = {n_a, n_b};
    for (int side = 0; side < 2; side++)
        for (size_t v = 0; firsts[side] && v < counts[side]; v++)
            if (firsts[side][v + 1] >= firsts[side][v] && firsts[side][v + 1] - firsts[side][v] > vdf::kAlignMaxWindows)
                return fail(ctx, VDF_E_INVAL, std::string("video ") + std::to_string(v) + (side ? " of B" : " of A") + " has more than 2^20 windows");
    for (int side = 0; side < 2; side++)
        for (size_t v = 0; firsts[side] && v < counts[side]; v++)
            if (firsts[side][v + 1] < firsts[side][v])
                return fail(ctx, VDF_E_INVAL, std::string("the first array") + (side ? " of B" : " of A") + " decreases at video " + std::to_string(v));
    if (n_listed) {
        if (n_a > 0xFFFFFFFFull || n_b > 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "more than 2^32 - 1 videos on one side: a video index does not fit 32 bits");
        if (*n_listed > vdf::kAlignMaxPairs) return fail(ctx, VDF_E_INVAL, std::string("more than 2^24 listed ") + listed_what + " in one call");
        return VDF_OK;
    }
    if (n_a > 0xFFFFFFFFull || n_b > 0xFFFFFFFFull || vdf::align_pair_count(n_a, self ? n_a : n_b, self) > vdf::kAlignMaxPairs)
        return fail(ctx, VDF_E_INVAL, "more than 2^24 pairs of videos in one call");
    return VDF_OK;
}

// the literal definition: every diagonal of the pair walked, XOR + popcount; *best.n_windows = 0: no competing run
// rects (nullable): the cells of these n_rects rectangles are misses (vdf_align_windows_stretches*: the ranks before this one)
void align_pair_host(const uint64_t *A, uint32_t Na, const uint8_t *skip_a, const uint64_t *B, uint32_t Nb, const uint8_t *skip_b, uint32_t tol,
                     uint32_t min_run, vdf_alignment *best, const vdf::AlignRect *rects = nullptr, uint32_t n_rects = 0)
{
    uint32_t best_score = 0;
    best->offset = 0; best->start_a = 0; best->n_windows = 0; best->dist_sum = 0;
    for (int64_t d = -((int64_t)Na - 1); d <= (int64_t)Nb - 1; d++) {
        const int64_t ka0 = std::max<int64_t>(0, -d), ka1 = std::min<int64_t>(Na, (int64_t)Nb - d);
        uint32_t len = 0, sum = 0;
        for (int64_t ka = ka0; ka <= ka1; ka++) {  // ka1: the cell behind the diagonal's last, a miss
            bool match = false;
            uint32_t dist = 0;
            if (ka < ka1 && !(skip_a && skip_a[ka]) && !(skip_b && skip_b[ka + d]) && !vdf::align_cell_masked(rects, n_rects, (uint32_t)ka, (uint32_t)(ka + d))) {
                const uint64_t *x = A + 16 * ka, *y = B + 16 * (ka + d);
                for (int w = 0; w < VDF_HASH_WORDS; w++) dist += (uint32_t)__builtin_popcountll(x[w] ^ y[w]);
                match = dist <= tol;
            }
            if (match) { len++; sum += dist; continue; }
            if (len >= min_run) {
                const uint32_t score = len * (tol + 1) - sum, start = (uint32_t)(ka - len);
                if (vdf::align_better(score, (int32_t)d, start, best_score, best->offset, best->start_a)) {
                    best_score = score; best->offset = (int32_t)d; best->start_a = start; best->n_windows = len; best->dist_sum = sum;
                }
            }
            len = 0; sum = 0;
        }
    }
}

// align_checks has passed on h_first_a / h_first_b (host copies of the device arrays); every array pointer is a device pointer
int align_locked(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, const uint32_t *h_first_a, size_t n_a, const uint8_t *d_a_skip,
                 const uint64_t *d_b_hashes, const uint32_t *d_b_first, const uint32_t *h_first_b, size_t n_b, const uint8_t *d_b_skip, bool self,
                 uint32_t tol_int, uint32_t min_run, vdf_alignment *out, size_t capacity, size_t *n_out, hipStream_t s,
                 const vdf_video_pair *list = nullptr, size_t n_list = 0)  // list: only these pairs (checked: align_pair_list_check), not all of them
{
    vdf::AlignCursor cur;
    vdf::AlignChunk ch;
    size_t found = 0, list_at = 0;
    while (list ? vdf::align_next_chunk_pairs(h_first_a, h_first_b, list, n_list, list_at, ch) : vdf::align_next_chunk(h_first_a, n_a, h_first_b, n_b, self, cur, ch)) {
        const size_t n_pairs = ch.pairs.size(), n_units = ch.n_units();
        const size_t pair_bytes = n_pairs * sizeof(vdf::AlignPair), off_bytes = (n_pairs + 1) * sizeof(uint32_t);
        VDF_HIP(ctx, ctx->align_plan.reserve(pair_bytes + off_bytes));
        VDF_HIP(ctx, ctx->align_scratch.reserve(vdf::align_scratch_bytes(n_pairs, n_units)));
        char *plan = ctx->align_plan.as<char>();
        VDF_HIP(ctx, hipMemcpyAsync(plan, ch.pairs.data(), pair_bytes, hipMemcpyHostToDevice, s));
        VDF_HIP(ctx, hipMemcpyAsync(plan + pair_bytes, ch.unit_offset.data(), off_bytes, hipMemcpyHostToDevice, s));
        vdf_alignment *d_dense = nullptr;
        uint32_t *d_total = nullptr;
        vdf::AlignLaunch L{};
        L.a_hashes = reinterpret_cast<const uint32_t *>(d_a_hashes); L.a_first = d_a_first; L.a_skip = d_a_skip;
        L.b_hashes = reinterpret_cast<const uint32_t *>(d_b_hashes); L.b_first = d_b_first; L.b_skip = d_b_skip;
        L.pairs = reinterpret_cast<const vdf::AlignPair *>(plan);
        L.unit_offset = reinterpret_cast<const uint32_t *>(plan + pair_bytes);
        L.n_pairs = (uint32_t)n_pairs; L.n_units = (uint32_t)n_units;
        L.tol = std::min<uint32_t>(tol_int, 1024u); L.min_run = min_run;
        L.scratch = ctx->align_scratch.p; L.dense_out = &d_dense; L.total_out = &d_total;
        VDF_HIP(ctx, vdf::launch_align_chunk(L, s));
        uint32_t total = 0;
        VDF_HIP(ctx, hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, s));
        VDF_HIP(ctx, hipStreamSynchronize(s));  // also: the chunk's plan arrays are free to change
        const size_t room = capacity > found ? capacity - found : 0, take = std::min<size_t>(total, room);
        if (take) {
            VDF_HIP(ctx, hipMemcpyAsync(out + found, d_dense, take * sizeof(vdf_alignment), hipMemcpyDeviceToHost, s));
            VDF_HIP(ctx, hipStreamSynchronize(s));
        }
        found += total;
    }
    *n_out = found;
    return VDF_OK;
}

// ---- more than one stretch per pair (include/vdf.h: vdf_align_windows_stretches[_device|_host]) ----------------------------------
// behind align_checks: max_stretches, then guard
int align_stretches_checks(vdf_ctx *ctx, uint32_t max_stretches, uint32_t guard)
{
    if (max_stretches < 1 || max_stretches > vdf::kAlignMaxStretches) return fail(ctx, VDF_E_INVAL, "max_stretches outside 1 ... 8");
    if (guard > vdf::kAlignMaxGuard) return fail(ctx, VDF_E_INVAL, "guard above 2^20 windows");
    return VDF_OK;
}

vdf_alignment_stretch stretch_of(const vdf_alignment &r, uint32_t rank)
{
    return vdf_alignment_stretch{r.a, r.b, r.offset, r.start_a, r.n_windows, r.dist_sum, rank};
}

// the rounds' record lists of one chunk (each in (a, b) order, the pairs of round r a subset of those of round r - 1) -> (a, b, rank) order
template <class Emit> void align_merge_rounds(const std::vector<std::vector<vdf_alignment>> &rounds, Emit emit)
{
    if (rounds.empty()) return;
    std::vector<size_t> at(rounds.size(), 0);
    for (const vdf_alignment &r0 : rounds[0]) {
        emit(stretch_of(r0, 0));
        for (size_t r = 1; r < rounds.size(); r++) {
            if (at[r] == rounds[r].size() || rounds[r][at[r]].a != r0.a || rounds[r][at[r]].b != r0.b) break;
            emit(stretch_of(rounds[r][at[r]++], (uint32_t)r));
        }
    }
}

struct AlignSides {  // device pointers, and the first arrays on the host as well
    const uint64_t *d_a_hashes; const uint32_t *d_a_first, *h_first_a; size_t n_a; const uint8_t *d_a_skip;
    const uint64_t *d_b_hashes; const uint32_t *d_b_first, *h_first_b; size_t n_b; const uint8_t *d_b_skip;
    bool self;
};

// one round of a chunk: plan up, the band kernel (masked from round 1 on) and the reductions, the dense records down into recs
static int align_run_round(vdf_ctx *ctx, const AlignSides &in, const vdf::AlignRound &round, uint32_t tol, uint32_t min_run, std::vector<vdf_alignment> &recs,
                           hipStream_t s)
{
    const size_t n_pairs = round.pairs.size(), n_units = round.n_units();
    const size_t pair_bytes = n_pairs * sizeof(vdf::AlignPair), off_bytes = (n_pairs + 1) * sizeof(uint32_t);
    const size_t rect_at = (pair_bytes + off_bytes + 15) & ~(size_t)15, rect_bytes = round.rects.size() * sizeof(vdf::AlignRect);
    VDF_HIP(ctx, ctx->align_plan.reserve(rect_at + rect_bytes));
    VDF_HIP(ctx, ctx->align_scratch.reserve(vdf::align_scratch_bytes(n_pairs, n_units)));
    char *plan = ctx->align_plan.as<char>();
    VDF_HIP(ctx, hipMemcpyAsync(plan, round.pairs.data(), pair_bytes, hipMemcpyHostToDevice, s));
    VDF_HIP(ctx, hipMemcpyAsync(plan + pair_bytes, round.unit_offset.data(), off_bytes, hipMemcpyHostToDevice, s));
    if (rect_bytes) VDF_HIP(ctx, hipMemcpyAsync(plan + rect_at, round.rects.data(), rect_bytes, hipMemcpyHostToDevice, s));
    vdf_alignment *d_dense = nullptr;
    uint32_t *d_total = nullptr;
    vdf::AlignLaunch L{};
    L.a_hashes = reinterpret_cast<const uint32_t *>(in.d_a_hashes); L.a_first = in.d_a_first; L.a_skip = in.d_a_skip;
    L.b_hashes = reinterpret_cast<const uint32_t *>(in.d_b_hashes); L.b_first = in.d_b_first; L.b_skip = in.d_b_skip;
    L.pairs = reinterpret_cast<const vdf::AlignPair *>(plan);
    L.unit_offset = reinterpret_cast<const uint32_t *>(plan + pair_bytes);
    L.n_pairs = (uint32_t)n_pairs; L.n_units = (uint32_t)n_units;
    L.tol = tol; L.min_run = min_run;
    L.scratch = ctx->align_scratch.p; L.dense_out = &d_dense; L.total_out = &d_total;
    L.rects = round.n_rects ? reinterpret_cast<const vdf::AlignRect *>(plan + rect_at) : nullptr;
    L.n_rects = round.n_rects;
    VDF_HIP(ctx, vdf::launch_align_chunk(L, s));
    uint32_t total = 0;
    VDF_HIP(ctx, hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipStreamSynchronize(s));  // also: the round's plan arrays are free to change
    if (total > n_pairs) return fail(ctx, VDF_E_HIP, "align: more records than pairs");
    recs.resize(total);
    if (total) {
        VDF_HIP(ctx, hipMemcpyAsync(recs.data(), d_dense, total * sizeof(vdf_alignment), hipMemcpyDeviceToHost, s));
        VDF_HIP(ctx, hipStreamSynchronize(s));
    }
    return VDF_OK;
}

// align_checks and align_stretches_checks have passed.  Per chunk: round 0 is the plain launch of align_locked; round r runs the masked kernel
// on the pairs that had a record in round r - 1 (align_plan.h: align_next_round), until a round has no survivors or max_stretches rounds have
// run; the rounds are merged into (a, b, rank) order.  Chunks arrive in (a, b) order and each is finished before the next, so the first
// `capacity` records of the call are the ones written.
int align_stretches_locked(vdf_ctx *ctx, const AlignSides &in, uint32_t tol_int, uint32_t min_run, uint32_t max_stretches, uint32_t guard,
                           vdf_alignment_stretch *out, size_t capacity, size_t *n_out, hipStream_t s, const vdf_video_pair *list = nullptr,
                           size_t n_list = 0)  // list: only these pairs (checked: align_pair_list_check), not all of them
{
    vdf::AlignCursor cur;
    vdf::AlignChunk ch;
    vdf::AlignRound round, next;
    std::vector<std::vector<vdf_alignment>> rounds;
    const uint32_t tol = std::min<uint32_t>(tol_int, 1024u);
    size_t found = 0, list_at = 0;
    while (list ? vdf::align_next_chunk_pairs(in.h_first_a, in.h_first_b, list, n_list, list_at, ch)
                : vdf::align_next_chunk(in.h_first_a, in.n_a, in.h_first_b, in.n_b, in.self, cur, ch)) {
        vdf::align_round_zero(ch, round);
        rounds.clear();
        for (uint32_t r = 0; r < max_stretches; r++) {
            rounds.emplace_back();
            if (int rc = align_run_round(ctx, in, round, tol, min_run, rounds.back(), s)) return rc;
            if (rounds.back().empty()) { rounds.pop_back(); break; }
            if (r + 1 == max_stretches) break;
            if (!vdf::align_next_round(round, rounds.back().data(), rounds.back().size(), in.h_first_a, in.h_first_b, guard, next))
                return fail(ctx, VDF_E_HIP, "align: a round's records do not belong to its pairs");
            std::swap(round, next);
        }
        align_merge_rounds(rounds, [&](const vdf_alignment_stretch &r) {
            if (found < capacity) out[found] = r;
            found++;
        });
    }
    *n_out = found;
    return VDF_OK;
}

// ---- seeded candidate pairs, and the align calls on a list of pairs (include/vdf.h: vdf_align_seed_pairs*, vdf_align_windows_pairs*)
// behind align_checks: what the list of a *_pairs call must be
int align_list_checks(vdf_ctx *ctx, const vdf_video_pair *list, size_t n_list, size_t n_a, size_t n_b, bool self)
{
    size_t at = 0;
    switch (vdf::align_pair_list_check(list, n_list, n_a, n_b, self, &at)) {
    case 1: return fail(ctx, VDF_E_INVAL, "the pair list is not strictly increasing in (a, b) at entry " + std::to_string(at));
    case 2: return fail(ctx, VDF_E_INVAL, "pair " + std::to_string(at) + " of the list names a video that does not exist");
    case 3: return fail(ctx, VDF_E_INVAL, "pair " + std::to_string(at) + " of the list has a >= b in self mode");
    default: return VDF_OK;
    }
}

// the literal definition of the candidate set: every seed of a against every window of b, XOR + popcount
bool seed_pair_host(const uint64_t *A, uint32_t Na, const uint8_t *skip_a, const uint64_t *B, uint32_t Nb, const uint8_t *skip_b, uint32_t tol, uint32_t min_run)
{
    for (uint64_t ka = 0; ka < Na; ka += min_run) {
        if (skip_a && skip_a[ka]) continue;
        for (uint32_t kb = 0; kb < Nb; kb++) {
            if (skip_b && skip_b[kb]) continue;
            uint32_t dist = 0;
            for (int w = 0; w < VDF_HASH_WORDS; w++) dist += (uint32_t)__builtin_popcountll(A[16 * ka + w] ^ B[16 * (size_t)kb + w]);
            if (dist <= tol) return true;
        }
    }
    return false;
}

// align_checks has passed on the host copies of the first arrays; every array pointer of `in` is a device pointer.  The bitmap is cleared on
// the call's stream, the seed kernel marks it, count + scan give the total; the host reads it, then the first min(total, capacity) pairs.
int align_seed_locked(vdf_ctx *ctx, const AlignSides &in, uint32_t tol_int, uint32_t min_run, vdf_video_pair *out, size_t capacity, size_t *n_out, hipStream_t s)
{
    *n_out = 0;
    vdf::AlignSeedPlan plan;
    vdf::align_seed_plan(in.h_first_a, in.n_a, in.h_first_b, in.n_b, in.self, min_run, plan);
    if (plan.n_units() == 0) return VDF_OK;  // no seed, no row of B, or (self mode) no seed below a row
    const uint64_t n_bits = (uint64_t)in.n_a * in.n_b;  // <= 2^25 + 2^13: align_checks
    const uint32_t n_words = (uint32_t)((n_bits + 31) / 32);
    const size_t n_seeds = plan.n_seeds(), n_chunks = plan.n_chunks();
    const size_t at_video = n_seeds * 4, at_row = at_video + n_seeds * 4, at_tile = at_row + (size_t)plan.n_rows * 4;
    const size_t at_unit = (at_tile + n_chunks * 4 + 7) & ~(size_t)7, plan_bytes = at_unit + (n_chunks + 1) * 8;
    VDF_HIP(ctx, ctx->seed_bitmap.reserve((size_t)n_words * 4));
    VDF_HIP(ctx, ctx->seed_plan.reserve(plan_bytes));
    VDF_HIP(ctx, ctx->align_scratch.reserve(vdf::align_seed_scratch_bytes(n_words)));
    char *dp = ctx->seed_plan.as<char>();
    VDF_HIP(ctx, hipMemsetAsync(ctx->seed_bitmap.p, 0, (size_t)n_words * 4, s));
    VDF_HIP(ctx, hipMemcpyAsync(dp, plan.seed_window.data(), n_seeds * 4, hipMemcpyHostToDevice, s));
    VDF_HIP(ctx, hipMemcpyAsync(dp + at_video, plan.seed_video.data(), n_seeds * 4, hipMemcpyHostToDevice, s));
    VDF_HIP(ctx, hipMemcpyAsync(dp + at_row, plan.row_video.data(), (size_t)plan.n_rows * 4, hipMemcpyHostToDevice, s));
    VDF_HIP(ctx, hipMemcpyAsync(dp + at_tile, plan.tile_first.data(), n_chunks * 4, hipMemcpyHostToDevice, s));
    VDF_HIP(ctx, hipMemcpyAsync(dp + at_unit, plan.unit_offset.data(), (n_chunks + 1) * 8, hipMemcpyHostToDevice, s));
    uint32_t *d_total = nullptr;
    vdf::AlignSeedLaunch L{};
    L.a_hashes = reinterpret_cast<const uint32_t *>(in.d_a_hashes); L.a_skip = in.d_a_skip;
    L.seed_window = reinterpret_cast<const uint32_t *>(dp); L.seed_video = reinterpret_cast<const uint32_t *>(dp + at_video);
    L.n_seeds = (uint32_t)n_seeds;
    L.b_hashes = reinterpret_cast<const uint32_t *>(in.d_b_hashes); L.b_skip = in.d_b_skip;
    L.row_video = reinterpret_cast<const uint32_t *>(dp + at_row); L.row_base = plan.row_base; L.n_rows = plan.n_rows;
    L.unit_offset = reinterpret_cast<const unsigned long long *>(dp + at_unit);
    L.tile_first = reinterpret_cast<const uint32_t *>(dp + at_tile);
    L.n_chunks = (uint32_t)n_chunks; L.n_units = plan.n_units();
    L.tol = std::min<uint32_t>(tol_int, 1024u); L.self_mode = in.self ? 1 : 0; L.n_b = (uint32_t)in.n_b;
    L.bitmap = ctx->seed_bitmap.as<uint32_t>(); L.n_words = n_words;
    L.scratch = ctx->align_scratch.p; L.total_out = &d_total;
    VDF_HIP(ctx, vdf::launch_align_seed(L, s));
    uint32_t total = 0;
    VDF_HIP(ctx, hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipStreamSynchronize(s));  // also: the plan arrays are free to go
    if ((uint64_t)total > n_bits) return fail(ctx, VDF_E_HIP, "align seed: more pairs than bits");
    const size_t take = std::min<size_t>(total, capacity);
    if (take) {
        VDF_HIP(ctx, ctx->seed_out.reserve(take * sizeof(vdf_video_pair)));
        VDF_HIP(ctx, vdf::launch_align_seed_scatter(L, ctx->seed_out.as<vdf_video_pair>(), (uint32_t)take, s));
        VDF_HIP(ctx, hipMemcpyAsync(out, ctx->seed_out.p, take * sizeof(vdf_video_pair), hipMemcpyDeviceToHost, s));
        VDF_HIP(ctx, hipStreamSynchronize(s));
    }
    *n_out = total;
    return VDF_OK;
}

// ---- retimed windows aligned in one call (include/vdf.h: vdf_align_windows_retimed*; align_retimed_plan.h) -----------------------
// behind align_checks: the rate, reduced by its gcd into *num / *den
int align_retimed_checks(vdf_ctx *ctx, uint32_t rate_num, uint32_t rate_den, uint32_t *num, uint32_t *den)
{
    switch (vdf::align_retimed_rate(rate_num, rate_den, num, den)) {
    case 1: return fail(ctx, VDF_E_INVAL, "the rate must have 1 <= den <= num <= 2 den");
    case 2: return fail(ctx, VDF_E_INVAL, "the rate's num is above 32 in lowest terms (VDF_ALIGN_RETIMED_MAX_NUM)");
    default: return VDF_OK;
    }
}

// the literal definition for one pair: every phase's sub-matrix walked diagonal by diagonal on the strided rows, XOR + popcount; every
// diagonal leaves its best run as a band record would, and the header's reduction - the one the kernel's records go through - picks the
// phase-bests and the pair's record.  best->n_windows = 0: no competing run
void align_retimed_pair_host(const uint64_t *A, uint32_t Na, const uint8_t *skip_a, const uint64_t *B, uint32_t Nb, const uint8_t *skip_b, uint32_t num,
                             uint32_t den, uint32_t tol, uint32_t min_run, vdf_alignment_retimed *best)
{
    const uint32_t nb0 = vdf::align_retimed_nb(Nb, den);
    vdf::AlignRetimedBest pair{0u, 0u, 0u, 0u, 0u};
    for (uint32_t p = 0; p < num; p++) {
        const uint32_t na = vdf::align_retimed_na(Na, num, p);
        if (na == 0 || nb0 == 0) continue;
        vdf_alignment ph{};  // the phase-best: align_pair_host's walk with the rows behind (i, j)
        uint32_t ph_score = 0;
        for (int64_t d = -((int64_t)na - 1); d <= (int64_t)nb0 - 1; d++) {
            const int64_t i0 = std::max<int64_t>(0, -d), i1 = std::min<int64_t>(na, (int64_t)nb0 - d);
            uint32_t len = 0, sum = 0;
            for (int64_t i = i0; i <= i1; i++) {  // i1: the cell behind the diagonal's last, a miss
                bool match = false;
                uint32_t dist = 0;
                if (i < i1) {
                    const size_t ra = vdf::align_retimed_row_a(p, num, (uint32_t)i), rb = vdf::align_retimed_row_b(den, (uint32_t)(i + d));
                    if (!(skip_a && skip_a[ra]) && !(skip_b && skip_b[rb])) {
                        const uint64_t *x = A + 16 * ra, *y = B + 16 * rb;
                        for (int w = 0; w < VDF_HASH_WORDS; w++) dist += (uint32_t)__builtin_popcountll(x[w] ^ y[w]);
                        match = dist <= tol;
                    }
                }
                if (match) { len++; sum += dist; continue; }
                if (len >= min_run) {
                    const uint32_t score = len * (tol + 1) - sum, start = (uint32_t)(i - len);
                    if (vdf::align_better(score, (int32_t)d, start, ph_score, ph.offset, ph.start_a)) {
                        ph_score = score; ph.offset = (int32_t)d; ph.start_a = start; ph.n_windows = len; ph.dist_sum = sum;
                    }
                }
                len = 0; sum = 0;
            }
        }
        if (ph_score == 0) continue;
        const uint32_t first_a = vdf::align_retimed_row_a(p, num, ph.start_a), first_b = vdf::align_retimed_row_b(den, (uint32_t)((int32_t)ph.start_a + ph.offset));
        if (vdf::align_retimed_better(ph_score, first_a, first_b, pair)) pair = vdf::AlignRetimedBest{ph_score, first_a, first_b, ph.n_windows, ph.dist_sum};
    }
    best->first_a = pair.first_a; best->first_b = pair.first_b; best->n_windows = pair.score ? pair.n_windows : 0u; best->dist_sum = pair.dist_sum;
}

// align_retimed_pair_host with rectangles (vdf_align_windows_rates_stretches*): the same walk, and a cell whose rows - row
// p + num i of a, row den j of b - lie in one of the n_rects rectangles is a miss.  The rectangles are in rows of the two videos, so each masks
// the cells of every phase.  best->n_windows = 0: no competing run
void align_retimed_pair_masked_host(const uint64_t *A, uint32_t Na, const uint8_t *skip_a, const uint64_t *B, uint32_t Nb, const uint8_t *skip_b, uint32_t num,
                                    uint32_t den, uint32_t tol, uint32_t min_run, const vdf::AlignRect *rects, uint32_t n_rects, vdf_alignment_retimed *best)
{
    const uint32_t nb0 = vdf::align_retimed_nb(Nb, den);
    vdf::AlignRetimedBest pair{0u, 0u, 0u, 0u, 0u};
    for (uint32_t p = 0; p < num; p++) {
        const uint32_t na = vdf::align_retimed_na(Na, num, p);
        if (na == 0 || nb0 == 0) continue;
        vdf_alignment ph{};  // the phase-best
        uint32_t ph_score = 0;
        for (int64_t d = -((int64_t)na - 1); d <= (int64_t)nb0 - 1; d++) {
            const int64_t i0 = std::max<int64_t>(0, -d), i1 = std::min<int64_t>(na, (int64_t)nb0 - d);
            uint32_t len = 0, sum = 0;
            for (int64_t i = i0; i <= i1; i++) {  // i1: the cell behind the diagonal's last, a miss
                bool match = false;
                uint32_t dist = 0;
                if (i < i1) {
                    const size_t ra = vdf::align_retimed_row_a(p, num, (uint32_t)i), rb = vdf::align_retimed_row_b(den, (uint32_t)(i + d));
                    if (!(skip_a && skip_a[ra]) && !(skip_b && skip_b[rb]) && !vdf::align_cell_masked(rects, n_rects, (uint32_t)ra, (uint32_t)rb)) {
                        const uint64_t *x = A + 16 * ra, *y = B + 16 * rb;
                        for (int w = 0; w < VDF_HASH_WORDS; w++) dist += (uint32_t)__builtin_popcountll(x[w] ^ y[w]);
                        match = dist <= tol;
                    }
                }
                if (match) { len++; sum += dist; continue; }
                if (len >= min_run) {
                    const uint32_t score = len * (tol + 1) - sum, start = (uint32_t)(i - len);
                    if (vdf::align_better(score, (int32_t)d, start, ph_score, ph.offset, ph.start_a)) {
                        ph_score = score; ph.offset = (int32_t)d; ph.start_a = start; ph.n_windows = len; ph.dist_sum = sum;
                    }
                }
                len = 0; sum = 0;
            }
        }
        if (ph_score == 0) continue;
        const uint32_t first_a = vdf::align_retimed_row_a(p, num, ph.start_a), first_b = vdf::align_retimed_row_b(den, (uint32_t)((int32_t)ph.start_a + ph.offset));
        if (vdf::align_retimed_better(ph_score, first_a, first_b, pair)) pair = vdf::AlignRetimedBest{ph_score, first_a, first_b, ph.n_windows, ph.dist_sum};
    }
    best->first_a = pair.first_a; best->first_b = pair.first_b; best->n_windows = pair.score ? pair.n_windows : 0u; best->dist_sum = pair.dist_sum;
}

// align_locked for the retimed call: the chunks hold (pair, phase, band) units; num / den in lowest terms.  `in` is never self.
int align_retimed_locked(vdf_ctx *ctx, const AlignSides &in, uint32_t tol_int, uint32_t min_run, uint32_t num, uint32_t den, vdf_alignment_retimed *out,
                         size_t capacity, size_t *n_out, hipStream_t s, const vdf_video_pair *list = nullptr, size_t n_list = 0)
{
    vdf::AlignCursor cur;
    vdf::AlignChunk ch;
    size_t found = 0, list_at = 0;
    while (list ? vdf::align_retimed_next_chunk_pairs(in.h_first_a, in.h_first_b, list, n_list, num, den, list_at, ch)
                : vdf::align_retimed_next_chunk(in.h_first_a, in.n_a, in.h_first_b, in.n_b, num, den, cur, ch)) {
        const size_t n_pairs = ch.pairs.size(), n_units = ch.n_units();
        const size_t pair_bytes = n_pairs * sizeof(vdf::AlignPair), off_bytes = (n_pairs + 1) * sizeof(uint32_t);
        VDF_HIP(ctx, ctx->align_plan.reserve(pair_bytes + off_bytes));
        VDF_HIP(ctx, ctx->align_scratch.reserve(vdf::align_scratch_bytes(n_pairs, n_units)));
        char *plan = ctx->align_plan.as<char>();
        VDF_HIP(ctx, hipMemcpyAsync(plan, ch.pairs.data(), pair_bytes, hipMemcpyHostToDevice, s));
        VDF_HIP(ctx, hipMemcpyAsync(plan + pair_bytes, ch.unit_offset.data(), off_bytes, hipMemcpyHostToDevice, s));
        vdf_alignment_retimed *d_dense = nullptr;
        uint32_t *d_total = nullptr;
        vdf::AlignLaunch L{};
        L.a_hashes = reinterpret_cast<const uint32_t *>(in.d_a_hashes); L.a_first = in.d_a_first; L.a_skip = in.d_a_skip;
        L.b_hashes = reinterpret_cast<const uint32_t *>(in.d_b_hashes); L.b_first = in.d_b_first; L.b_skip = in.d_b_skip;
        L.pairs = reinterpret_cast<const vdf::AlignPair *>(plan);
        L.unit_offset = reinterpret_cast<const uint32_t *>(plan + pair_bytes);
        L.n_pairs = (uint32_t)n_pairs; L.n_units = (uint32_t)n_units;
        L.tol = std::min<uint32_t>(tol_int, 1024u); L.min_run = min_run;
        L.scratch = ctx->align_scratch.p; L.total_out = &d_total;
        VDF_HIP(ctx, vdf::launch_align_retimed_chunk(L, num, den, &d_dense, s));
        uint32_t total = 0;
        VDF_HIP(ctx, hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, s));
        VDF_HIP(ctx, hipStreamSynchronize(s));  // also: the chunk's plan arrays are free to change
        if (total > n_pairs) return fail(ctx, VDF_E_HIP, "align retimed: more records than pairs");
        const size_t room = capacity > found ? capacity - found : 0, take = std::min<size_t>(total, room);
        if (take) {
            VDF_HIP(ctx, hipMemcpyAsync(out + found, d_dense, take * sizeof(vdf_alignment_retimed), hipMemcpyDeviceToHost, s));
            VDF_HIP(ctx, hipStreamSynchronize(s));
        }
        found += total;
    }
    *n_out = found;
    return VDF_OK;
}

}  // namespace vdf_impl

using namespace vdf_impl;

extern "C" {

int vdf_ctx_create(int device_id, vdf_ctx **out)
{
    if (!out) return VDF_E_INVAL;
    return create_single(device_id, out, &g_create_error);
}

void vdf_ctx_destroy(vdf_ctx *ctx)
{
    if (!ctx) return;
    if (ctx->subs.empty()) {
        (void)hipSetDevice(ctx->device);
        (void)hipDeviceSynchronize();
    }
    delete ctx;  // a multi-GPU parent joins its workers and destroys its sub-contexts (multi.cpp)
}

const char *vdf_last_error(const vdf_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }
int vdf_ctx_device(const vdf_ctx *ctx) { return ctx ? ctx->device : -1; }

int vdf_ctx_set_hit_capacity(vdf_ctx *ctx, uint64_t capacity)
{
    if (!ctx || capacity == 0 || capacity > (1ull << 32)) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->hit_capacity = capacity;
    return VDF_OK;
}

int vdf_ctx_last_search_stats(const vdf_ctx *ctx, vdf_search_stats *out)
{
    if (!ctx || !out) return VDF_E_INVAL;
    *out = ctx->stats;
    return VDF_OK;
}

long long vdf_live_device_bytes(void) { return g_live_device_bytes.load(); }
long long vdf_live_pinned_bytes(void) { return g_live_pinned_bytes.load(); }

int vdf_ctx_last_search_timing(const vdf_ctx *ctx, vdf_search_timing *out)
{
    if (!ctx || !out) return VDF_E_INVAL;
    *out = ctx->timing;
    return VDF_OK;
}

uint32_t vdf_row_tile_size(void) { return vdf::kMfmaRowPad; }  // MFMA backend (default); the VALU backend uses 256 x rows-per-lane

#define VDF_SINGLE_DEVICE_ONLY(ctx)                                                                                   \
    if (!(ctx)->subs.empty())                                                                                         \
        return fail((ctx), VDF_E_INVAL, "device-pointer entry points take a single-device context; a multi-GPU context " \
                                        "offers the host-array calls and the *_shards calls")

int vdf_ctx_pin_database(vdf_ctx *ctx, const uint64_t *d_hashes, size_t n)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    ctx->pinned_db = d_hashes;
    ctx->pinned_n = d_hashes ? n : 0;
    ctx->exp_owner = ExpOwner{};  // whatever was expanded before was not covered by this promise
    return VDF_OK;
}

int vdf_hash_frames_u8_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                              uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride, uint64_t *d_out_hashes,
                              uint32_t *d_out_dontcare, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    return hash_device_locked(ctx, d_frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride, d_out_hashes,
                              d_out_dontcare, s);
}

// Host frames -> hashes.  On a multi-GPU context the clips are split contiguously over the devices (clips are
// independent: no communication); every device stages and hashes its share on its own host thread.
static int hash_host_entry(vdf_ctx *ctx, const uint8_t *frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w,
                           uint32_t h, size_t frame_stride, size_t clip_stride, int letterbox, uint64_t *out_hashes,
                           uint32_t *out_crops, uint32_t *out_dontcare)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (frames_per_clip < VDF_DCT_SIZE) return fail(ctx, VDF_E_NOT_ENOUGH_FRAMES, "fewer than 16 frames per clip");
    if (w == 0 || h == 0) return fail(ctx, VDF_E_BAD_DIMS, "zero frame dimension");
    if (frame_stride < (size_t)w * h) return fail(ctx, VDF_E_INVAL, "frame_stride smaller than a frame");
    if (n_clips == 0) return VDF_OK;
    if (!frames || !out_hashes) return fail(ctx, VDF_E_INVAL, "null pointer");
    const int G = device_count(ctx);
    return for_each_device(ctx, [&](int k, vdf_ctx *d) {
        const size_t base = n_clips / (size_t)G, rem = n_clips % (size_t)G;
        const size_t lo = (size_t)k * base + std::min<size_t>((size_t)k, rem), cnt = base + ((size_t)k < rem ? 1 : 0);
        if (cnt == 0) return (int)VDF_OK;
        return hash_host_locked(d, frames + lo * clip_stride, cnt, w, h, frame_stride, clip_stride, letterbox,
                                out_hashes + lo * VDF_HASH_WORDS, out_crops ? out_crops + 4 * lo : nullptr,
                                out_dontcare ? out_dontcare + lo : nullptr);
    });
}

int vdf_hash_frames_u8(vdf_ctx *ctx, const uint8_t *frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w,
                       uint32_t h, size_t frame_stride, size_t clip_stride, uint64_t *out_hashes,
                       uint32_t *out_dontcare)
{
    return hash_host_entry(ctx, frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride, 0, out_hashes, nullptr,
                           out_dontcare);
}

int vdf_hash_frames_u8_letterbox(vdf_ctx *ctx, const uint8_t *frames, size_t n_clips, uint32_t frames_per_clip,
                                 uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride, uint64_t *out_hashes,
                                 uint32_t *out_crops, uint32_t *out_dontcare)
{
    return hash_host_entry(ctx, frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride, 1, out_hashes, out_crops,
                           out_dontcare);
}

int vdf_align_windows_host(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes,
                           const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, uint32_t tol_int, uint32_t min_run, vdf_alignment *out,
                           size_t capacity, size_t *n_out)
{
    if (int rc = align_checks(nullptr, a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first, b_first, min_run, out, capacity, n_out)) return rc;
    const bool self = b_hashes == nullptr;
    if (self) { b_hashes = a_hashes; b_first = a_first; n_b = n_a; b_skip = a_skip; }
    const uint32_t tol = std::min<uint32_t>(tol_int, 1024u);
    size_t found = 0;
    for (size_t a = 0; a < n_a; a++)
        for (size_t b = self ? a + 1 : 0; b < n_b; b++) {
            vdf_alignment r;
            align_pair_host(a_hashes + 16 * (size_t)a_first[a], a_first[a + 1] - a_first[a], a_skip ? a_skip + a_first[a] : nullptr,
                            b_hashes + 16 * (size_t)b_first[b], b_first[b + 1] - b_first[b], b_skip ? b_skip + b_first[b] : nullptr, tol, min_run, &r);
            if (r.n_windows == 0) continue;
            r.a = (uint32_t)a; r.b = (uint32_t)b;
            if (found < capacity) out[found] = r;
            found++;
        }
    *n_out = found;
    return VDF_OK;
}

int vdf_align_windows_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a, const uint8_t *d_a_skip,
                             const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b, const uint8_t *d_b_skip, uint32_t tol_int,
                             uint32_t min_run, vdf_alignment *out, size_t capacity, size_t *n_out, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    // everything that can be said without the first arrays; then they come down, are checked, and plan the launch
    if (int rc = align_checks(ctx, d_a_hashes, nullptr, n_a, d_b_hashes, nullptr, n_b, d_a_first, d_b_first, min_run, out, capacity, n_out)) return rc;
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "vdf_align_windows_device takes a single-device context");
    const bool self = d_b_hashes == nullptr;
    *n_out = 0;
    if (n_a == 0 || (self ? n_a < 2 : n_b == 0)) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    std::vector<uint32_t> fa(n_a + 1), fb(self ? 0 : n_b + 1);
    VDF_HIP(ctx, hipMemcpyAsync(fa.data(), d_a_first, fa.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (!self) VDF_HIP(ctx, hipMemcpyAsync(fb.data(), d_b_first, fb.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipStreamSynchronize(s));
    if (int rc = align_checks(ctx, d_a_hashes, fa.data(), n_a, d_b_hashes, self ? nullptr : fb.data(), n_b, d_a_first, d_b_first, min_run, out, capacity, n_out))
        return rc;
    if (self) return align_locked(ctx, d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, true, tol_int, min_run,
                                  out, capacity, n_out, s);
    return align_locked(ctx, d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, d_b_hashes, d_b_first, fb.data(), n_b, d_b_skip, false, tol_int, min_run, out,
                        capacity, n_out, s);
}

// Host arrays of an align call -> the context's staging buffers: the hashes of A (up_hashes) and, unless self, of B (up_ref_hashes), the first
// arrays rebased to the uploaded windows and the skip arrays ([first a | first b | skip a | skip b] in align_up).
struct AlignUploaded {
    std::vector<uint32_t> fa, fb;  // the rebased first arrays, on the host
    const uint32_t *d_fa, *d_fb;
    const uint8_t *d_ska, *d_skb;
};
static int align_upload(vdf_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes,
                        const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, bool self, hipStream_t s, AlignUploaded *u)
{
    const size_t wa = a_first[n_a] - a_first[0], wb = self ? 0 : b_first[n_b] - b_first[0];
    std::vector<uint32_t> &fa = u->fa, &fb = u->fb;
    fa.assign(n_a + 1, 0);
    fb.assign(self ? 0 : n_b + 1, 0);
    for (size_t v = 0; v <= n_a; v++) fa[v] = a_first[v] - a_first[0];
    for (size_t v = 0; v < fb.size(); v++) fb[v] = b_first[v] - b_first[0];
    const size_t fa_bytes = fa.size() * sizeof(uint32_t), fb_bytes = fb.size() * sizeof(uint32_t);
    const size_t ska = a_skip ? wa : 0, skb = (!self && b_skip) ? wb : 0;
    VDF_HIP(ctx, ctx->align_up.reserve(fa_bytes + fb_bytes + ska + skb + 16));
    char *up = ctx->align_up.as<char>();
    VDF_HIP(ctx, hipMemcpyAsync(up, fa.data(), fa_bytes, hipMemcpyHostToDevice, s));
    if (fb_bytes) VDF_HIP(ctx, hipMemcpyAsync(up + fa_bytes, fb.data(), fb_bytes, hipMemcpyHostToDevice, s));
    if (ska) VDF_HIP(ctx, hipMemcpyAsync(up + fa_bytes + fb_bytes, a_skip + a_first[0], ska, hipMemcpyHostToDevice, s));
    if (skb) VDF_HIP(ctx, hipMemcpyAsync(up + fa_bytes + fb_bytes + ska, b_skip + b_first[0], skb, hipMemcpyHostToDevice, s));
    if (int rc = upload(ctx, ctx->up_hashes, a_hashes + 16 * (size_t)a_first[0], wa * 16 * sizeof(uint64_t), s)) return rc;
    if (!self)
        if (int rc = upload(ctx, ctx->up_ref_hashes, b_hashes + 16 * (size_t)b_first[0], wb * 16 * sizeof(uint64_t), s)) return rc;
    u->d_fa = reinterpret_cast<const uint32_t *>(up);
    u->d_fb = reinterpret_cast<const uint32_t *>(up + fa_bytes);
    u->d_ska = ska ? reinterpret_cast<const uint8_t *>(up + fa_bytes + fb_bytes) : nullptr;
    u->d_skb = skb ? reinterpret_cast<const uint8_t *>(up + fa_bytes + fb_bytes + ska) : nullptr;
    return VDF_OK;
}

// Host arrays: hashes, first and skip arrays go up through the context's staging buffers, the device form's core runs on them.
int vdf_align_windows(vdf_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes,
                      const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, uint32_t tol_int, uint32_t min_run, vdf_alignment *out, size_t capacity,
                      size_t *n_out)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int rc = align_checks(ctx, a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first, b_first, min_run, out, capacity, n_out)) return rc;
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "vdf_align_windows takes a single-device context");
    const bool self = b_hashes == nullptr;
    *n_out = 0;
    if (n_a == 0 || (self ? n_a < 2 : n_b == 0)) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    AlignUploaded u;
    if (int rc = align_upload(ctx, a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip, self, s, &u)) return rc;
    if (self) return align_locked(ctx, ctx->up_hashes.as<uint64_t>(), u.d_fa, u.fa.data(), n_a, u.d_ska, ctx->up_hashes.as<uint64_t>(), u.d_fa, u.fa.data(), n_a,
                                  u.d_ska, true, tol_int, min_run, out, capacity, n_out, s);
    return align_locked(ctx, ctx->up_hashes.as<uint64_t>(), u.d_fa, u.fa.data(), n_a, u.d_ska, ctx->up_ref_hashes.as<uint64_t>(), u.d_fb, u.fb.data(), n_b, u.d_skb,
                        false, tol_int, min_run, out, capacity, n_out, s);
}

int vdf_align_windows_stretches_host(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes,
                                     const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, uint32_t tol_int, uint32_t min_run, uint32_t max_stretches,
                                     uint32_t guard, vdf_alignment_stretch *out, size_t capacity, size_t *n_out)
{
    if (int rc = align_checks(nullptr, a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first, b_first, min_run, out, capacity, n_out)) return rc;
    if (int rc = align_stretches_checks(nullptr, max_stretches, guard)) return rc;
    const bool self = b_hashes == nullptr;
    if (self) { b_hashes = a_hashes; b_first = a_first; n_b = n_a; b_skip = a_skip; }
    const uint32_t tol = std::min<uint32_t>(tol_int, 1024u);
    size_t found = 0;
    for (size_t a = 0; a < n_a; a++)
        for (size_t b = self ? a + 1 : 0; b < n_b; b++) {
            const uint32_t Na = a_first[a + 1] - a_first[a], Nb = b_first[b + 1] - b_first[b];
            vdf::AlignRect rects[vdf::kAlignMaxStretches];
            for (uint32_t rank = 0; rank < max_stretches; rank++) {
                vdf_alignment r;
                align_pair_host(a_hashes + 16 * (size_t)a_first[a], Na, a_skip ? a_skip + a_first[a] : nullptr, b_hashes + 16 * (size_t)b_first[b], Nb,
                                b_skip ? b_skip + b_first[b] : nullptr, tol, min_run, &r, rects, rank);
                if (r.n_windows == 0) break;
                r.a = (uint32_t)a; r.b = (uint32_t)b;
                if (found < capacity) out[found] = stretch_of(r, rank);
                found++;
                rects[rank] = vdf::align_rect_of(r.offset, r.start_a, r.n_windows, guard, Na, Nb);
            }
        }
    *n_out = found;
    return VDF_OK;
}

int vdf_align_windows_stretches_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a, const uint8_t *d_a_skip,
                                       const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b, const uint8_t *d_b_skip, uint32_t tol_int,
                                       uint32_t min_run, uint32_t max_stretches, uint32_t guard, vdf_alignment_stretch *out, size_t capacity,
                                       size_t *n_out, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const bool self = d_b_hashes == nullptr;
    // as vdf_align_windows_device: everything that can be said without the first arrays; then they come down, are checked, and plan the launch
    if (int rc = align_checks(ctx, d_a_hashes, nullptr, n_a, d_b_hashes, nullptr, n_b, d_a_first, d_b_first, min_run, out, capacity, n_out)) return rc;
    auto later_checks = [&]() -> int {
        if (int rc = align_stretches_checks(ctx, max_stretches, guard)) return rc;
        if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "vdf_align_windows_stretches_device takes a single-device context");
        return VDF_OK;
    };
    *n_out = 0;
    if (n_a == 0 || (self ? n_a < 2 : n_b == 0)) return later_checks();
    if (!ctx->subs.empty()) return later_checks();  // the first arrays of a multi-GPU context's caller are not read: the call is refused either way
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    std::vector<uint32_t> fa(n_a + 1), fb(self ? 0 : n_b + 1);
    VDF_HIP(ctx, hipMemcpyAsync(fa.data(), d_a_first, fa.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (!self) VDF_HIP(ctx, hipMemcpyAsync(fb.data(), d_b_first, fb.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipStreamSynchronize(s));
    if (int rc = align_checks(ctx, d_a_hashes, fa.data(), n_a, d_b_hashes, self ? nullptr : fb.data(), n_b, d_a_first, d_b_first, min_run, out, capacity, n_out))
        return rc;
    if (int rc = later_checks()) return rc;
    const AlignSides in = self ? AlignSides{d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, true}
                               : AlignSides{d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, d_b_hashes, d_b_first, fb.data(), n_b, d_b_skip, false};
    return align_stretches_locked(ctx, in, tol_int, min_run, max_stretches, guard, out, capacity, n_out, s);
}

// Host arrays: uploaded as vdf_align_windows uploads them, then the device form's core.
int vdf_align_windows_stretches(vdf_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes,
                                const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, uint32_t tol_int, uint32_t min_run, uint32_t max_stretches,
                                uint32_t guard, vdf_alignment_stretch *out, size_t capacity, size_t *n_out)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int rc = align_checks(ctx, a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first, b_first, min_run, out, capacity, n_out)) return rc;
    if (int rc = align_stretches_checks(ctx, max_stretches, guard)) return rc;
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "vdf_align_windows_stretches takes a single-device context");
    const bool self = b_hashes == nullptr;
    *n_out = 0;
    if (n_a == 0 || (self ? n_a < 2 : n_b == 0)) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    AlignUploaded u;
    if (int rc = align_upload(ctx, a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip, self, s, &u)) return rc;
    const uint64_t *d_a = ctx->up_hashes.as<uint64_t>();
    const AlignSides in = self ? AlignSides{d_a, u.d_fa, u.fa.data(), n_a, u.d_ska, d_a, u.d_fa, u.fa.data(), n_a, u.d_ska, true}
                               : AlignSides{d_a, u.d_fa, u.fa.data(), n_a, u.d_ska, ctx->up_ref_hashes.as<uint64_t>(), u.d_fb, u.fb.data(), n_b, u.d_skb, false};
    return align_stretches_locked(ctx, in, tol_int, min_run, max_stretches, guard, out, capacity, n_out, s);
}

// ---- seeded candidate pairs, and the align calls on a list of pairs ---------------------------------------------------------------
int vdf_align_seed_pairs_host(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes,
                              const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, uint32_t tol_int, uint32_t min_run, vdf_video_pair *out,
                              size_t capacity, size_t *n_out)
{
    if (int rc = align_checks(nullptr, a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first, b_first, min_run, out, capacity, n_out)) return rc;
    const bool self = b_hashes == nullptr;
    if (self) { b_hashes = a_hashes; b_first = a_first; n_b = n_a; b_skip = a_skip; }
    const uint32_t tol = std::min<uint32_t>(tol_int, 1024u);
    size_t found = 0;
    for (size_t a = 0; a < n_a; a++)
        for (size_t b = self ? a + 1 : 0; b < n_b; b++) {
            if (!seed_pair_host(a_hashes + 16 * (size_t)a_first[a], a_first[a + 1] - a_first[a], a_skip ? a_skip + a_first[a] : nullptr,
                                b_hashes + 16 * (size_t)b_first[b], b_first[b + 1] - b_first[b], b_skip ? b_skip + b_first[b] : nullptr, tol, min_run))
                continue;
            if (found < capacity) out[found] = vdf_video_pair{(uint32_t)a, (uint32_t)b};
            found++;
        }
    *n_out = found;
    return VDF_OK;
}

// The first arrays of a device form come down to plan the launch (as vdf_align_windows_device reads them)
static int align_first_down(vdf_ctx *ctx, const uint32_t *d_a_first, size_t n_a, const uint32_t *d_b_first, size_t n_b, bool self, hipStream_t s,
                            std::vector<uint32_t> &fa, std::vector<uint32_t> &fb)
{
    fa.assign(n_a + 1, 0);
    fb.assign(self ? 0 : n_b + 1, 0);
    VDF_HIP(ctx, hipMemcpyAsync(fa.data(), d_a_first, fa.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (!self) VDF_HIP(ctx, hipMemcpyAsync(fb.data(), d_b_first, fb.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipStreamSynchronize(s));
    return VDF_OK;
}

int vdf_align_seed_pairs_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a, const uint8_t *d_a_skip,
                                const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b, const uint8_t *d_b_skip, uint32_t tol_int,
                                uint32_t min_run, vdf_video_pair *out, size_t capacity, size_t *n_out, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    // as vdf_align_windows_device: everything that can be said without the first arrays; then they come down, are checked, and plan the launch
    if (int rc = align_checks(ctx, d_a_hashes, nullptr, n_a, d_b_hashes, nullptr, n_b, d_a_first, d_b_first, min_run, out, capacity, n_out)) return rc;
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "vdf_align_seed_pairs_device takes a single-device context");
    const bool self = d_b_hashes == nullptr;
    *n_out = 0;
    if (n_a == 0 || (self ? n_a < 2 : n_b == 0)) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    std::vector<uint32_t> fa, fb;
    if (int rc = align_first_down(ctx, d_a_first, n_a, d_b_first, n_b, self, s, fa, fb)) return rc;
    if (int rc = align_checks(ctx, d_a_hashes, fa.data(), n_a, d_b_hashes, self ? nullptr : fb.data(), n_b, d_a_first, d_b_first, min_run, out, capacity, n_out))
        return rc;
    const AlignSides in = self ? AlignSides{d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, true}
                               : AlignSides{d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, d_b_hashes, d_b_first, fb.data(), n_b, d_b_skip, false};
    return align_seed_locked(ctx, in, tol_int, min_run, out, capacity, n_out, s);
}

// the sides of a host-array call once align_upload has staged them
static AlignSides align_sides_uploaded(vdf_ctx *ctx, const AlignUploaded &u, size_t n_a, size_t n_b, bool self)
{
    const uint64_t *d_a = ctx->up_hashes.as<uint64_t>();
    return self ? AlignSides{d_a, u.d_fa, u.fa.data(), n_a, u.d_ska, d_a, u.d_fa, u.fa.data(), n_a, u.d_ska, true}
                : AlignSides{d_a, u.d_fa, u.fa.data(), n_a, u.d_ska, ctx->up_ref_hashes.as<uint64_t>(), u.d_fb, u.fb.data(), n_b, u.d_skb, false};
}

int vdf_align_seed_pairs(vdf_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes,
                         const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, uint32_t tol_int, uint32_t min_run, vdf_video_pair *out,
                         size_t capacity, size_t *n_out)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int rc = align_checks(ctx, a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first, b_first, min_run, out, capacity, n_out)) return rc;
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "vdf_align_seed_pairs takes a single-device context");
    const bool self = b_hashes == nullptr;
    *n_out = 0;
    if (n_a == 0 || (self ? n_a < 2 : n_b == 0)) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    AlignUploaded u;
    if (int rc = align_upload(ctx, a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip, self, s, &u)) return rc;
    return align_seed_locked(ctx, align_sides_uploaded(ctx, u, n_a, n_b, self), tol_int, min_run, out, capacity, n_out, s);
}

// The checks of the *_pairs forms, in the order include/vdf.h gives them.  stretches: max_stretches and guard are checked too, behind the
// align checks.  first arrays on the host, or null (a device form before they have come down).
static int align_pairs_checks(vdf_ctx *ctx, const char *name, const void *a_hashes, const uint32_t *a_first, size_t n_a, const void *b_hashes,
                              const uint32_t *b_first, size_t n_b, const void *a_first_ptr, const void *b_first_ptr, const vdf_video_pair *pairs,
                              size_t n_pairs, uint32_t min_run, bool stretches, uint32_t max_stretches, uint32_t guard, const void *out, size_t capacity,
                              const size_t *n_out, bool device_ctx)
{
    if (n_pairs && !pairs) return fail(ctx, VDF_E_INVAL, "null pair list");
    if (int rc = align_checks(ctx, a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first_ptr, b_first_ptr, min_run, out, capacity, n_out, &n_pairs)) return rc;
    if (stretches)
        if (int rc = align_stretches_checks(ctx, max_stretches, guard)) return rc;
    if (int rc = align_list_checks(ctx, pairs, n_pairs, n_a, n_b, b_hashes == nullptr)) return rc;
    if (device_ctx && !ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, std::string(name) + " takes a single-device context");
    return VDF_OK;
}

// The plain and the stretches form share their bodies: `stretches` says which of out / out_st is written (the plain form: max_stretches 1).
static int align_pairs_host_impl(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes,
                                 const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, const vdf_video_pair *pairs, size_t n_pairs, uint32_t tol_int,
                                 uint32_t min_run, bool stretches, uint32_t max_stretches, uint32_t guard, vdf_alignment *out, vdf_alignment_stretch *out_st,
                                 size_t capacity, size_t *n_out)
{
    const void *o = stretches ? (const void *)out_st : (const void *)out;
    if (int rc = align_pairs_checks(nullptr, "", a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first, b_first, pairs, n_pairs, min_run, stretches,
                                    max_stretches, guard, o, capacity, n_out, false))
        return rc;
    const bool self = b_hashes == nullptr;
    if (self) { b_hashes = a_hashes; b_first = a_first; n_b = n_a; b_skip = a_skip; }
    const uint32_t tol = std::min<uint32_t>(tol_int, 1024u);
    size_t found = 0;
    for (size_t i = 0; i < n_pairs; i++) {
        const uint32_t a = pairs[i].a, b = pairs[i].b;
        const uint32_t Na = a_first[a + 1] - a_first[a], Nb = b_first[b + 1] - b_first[b];
        vdf::AlignRect rects[vdf::kAlignMaxStretches];
        for (uint32_t rank = 0; rank < max_stretches; rank++) {
            vdf_alignment r;
            align_pair_host(a_hashes + 16 * (size_t)a_first[a], Na, a_skip ? a_skip + a_first[a] : nullptr, b_hashes + 16 * (size_t)b_first[b], Nb,
                            b_skip ? b_skip + b_first[b] : nullptr, tol, min_run, &r, rects, rank);
            if (r.n_windows == 0) break;
            r.a = a; r.b = b;
            if (found < capacity) {
                if (stretches) out_st[found] = stretch_of(r, rank);
                else out[found] = r;
            }
            found++;
            rects[rank] = vdf::align_rect_of(r.offset, r.start_a, r.n_windows, guard, Na, Nb);
        }
    }
    *n_out = found;
    return VDF_OK;
}

static int align_pairs_run(vdf_ctx *ctx, const AlignSides &in, const vdf_video_pair *pairs, size_t n_pairs, uint32_t tol_int, uint32_t min_run, bool stretches,
                           uint32_t max_stretches, uint32_t guard, vdf_alignment *out, vdf_alignment_stretch *out_st, size_t capacity, size_t *n_out, hipStream_t s)
{
    if (stretches) return align_stretches_locked(ctx, in, tol_int, min_run, max_stretches, guard, out_st, capacity, n_out, s, pairs, n_pairs);
    return align_locked(ctx, in.d_a_hashes, in.d_a_first, in.h_first_a, in.n_a, in.d_a_skip, in.d_b_hashes, in.d_b_first, in.h_first_b, in.n_b, in.d_b_skip,
                        in.self, tol_int, min_run, out, capacity, n_out, s, pairs, n_pairs);
}

static int align_pairs_device_impl(vdf_ctx *ctx, const char *name, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a, const uint8_t *d_a_skip,
                                   const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b, const uint8_t *d_b_skip, const vdf_video_pair *pairs,
                                   size_t n_pairs, uint32_t tol_int, uint32_t min_run, bool stretches, uint32_t max_stretches, uint32_t guard,
                                   vdf_alignment *out, vdf_alignment_stretch *out_st, size_t capacity, size_t *n_out, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const void *o = stretches ? (const void *)out_st : (const void *)out;
    const bool self = d_b_hashes == nullptr;
    // everything that can be said without the first arrays - the multi-GPU refusal last; then they come down and are checked
    if (int rc = align_pairs_checks(ctx, name, d_a_hashes, nullptr, n_a, d_b_hashes, nullptr, n_b, d_a_first, d_b_first, pairs, n_pairs, min_run, stretches,
                                    max_stretches, guard, o, capacity, n_out, true))
        return rc;
    *n_out = 0;
    if (n_pairs == 0) return VDF_OK;  // (a checked list with an entry: both sides have a video)
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    std::vector<uint32_t> fa, fb;
    if (int rc = align_first_down(ctx, d_a_first, n_a, d_b_first, n_b, self, s, fa, fb)) return rc;
    if (int rc = align_checks(ctx, d_a_hashes, fa.data(), n_a, d_b_hashes, self ? nullptr : fb.data(), n_b, d_a_first, d_b_first, min_run, o, capacity, n_out, &n_pairs))
        return rc;
    const AlignSides in = self ? AlignSides{d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, true}
                               : AlignSides{d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, d_b_hashes, d_b_first, fb.data(), n_b, d_b_skip, false};
    return align_pairs_run(ctx, in, pairs, n_pairs, tol_int, min_run, stretches, max_stretches, guard, out, out_st, capacity, n_out, s);
}

static int align_pairs_ctx_impl(vdf_ctx *ctx, const char *name, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, const vdf_video_pair *pairs, size_t n_pairs,
                                uint32_t tol_int, uint32_t min_run, bool stretches, uint32_t max_stretches, uint32_t guard, vdf_alignment *out,
                                vdf_alignment_stretch *out_st, size_t capacity, size_t *n_out)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const void *o = stretches ? (const void *)out_st : (const void *)out;
    if (int rc = align_pairs_checks(ctx, name, a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first, b_first, pairs, n_pairs, min_run, stretches, max_stretches,
                                    guard, o, capacity, n_out, true))
        return rc;
    const bool self = b_hashes == nullptr;
    *n_out = 0;
    if (n_pairs == 0) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    AlignUploaded u;
    if (int rc = align_upload(ctx, a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip, self, s, &u)) return rc;
    return align_pairs_run(ctx, align_sides_uploaded(ctx, u, n_a, n_b, self), pairs, n_pairs, tol_int, min_run, stretches, max_stretches, guard, out, out_st,
                           capacity, n_out, s);
}

int vdf_align_windows_pairs_host(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes,
                                 const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, const vdf_video_pair *pairs, size_t n_pairs, uint32_t tol_int,
                                 uint32_t min_run, vdf_alignment *out, size_t capacity, size_t *n_out)
{
    return align_pairs_host_impl(a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip, pairs, n_pairs, tol_int, min_run, false, 1,
                                                       0, out, nullptr, capacity, n_out);
}

int vdf_align_windows_stretches_pairs_host(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes,
                                           const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, const vdf_video_pair *pairs, size_t n_pairs,
                                           uint32_t tol_int, uint32_t min_run, uint32_t max_stretches, uint32_t guard, vdf_alignment_stretch *out,
                                           size_t capacity, size_t *n_out)
{
    return align_pairs_host_impl(a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip, pairs, n_pairs, tol_int, min_run, true, max_stretches, guard,
                                 nullptr, out, capacity, n_out);
}

int vdf_align_windows_pairs_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a, const uint8_t *d_a_skip,
                                   const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b, const uint8_t *d_b_skip, const vdf_video_pair *pairs,
                                   size_t n_pairs, uint32_t tol_int, uint32_t min_run, vdf_alignment *out, size_t capacity, size_t *n_out, void *stream)
{
    return align_pairs_device_impl(ctx, "vdf_align_windows_pairs_device", d_a_hashes, d_a_first, n_a, d_a_skip, d_b_hashes, d_b_first, n_b, d_b_skip, pairs,
                                   n_pairs, tol_int, min_run, false, 1, 0, out, nullptr, capacity, n_out, stream);
}

int vdf_align_windows_stretches_pairs_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a, const uint8_t *d_a_skip,
                                             const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b, const uint8_t *d_b_skip,
                                             const vdf_video_pair *pairs, size_t n_pairs, uint32_t tol_int, uint32_t min_run, uint32_t max_stretches,
                                             uint32_t guard, vdf_alignment_stretch *out, size_t capacity, size_t *n_out, void *stream)
{
    return align_pairs_device_impl(ctx, "vdf_align_windows_stretches_pairs_device", d_a_hashes, d_a_first, n_a, d_a_skip, d_b_hashes, d_b_first, n_b, d_b_skip,
                                   pairs, n_pairs, tol_int, min_run, true, max_stretches, guard, nullptr, out, capacity, n_out, stream);
}

int vdf_align_windows_pairs(vdf_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes,
                            const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, const vdf_video_pair *pairs, size_t n_pairs, uint32_t tol_int,
                            uint32_t min_run, vdf_alignment *out, size_t capacity, size_t *n_out)
{
    return align_pairs_ctx_impl(ctx, "vdf_align_windows_pairs", a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip, pairs, n_pairs, tol_int, min_run,
                                false, 1, 0, out, nullptr, capacity, n_out);
}

int vdf_align_windows_stretches_pairs(vdf_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                      const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, const vdf_video_pair *pairs,
                                      size_t n_pairs, uint32_t tol_int, uint32_t min_run, uint32_t max_stretches, uint32_t guard, vdf_alignment_stretch *out,
                                      size_t capacity, size_t *n_out)
{
    return align_pairs_ctx_impl(ctx, "vdf_align_windows_stretches_pairs", a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip, pairs, n_pairs, tol_int,
                                min_run, true, max_stretches, guard, nullptr, out, capacity, n_out);
}

// ---- retimed windows aligned in one call ------------------------------------------------------------------------------------------
// The checks of the six forms, in the order include/vdf.h gives them; `listed`: a *_pairs form.  first arrays on the host, or null (a device
// form before they have come down).  *num / *den: the rate in lowest terms.
static int align_retimed_all_checks(vdf_ctx *ctx, const char *name, const void *a_hashes, const uint32_t *a_first, size_t n_a, const void *b_hashes,
                                    const uint32_t *b_first, size_t n_b, const void *a_first_ptr, const void *b_first_ptr, const vdf_video_pair *pairs,
                                    size_t n_pairs, bool listed, uint32_t min_run, uint32_t rate_num, uint32_t rate_den, uint32_t *num, uint32_t *den,
                                    const void *out, size_t capacity, const size_t *n_out, bool device_ctx)
{
    if (listed && n_pairs && !pairs) return fail(ctx, VDF_E_INVAL, "null pair list");
    // no self mode: a missing B is a null pointer like any other (an empty B may come without hashes)
    if (!b_hashes && n_b) return fail(ctx, VDF_E_INVAL, "null pointer");
    static const uint64_t no_hashes = 0;
    if (int rc = align_checks(ctx, a_hashes, a_first, n_a, b_hashes ? b_hashes : &no_hashes, b_first, n_b, a_first_ptr, b_first_ptr, min_run, out, capacity,
                              n_out, listed ? &n_pairs : nullptr))
        return rc;
    if (int rc = align_retimed_checks(ctx, rate_num, rate_den, num, den)) return rc;
    if (listed)
        if (int rc = align_list_checks(ctx, pairs, n_pairs, n_a, n_b, false)) return rc;
    if (device_ctx && !ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, std::string(name) + " takes a single-device context");
    return VDF_OK;
}

static int align_retimed_host_impl(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes,
                                   const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, const vdf_video_pair *pairs, size_t n_pairs, bool listed,
                                   uint32_t tol_int, uint32_t min_run, uint32_t rate_num, uint32_t rate_den, vdf_alignment_retimed *out, size_t capacity,
                                   size_t *n_out)
{
    uint32_t num = 1, den = 1;
    if (int rc = align_retimed_all_checks(nullptr, "", a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first, b_first, pairs, n_pairs, listed, min_run,
                                          rate_num, rate_den, &num, &den, out, capacity, n_out, false))
        return rc;
    const uint32_t tol = std::min<uint32_t>(tol_int, 1024u);
    size_t found = 0;
    const auto pair = [&](uint32_t a, uint32_t b) {
        vdf_alignment_retimed r;
        align_retimed_pair_host(a_hashes + 16 * (size_t)a_first[a], a_first[a + 1] - a_first[a], a_skip ? a_skip + a_first[a] : nullptr,
                                b_hashes + 16 * (size_t)b_first[b], b_first[b + 1] - b_first[b], b_skip ? b_skip + b_first[b] : nullptr, num, den, tol, min_run,
                                &r);
        if (r.n_windows == 0) return;
        r.a = a; r.b = b;
        if (found < capacity) out[found] = r;
        found++;
    };
    if (listed)
        for (size_t i = 0; i < n_pairs; i++) pair(pairs[i].a, pairs[i].b);
    else
        for (size_t a = 0; a < n_a; a++)
            for (size_t b = 0; b < n_b; b++) pair((uint32_t)a, (uint32_t)b);
    *n_out = found;
    return VDF_OK;
}

static int align_retimed_device_impl(vdf_ctx *ctx, const char *name, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a, const uint8_t *d_a_skip,
                                     const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b, const uint8_t *d_b_skip, const vdf_video_pair *pairs,
                                     size_t n_pairs, bool listed, uint32_t tol_int, uint32_t min_run, uint32_t rate_num, uint32_t rate_den,
                                     vdf_alignment_retimed *out, size_t capacity, size_t *n_out, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    uint32_t num = 1, den = 1;
    // everything that can be said without the first arrays - the multi-GPU refusal last; then they come down and are checked
    if (int rc = align_retimed_all_checks(ctx, name, d_a_hashes, nullptr, n_a, d_b_hashes, nullptr, n_b, d_a_first, d_b_first, pairs, n_pairs, listed, min_run,
                                          rate_num, rate_den, &num, &den, out, capacity, n_out, true))
        return rc;
    *n_out = 0;
    if (listed ? n_pairs == 0 : (n_a == 0 || n_b == 0)) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    std::vector<uint32_t> fa, fb;
    if (int rc = align_first_down(ctx, d_a_first, n_a, d_b_first, n_b, false, s, fa, fb)) return rc;
    if (int rc = align_checks(ctx, d_a_hashes, fa.data(), n_a, d_b_hashes, fb.data(), n_b, d_a_first, d_b_first, min_run, out, capacity, n_out,
                              listed ? &n_pairs : nullptr))
        return rc;
    const AlignSides in{d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, d_b_hashes, d_b_first, fb.data(), n_b, d_b_skip, false};
    return align_retimed_locked(ctx, in, tol_int, min_run, num, den, out, capacity, n_out, s, listed ? pairs : nullptr, n_pairs);
}

static int align_retimed_ctx_impl(vdf_ctx *ctx, const char *name, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                  const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, const vdf_video_pair *pairs, size_t n_pairs,
                                  bool listed, uint32_t tol_int, uint32_t min_run, uint32_t rate_num, uint32_t rate_den, vdf_alignment_retimed *out,
                                  size_t capacity, size_t *n_out)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    uint32_t num = 1, den = 1;
    if (int rc = align_retimed_all_checks(ctx, name, a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first, b_first, pairs, n_pairs, listed, min_run, rate_num,
                                          rate_den, &num, &den, out, capacity, n_out, true))
        return rc;
    *n_out = 0;
    if (listed ? n_pairs == 0 : (n_a == 0 || n_b == 0)) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    AlignUploaded u;
    if (int rc = align_upload(ctx, a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip, false, s, &u)) return rc;
    return align_retimed_locked(ctx, align_sides_uploaded(ctx, u, n_a, n_b, false), tol_int, min_run, num, den, out, capacity, n_out, s,
                                listed ? pairs : nullptr, n_pairs);
}

int vdf_align_windows_retimed_host(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes,
                                   const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, uint32_t tol_int, uint32_t min_run, uint32_t rate_num,
                                   uint32_t rate_den, vdf_alignment_retimed *out, size_t capacity, size_t *n_out)
{
    return align_retimed_host_impl(a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip, nullptr, 0, false, tol_int, min_run, rate_num, rate_den, out,
                                   capacity, n_out);
}

int vdf_align_windows_retimed(vdf_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes,
                              const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, uint32_t tol_int, uint32_t min_run, uint32_t rate_num,
                              uint32_t rate_den, vdf_alignment_retimed *out, size_t capacity, size_t *n_out)
{
    return align_retimed_ctx_impl(ctx, "vdf_align_windows_retimed", a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip, nullptr, 0, false, tol_int,
                                  min_run, rate_num, rate_den, out, capacity, n_out);
}

int vdf_align_windows_retimed_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a, const uint8_t *d_a_skip,
                                     const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b, const uint8_t *d_b_skip, uint32_t tol_int,
                                     uint32_t min_run, uint32_t rate_num, uint32_t rate_den, vdf_alignment_retimed *out, size_t capacity, size_t *n_out,
                                     void *stream)
{
    return align_retimed_device_impl(ctx, "vdf_align_windows_retimed_device", d_a_hashes, d_a_first, n_a, d_a_skip, d_b_hashes, d_b_first, n_b, d_b_skip, nullptr,
                                     0, false, tol_int, min_run, rate_num, rate_den, out, capacity, n_out, stream);
}

int vdf_align_windows_retimed_pairs_host(const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes,
                                         const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, const vdf_video_pair *pairs, size_t n_pairs,
                                         uint32_t tol_int, uint32_t min_run, uint32_t rate_num, uint32_t rate_den, vdf_alignment_retimed *out,
                                         size_t capacity, size_t *n_out)
{
    return align_retimed_host_impl(a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip, pairs, n_pairs, true, tol_int, min_run, rate_num, rate_den,
                                   out, capacity, n_out);
}

int vdf_align_windows_retimed_pairs(vdf_ctx *ctx, const uint64_t *a_hashes, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                    const uint64_t *b_hashes, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, const vdf_video_pair *pairs,
                                    size_t n_pairs, uint32_t tol_int, uint32_t min_run, uint32_t rate_num, uint32_t rate_den, vdf_alignment_retimed *out,
                                    size_t capacity, size_t *n_out)
{
    return align_retimed_ctx_impl(ctx, "vdf_align_windows_retimed_pairs", a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip, pairs, n_pairs, true,
                                  tol_int, min_run, rate_num, rate_den, out, capacity, n_out);
}

int vdf_align_windows_retimed_pairs_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, size_t n_a, const uint8_t *d_a_skip,
                                           const uint64_t *d_b_hashes, const uint32_t *d_b_first, size_t n_b, const uint8_t *d_b_skip,
                                           const vdf_video_pair *pairs, size_t n_pairs, uint32_t tol_int, uint32_t min_run, uint32_t rate_num,
                                           uint32_t rate_den, vdf_alignment_retimed *out, size_t capacity, size_t *n_out, void *stream)
{
    return align_retimed_device_impl(ctx, "vdf_align_windows_retimed_pairs_device", d_a_hashes, d_a_first, n_a, d_a_skip, d_b_hashes, d_b_first, n_b, d_b_skip,
                                     pairs, n_pairs, true, tol_int, min_run, rate_num, rate_den, out, capacity, n_out, stream);
}

// ---- the retimed alignment, seeded: every phase of up to 8 rates from one pass (include/vdf.h: vdf_align_seed_pairs_rates*; DESIGN.md 4.22;
// align_seed_rates_plan.h) --------------------------------------------------------------------------------------------------------------------
// The checks of the three forms, in the header's order: align_checks' kinds, each on B first and then on the blocks of A; then the rate list,
// exclude_same, the context.  First arrays on the host, or null (the device form before they have come down).  rates: the list in lowest terms.
static int seed_rates_checks(vdf_ctx *ctx, const char *name, const vdf_align_seed_rates_job *j, const uint32_t *a_first, const uint32_t *b_first,
                             vdf::AlignSeedRate *rates, bool ctx_check = true)  // false: vdf_align_windows_rates*, whose list checks come before the context's
{
    const size_t n_a = j->n_a, n_b = j->n_b;
    const uint32_t n_blocks = std::min<uint32_t>(j->n_rates, VDF_WINDOWS_MAX_RATES);
    if (!j->n_out || (j->capacity && !j->out) || (n_b && (!j->b_hashes || !j->b_first)) || (n_a && (!j->a_hashes || !j->a_first)))
        return fail(ctx, VDF_E_INVAL, "null pointer");
    if (j->min_run == 0) return fail(ctx, VDF_E_INVAL, "min_run of zero");
    const auto block = [&](uint32_t r) { return a_first + (size_t)r * (n_a + 1); };
    for (size_t v = 0; b_first && v < n_b; v++)
        if (b_first[v + 1] >= b_first[v] && b_first[v + 1] - b_first[v] > vdf::kAlignMaxWindows)
            return fail(ctx, VDF_E_INVAL, "video " + std::to_string(v) + " of B has more than 2^20 windows");
    for (uint32_t r = 0; a_first && r < n_blocks; r++)
        for (size_t v = 0; v < n_a; v++)
            if (block(r)[v + 1] >= block(r)[v] && block(r)[v + 1] - block(r)[v] > vdf::kAlignMaxWindows)
                return fail(ctx, VDF_E_INVAL, "video " + std::to_string(v) + " of A has more than 2^20 windows at rate " + std::to_string(r));
    for (size_t v = 0; b_first && v < n_b; v++)
        if (b_first[v + 1] < b_first[v]) return fail(ctx, VDF_E_INVAL, "the first array of B decreases at video " + std::to_string(v));
    for (uint32_t r = 0; a_first && r < n_blocks; r++)
        for (size_t v = 0; v < n_a; v++)
            if (block(r)[v + 1] < block(r)[v])
                return fail(ctx, VDF_E_INVAL, "the first array of A decreases at video " + std::to_string(v) + " of rate " + std::to_string(r));
    for (uint32_t r = 0; a_first && n_a && r < n_blocks; r++) {
        const uint64_t base = j->a_rate_first ? (uint64_t)j->a_rate_first[r] : 0ull;
        if (base > 0xFFFFFFFFull || base + block(r)[n_a] > 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "2^32 rows of A or more");
    }
    if (n_a > 0xFFFFFFFFull || n_b > 0xFFFFFFFFull || (uint64_t)n_a * n_b > vdf::kAlignMaxPairs)
        return fail(ctx, VDF_E_INVAL, "more than 2^24 pairs of videos in one call");
    if (j->n_rates < 1 || j->n_rates > VDF_WINDOWS_MAX_RATES || !j->rate_num || !j->rate_den)
        return fail(ctx, VDF_E_INVAL, "n_rates outside 1 ... 8 or a null rate array");
    int worst = 0;
    for (uint32_t r = 0; r < j->n_rates; r++) {
        const int rc = vdf::align_retimed_rate(j->rate_num[r], j->rate_den[r], &rates[r].num, &rates[r].den);
        if (rc == 1) return fail(ctx, VDF_E_INVAL, "rate " + std::to_string(r) + " must have 1 <= den <= num <= 2 den");
        if (rc == 2 && !worst) worst = (int)r + 1;
    }
    if (worst) return fail(ctx, VDF_E_INVAL, "the num of rate " + std::to_string(worst - 1) + " is above 32 in lowest terms (VDF_ALIGN_RETIMED_MAX_NUM)");
    if (j->exclude_same && n_a != n_b) return fail(ctx, VDF_E_INVAL, "exclude_same takes n_a == n_b");
    if (ctx_check && ctx && !ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, std::string(name) + " takes a single-device context");
    return VDF_OK;
}

int vdf_align_seed_pairs_rates_host(const vdf_align_seed_rates_job *j)
{
    if (!j) return VDF_E_INVAL;
    vdf::AlignSeedRate rates[VDF_WINDOWS_MAX_RATES];
    if (int rc = seed_rates_checks(nullptr, "vdf_align_seed_pairs_rates_host", j, j->a_first, j->b_first, rates)) return rc;
    *j->n_out = 0;
    if (j->n_a == 0 || j->n_b == 0) return VDF_OK;
    const uint32_t tol = std::min<uint32_t>(j->tol_int, 1024u);
    size_t found = 0;
    // the literal definition: every seed of a under r against every row of b under r, XOR + popcount
    for (uint32_t r = 0; r < j->n_rates; r++) {
        const uint32_t *fa = j->a_first + (size_t)r * (j->n_a + 1);
        const size_t base = j->a_rate_first ? j->a_rate_first[r] : 0;
        for (size_t a = 0; a < j->n_a; a++)
            for (size_t b = 0; b < j->n_b; b++) {
                if (j->exclude_same && a == b) continue;
                const uint32_t Na = fa[a + 1] - fa[a], Nb = j->b_first[b + 1] - j->b_first[b];
                bool hit = false;
                for (uint32_t ka = 0; ka < Na && !hit; ka++) {
                    const size_t ra = base + fa[a] + ka;
                    if (!vdf::align_seed_rates_is_seed(ka, rates[r].num, j->min_run) || (j->a_skip && j->a_skip[ra])) continue;
                    for (uint64_t kb = 0; kb < Nb && !hit; kb += rates[r].den) {
                        const size_t rb = (size_t)j->b_first[b] + kb;
                        if (j->b_skip && j->b_skip[rb]) continue;
                        uint32_t dist = 0;
                        for (int w = 0; w < VDF_HASH_WORDS; w++) dist += (uint32_t)__builtin_popcountll(j->a_hashes[16 * ra + w] ^ j->b_hashes[16 * rb + w]);
                        hit = dist <= tol;
                    }
                }
                if (!hit) continue;
                if (found < j->capacity) j->out[found] = vdf_video_pair_rate{(uint32_t)a, (uint32_t)b, r};
                found++;
            }
    }
    *j->n_out = found;
    return VDF_OK;
}

// the checks have passed on the host copies of the first arrays; the hashes and skip bytes are device pointers whose row 0 is row a_shift /
// b_shift of the caller's arrays.  The plan goes up in one piece, the bitmap is cleared on the call's stream, the seed kernel marks it,
// count + scan give the total; the host reads it, then the first min(total, capacity) triples.  all (nullable): the internal entry of
// vdf_align_windows_rates* - the job's out, capacity and n_out are not touched, and ALL triples come down into *all, which grows to the total.
static int align_seed_rates_locked(vdf_ctx *ctx, const vdf_align_seed_rates_job *j, const vdf::AlignSeedRate *rates, const uint64_t *d_a_hashes,
                                   const uint8_t *d_a_skip, const uint32_t *h_first_a, uint64_t a_shift, const uint64_t *d_b_hashes, const uint8_t *d_b_skip,
                                   const uint32_t *h_first_b, uint64_t b_shift, hipStream_t s, std::vector<vdf_video_pair_rate> *all = nullptr)
{
    if (all) all->clear();
    vdf::AlignSeedRatesPlan plan;
    vdf::align_seed_rates_plan(h_first_a, j->a_rate_first, j->n_a, h_first_b, j->n_b, rates, j->n_rates, j->min_run, a_shift, b_shift, plan);
    if (plan.n_units() == 0) return VDF_OK;  // no seed or no row of B
    const uint64_t n_bits = (uint64_t)j->n_rates * j->n_a * j->n_b;  // <= 2^27: the checks
    const uint32_t n_words = (uint32_t)((n_bits + 31) / 32);
    const size_t n_seeds = plan.n_seeds(), n_rows = plan.row_window.size(), n_chunks = plan.n_chunks();
    // one upload, in dwords: seed_window | seed_video | seed_slot | row_window | row_video | chunk_first | tile_first | (pad) | unit_offset
    const size_t at_video = n_seeds, at_slot = 2 * n_seeds, at_row = 3 * n_seeds, at_rvid = at_row + n_rows, at_chunk = at_rvid + n_rows;
    const size_t at_tile = at_chunk + n_chunks + 1, at_unit = (at_tile + n_chunks + 1) & ~(size_t)1, n_dwords = at_unit + 2 * (n_chunks + 1);
    std::vector<uint32_t> blob(n_dwords, 0u);
    std::copy(plan.seed_window.begin(), plan.seed_window.end(), blob.begin());
    std::copy(plan.seed_video.begin(), plan.seed_video.end(), blob.begin() + at_video);
    std::copy(plan.seed_slot.begin(), plan.seed_slot.end(), blob.begin() + at_slot);
    std::copy(plan.row_window.begin(), plan.row_window.end(), blob.begin() + at_row);
    std::copy(plan.row_video.begin(), plan.row_video.end(), blob.begin() + at_rvid);
    std::copy(plan.chunk_first.begin(), plan.chunk_first.end(), blob.begin() + at_chunk);
    std::copy(plan.tile_first.begin(), plan.tile_first.end(), blob.begin() + at_tile);
    std::memcpy(blob.data() + at_unit, plan.unit_offset.data(), (n_chunks + 1) * 8);
    VDF_HIP(ctx, ctx->seed_bitmap.reserve((size_t)n_words * 4));
    VDF_HIP(ctx, ctx->seed_plan.reserve(n_dwords * 4));
    VDF_HIP(ctx, ctx->align_scratch.reserve(vdf::align_seed_scratch_bytes(n_words)));
    const uint32_t *dp = ctx->seed_plan.as<uint32_t>();
    VDF_HIP(ctx, hipMemsetAsync(ctx->seed_bitmap.p, 0, (size_t)n_words * 4, s));
    VDF_HIP(ctx, hipMemcpyAsync(ctx->seed_plan.p, blob.data(), n_dwords * 4, hipMemcpyHostToDevice, s));
    uint32_t *d_total = nullptr;
    vdf::AlignSeedRatesLaunch L{};
    L.a_hashes = reinterpret_cast<const uint32_t *>(d_a_hashes); L.a_skip = d_a_skip;
    L.seed_window = dp; L.seed_video = dp + at_video; L.seed_slot = dp + at_slot; L.chunk_first = dp + at_chunk;
    L.b_hashes = reinterpret_cast<const uint32_t *>(d_b_hashes); L.b_skip = d_b_skip;
    L.row_window = dp + at_row; L.row_video = dp + at_rvid;
    L.unit_offset = reinterpret_cast<const unsigned long long *>(dp + at_unit); L.tile_first = dp + at_tile;
    L.n_chunks = (uint32_t)n_chunks; L.n_units = plan.n_units();
    L.tol = std::min<uint32_t>(j->tol_int, 1024u); L.exclude_same = j->exclude_same ? 1 : 0;
    L.n_slots = j->n_rates; L.n_a = (uint32_t)j->n_a; L.n_b = (uint32_t)j->n_b;
    L.bitmap = ctx->seed_bitmap.as<uint32_t>(); L.n_words = n_words;
    L.scratch = ctx->align_scratch.p; L.total_out = &d_total;
    VDF_HIP(ctx, vdf::launch_align_seed_rates(L, s));
    uint32_t total = 0;
    VDF_HIP(ctx, hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipStreamSynchronize(s));  // also: the plan is free to go
    if ((uint64_t)total > n_bits) return fail(ctx, VDF_E_HIP, "align seed rates: more triples than bits");
    const size_t take = all ? (size_t)total : std::min<size_t>(total, j->capacity);
    if (all) all->resize(take);
    if (take) {
        VDF_HIP(ctx, ctx->seed_out.reserve(take * sizeof(vdf_video_pair_rate)));
        VDF_HIP(ctx, vdf::launch_align_seed_rates_scatter(L, ctx->seed_out.as<vdf_video_pair_rate>(), (uint32_t)take, s));
        VDF_HIP(ctx, hipMemcpyAsync(all ? all->data() : j->out, ctx->seed_out.p, take * sizeof(vdf_video_pair_rate), hipMemcpyDeviceToHost, s));
        VDF_HIP(ctx, hipStreamSynchronize(s));
    }
    if (!all) *j->n_out = total;
    return VDF_OK;
}

int vdf_align_seed_pairs_rates_device(vdf_ctx *ctx, const vdf_align_seed_rates_job *j)
{
    if (!ctx || !j) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    vdf::AlignSeedRate rates[VDF_WINDOWS_MAX_RATES];
    // everything that can be said without the first arrays - the multi-GPU refusal last; then they come down and are checked
    if (int rc = seed_rates_checks(ctx, "vdf_align_seed_pairs_rates_device", j, nullptr, nullptr, rates)) return rc;
    *j->n_out = 0;
    if (j->n_a == 0 || j->n_b == 0) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = j->stream ? (hipStream_t)j->stream : ctx->stream;
    std::vector<uint32_t> fa((size_t)j->n_rates * (j->n_a + 1)), fb(j->n_b + 1);
    VDF_HIP(ctx, hipMemcpyAsync(fa.data(), j->a_first, fa.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipMemcpyAsync(fb.data(), j->b_first, fb.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipStreamSynchronize(s));
    if (int rc = seed_rates_checks(ctx, "vdf_align_seed_pairs_rates_device", j, fa.data(), fb.data(), rates)) return rc;
    return align_seed_rates_locked(ctx, j, rates, j->a_hashes, j->a_skip, fa.data(), 0, j->b_hashes, j->b_skip, fb.data(), 0, s);
}

// Host arrays: the rows of A that the blocks span and the rows of B go up once through the context's staging buffers, the skip bytes beside
// them; the device form's core runs on them.
int vdf_align_seed_pairs_rates(vdf_ctx *ctx, const vdf_align_seed_rates_job *j)
{
    if (!ctx || !j) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    vdf::AlignSeedRate rates[VDF_WINDOWS_MAX_RATES];
    if (int rc = seed_rates_checks(ctx, "vdf_align_seed_pairs_rates", j, j->a_first, j->b_first, rates)) return rc;
    *j->n_out = 0;
    if (j->n_a == 0 || j->n_b == 0) return VDF_OK;
    uint64_t a_lo = ~0ull, a_hi = 0;
    for (uint32_t r = 0; r < j->n_rates; r++) {
        const uint32_t *fa = j->a_first + (size_t)r * (j->n_a + 1);
        const uint64_t base = j->a_rate_first ? (uint64_t)j->a_rate_first[r] : 0ull;
        a_lo = std::min(a_lo, base + fa[0]);
        a_hi = std::max(a_hi, base + fa[j->n_a]);
    }
    const uint64_t b_lo = j->b_first[0], b_hi = j->b_first[j->n_b];
    const size_t wa = (size_t)(a_hi - a_lo), wb = (size_t)(b_hi - b_lo);
    if (wa == 0 || wb == 0) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t ska = j->a_skip ? (wa + 3) & ~(size_t)3 : 0, skb = j->b_skip ? wb : 0;
    VDF_HIP(ctx, ctx->align_up.reserve(ska + skb + 16));
    char *up = ctx->align_up.as<char>();
    if (ska) VDF_HIP(ctx, hipMemcpyAsync(up, j->a_skip + a_lo, wa, hipMemcpyHostToDevice, s));
    if (skb) VDF_HIP(ctx, hipMemcpyAsync(up + ska, j->b_skip + b_lo, wb, hipMemcpyHostToDevice, s));
    if (int rc = upload(ctx, ctx->up_hashes, j->a_hashes + 16 * (size_t)a_lo, wa * 16 * sizeof(uint64_t), s)) return rc;
    if (int rc = upload(ctx, ctx->up_ref_hashes, j->b_hashes + 16 * (size_t)b_lo, wb * 16 * sizeof(uint64_t), s)) return rc;
    return align_seed_rates_locked(ctx, j, rates, ctx->up_hashes.as<uint64_t>(), ska ? reinterpret_cast<const uint8_t *>(up) : nullptr, j->a_first, a_lo,
                                   ctx->up_ref_hashes.as<uint64_t>(), skb ? reinterpret_cast<const uint8_t *>(up + ska) : nullptr, j->b_first, b_lo, s);
}

// ---- retimed windows aligned at up to 8 rates in one call: (rate, a, b) triples (include/vdf.h: vdf_align_windows_rates*; DESIGN.md 4.23;
// align_rates_plan.h) ---------------------------------------------------------------------------------------------------------------------------
// the seed job on an align job's arguments: same arrays, same rates, same tol / min_run / exclude_same; out is only tested for null
static vdf_align_seed_rates_job align_rates_seed_job(const vdf_align_rates_job *j)
{
    vdf_align_seed_rates_job q{};
    q.a_hashes = j->a_hashes; q.a_first = j->a_first; q.a_rate_first = j->a_rate_first; q.a_skip = j->a_skip; q.n_a = j->n_a;
    q.b_hashes = j->b_hashes; q.b_first = j->b_first; q.b_skip = j->b_skip; q.n_b = j->n_b;
    q.n_rates = j->n_rates; q.rate_num = j->rate_num; q.rate_den = j->rate_den;
    q.tol_int = j->tol_int; q.min_run = j->min_run; q.exclude_same = j->exclude_same;
    q.out = reinterpret_cast<vdf_video_pair_rate *>(j->out); q.capacity = j->capacity; q.n_out = j->n_out; q.stream = j->stream;
    return q;
}

// The checks of the three forms, in the header's order: the seed call's up to and including the rate list and exclude_same (first arrays on the
// host, or null: the device form before they have come down), a list together with seed or exclude_same, the list, the context.
static int align_rates_checks(vdf_ctx *ctx, const char *name, const vdf_align_rates_job *j, const uint32_t *a_first, const uint32_t *b_first,
                              vdf::AlignSeedRate *rates)
{
    const vdf_align_seed_rates_job q = align_rates_seed_job(j);
    if (int rc = seed_rates_checks(ctx, name, &q, a_first, b_first, rates, false)) return rc;
    if (j->triples) {
        if (j->seed || j->exclude_same) return fail(ctx, VDF_E_INVAL, "a triple list together with seed or exclude_same");
        if (j->n_triples > vdf::kAlignRatesMaxTriples) return fail(ctx, VDF_E_INVAL, "more than 2^27 listed triples in one call");
        size_t at = 0;
        switch (vdf::align_rates_list_check(j->triples, j->n_triples, j->n_a, j->n_b, j->n_rates, &at)) {
        case 1: return fail(ctx, VDF_E_INVAL, "the triple list is not strictly increasing in (rate, a, b) at entry " + std::to_string(at));
        case 2: return fail(ctx, VDF_E_INVAL, "triple " + std::to_string(at) + " of the list names a video that does not exist");
        case 4: return fail(ctx, VDF_E_INVAL, "triple " + std::to_string(at) + " of the list names a rate that is not in the rate list");
        default: break;
        }
    }
    if (ctx && !ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, std::string(name) + " takes a single-device context");
    return VDF_OK;
}

int vdf_align_windows_rates_host(const vdf_align_rates_job *j)
{
    if (!j) return VDF_E_INVAL;
    vdf::AlignSeedRate rates[VDF_WINDOWS_MAX_RATES];
    if (int rc = align_rates_checks(nullptr, "vdf_align_windows_rates_host", j, j->a_first, j->b_first, rates)) return rc;
    *j->n_out = 0;
    if (j->n_a == 0 || j->n_b == 0 || (j->triples && j->n_triples == 0)) return VDF_OK;
    const uint32_t tol = std::min<uint32_t>(j->tol_int, 1024u);
    size_t found = 0;
    // vdf_align_windows_retimed_pairs_host's definition for the pair (a, b) on block r
    const auto triple = [&](uint32_t r, uint32_t a, uint32_t b) {
        const uint32_t *fa = j->a_first + (size_t)r * (j->n_a + 1);
        const size_t ra = (j->a_rate_first ? j->a_rate_first[r] : 0) + (size_t)fa[a], rb = j->b_first[b];
        vdf_alignment_retimed rec;
        align_retimed_pair_host(j->a_hashes + 16 * ra, fa[a + 1] - fa[a], j->a_skip ? j->a_skip + ra : nullptr, j->b_hashes + 16 * rb,
                                j->b_first[b + 1] - j->b_first[b], j->b_skip ? j->b_skip + rb : nullptr, rates[r].num, rates[r].den, tol, j->min_run, &rec);
        if (rec.n_windows == 0) return;
        if (found < j->capacity)
            j->out[found] = vdf_alignment_rate{a, b, r, rec.first_a, rec.first_b, rec.n_windows, rec.dist_sum, (rec.n_windows - 1) * rates[r].den + 16u};
        found++;
    };
    if (j->triples) {
        for (size_t i = 0; i < j->n_triples; i++) triple(j->triples[i].rate, j->triples[i].a, j->triples[i].b);
    } else if (j->seed) {
        std::vector<vdf_video_pair_rate> cand(1024);
        size_t n_cand = 0;
        vdf_align_seed_rates_job q = align_rates_seed_job(j);
        for (int pass = 0; pass < 2; pass++) {  // its own capacity growth: the second pass has room for everything the first one counted
            q.out = cand.data(); q.capacity = cand.size(); q.n_out = &n_cand;
            if (int rc = vdf_align_seed_pairs_rates_host(&q)) return rc;
            if (n_cand <= cand.size()) break;
            cand.resize(n_cand);
        }
        for (size_t i = 0; i < n_cand; i++) triple(cand[i].rate, cand[i].a, cand[i].b);
    } else {
        for (uint32_t r = 0; r < j->n_rates; r++)
            for (size_t a = 0; a < j->n_a; a++)
                for (size_t b = 0; b < j->n_b; b++)
                    if (!(j->exclude_same && a == b)) triple(r, (uint32_t)a, (uint32_t)b);
    }
    *j->n_out = found;
    return VDF_OK;
}

// The checks have passed on the host copies of the first arrays; hashes, skip bytes and first arrays are device pointers.  Row 0 of d_a_hashes /
// d_a_skip is row a_shift of the caller's arrays (a host-array call cuts off what no block uses); B's first arrays count from row 0 of d_b_hashes.
// seed: the candidates come from the seed pass on these same resident arrays (its internal entry: no second upload, all triples come down).
// Then the chunks: table | triples | unit_offset go up in one copy, the band walk, the reduction, the dense records down.
static int align_rates_locked(vdf_ctx *ctx, const vdf_align_rates_job *j, const vdf::AlignSeedRate *rates, const uint64_t *d_a_hashes, const uint8_t *d_a_skip,
                              const uint32_t *d_a_first, const uint32_t *h_first_a, uint64_t a_shift, const uint64_t *d_b_hashes, const uint8_t *d_b_skip,
                              const uint32_t *d_b_first, const uint32_t *h_first_b, hipStream_t s)
{
    std::vector<vdf_video_pair_rate> cand;
    const vdf_video_pair_rate *list = j->triples;
    size_t n_list = j->n_triples;
    if (!list && j->seed) {
        const vdf_align_seed_rates_job q = align_rates_seed_job(j);
        if (int rc = align_seed_rates_locked(ctx, &q, rates, d_a_hashes, d_a_skip, h_first_a, a_shift, d_b_hashes, d_b_skip, h_first_b, 0, s, &cand)) return rc;
        if (cand.empty()) return VDF_OK;
        list = cand.data();
        n_list = cand.size();
    }
    const vdf::AlignRatesTable table = vdf::align_rates_table(rates, j->n_rates, j->a_rate_first, j->n_a, a_shift);
    vdf::AlignRatesCursor cur;
    vdf::AlignRatesChunk ch;
    size_t found = 0, list_at = 0;
    while (list ? vdf::align_rates_next_chunk_triples(h_first_a, j->n_a, h_first_b, list, n_list, rates, list_at, ch)
                : vdf::align_rates_next_chunk(h_first_a, j->n_a, h_first_b, j->n_b, rates, j->n_rates, j->exclude_same != 0, cur, ch)) {
        const size_t n_triples = ch.n_triples(), n_units = ch.n_units(), plan_bytes = vdf::align_rates_plan_bytes(n_triples);
        VDF_HIP(ctx, ctx->align_plan.reserve(plan_bytes));
        VDF_HIP(ctx, ctx->align_scratch.reserve(vdf::align_rates_scratch_bytes(n_triples, n_units)));
        VDF_HIP(ctx, hipMemcpyAsync(ctx->align_plan.p, ch.seal(table), plan_bytes, hipMemcpyHostToDevice, s));  // the triples go up from where the planner wrote them
        vdf_alignment_rate *d_dense = nullptr;
        uint32_t *d_total = nullptr;
        vdf::AlignRatesLaunch L{};
        L.a_hashes = reinterpret_cast<const uint32_t *>(d_a_hashes); L.a_first = d_a_first; L.a_skip = d_a_skip;
        L.b_hashes = reinterpret_cast<const uint32_t *>(d_b_hashes); L.b_first = d_b_first; L.b_skip = d_b_skip;
        L.plan = ctx->align_plan.p;
        L.n_triples = (uint32_t)n_triples; L.n_units = (uint32_t)n_units;
        L.tol = std::min<uint32_t>(j->tol_int, 1024u); L.min_run = j->min_run;
        L.scratch = ctx->align_scratch.p; L.dense_out = &d_dense; L.total_out = &d_total;
        VDF_HIP(ctx, vdf::launch_align_rates_chunk(L, s));
        uint32_t total = 0;
        VDF_HIP(ctx, hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, s));
        VDF_HIP(ctx, hipStreamSynchronize(s));  // also: the chunk's plan is free to change
        if (total > n_triples) return fail(ctx, VDF_E_HIP, "align rates: more records than triples");
        const size_t room = j->capacity > found ? j->capacity - found : 0, take = std::min<size_t>(total, room);
        if (take) {
            VDF_HIP(ctx, hipMemcpyAsync(j->out + found, d_dense, take * sizeof(vdf_alignment_rate), hipMemcpyDeviceToHost, s));
            VDF_HIP(ctx, hipStreamSynchronize(s));
        }
        found += total;
    }
    *j->n_out = found;
    return VDF_OK;
}

int vdf_align_windows_rates_device(vdf_ctx *ctx, const vdf_align_rates_job *j)
{
    if (!ctx || !j) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    vdf::AlignSeedRate rates[VDF_WINDOWS_MAX_RATES];
    // everything that can be said without the first arrays - the multi-GPU refusal last; then they come down and are checked
    if (int rc = align_rates_checks(ctx, "vdf_align_windows_rates_device", j, nullptr, nullptr, rates)) return rc;
    *j->n_out = 0;
    if (j->n_a == 0 || j->n_b == 0 || (j->triples && j->n_triples == 0)) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = j->stream ? (hipStream_t)j->stream : ctx->stream;
    std::vector<uint32_t> fa((size_t)j->n_rates * (j->n_a + 1)), fb(j->n_b + 1);
    VDF_HIP(ctx, hipMemcpyAsync(fa.data(), j->a_first, fa.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipMemcpyAsync(fb.data(), j->b_first, fb.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipStreamSynchronize(s));
    if (int rc = align_rates_checks(ctx, "vdf_align_windows_rates_device", j, fa.data(), fb.data(), rates)) return rc;
    return align_rates_locked(ctx, j, rates, j->a_hashes, j->a_skip, j->a_first, fa.data(), 0, j->b_hashes, j->b_skip, j->b_first, fb.data(), s);
}

// Host arrays: the rows of A that the blocks span and the rows of B go up ONCE through the context's staging buffers, for the seed pass and the
// walk alike; beside them, in align_up, [first a | first b, rebased to the uploaded rows | skip a | skip b].
int vdf_align_windows_rates(vdf_ctx *ctx, const vdf_align_rates_job *j)
{
    if (!ctx || !j) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    vdf::AlignSeedRate rates[VDF_WINDOWS_MAX_RATES];
    if (int rc = align_rates_checks(ctx, "vdf_align_windows_rates", j, j->a_first, j->b_first, rates)) return rc;
    *j->n_out = 0;
    if (j->n_a == 0 || j->n_b == 0 || (j->triples && j->n_triples == 0)) return VDF_OK;
    uint64_t a_lo = ~0ull, a_hi = 0;
    for (uint32_t r = 0; r < j->n_rates; r++) {
        const uint32_t *fa = j->a_first + (size_t)r * (j->n_a + 1);
        const uint64_t base = j->a_rate_first ? (uint64_t)j->a_rate_first[r] : 0ull;
        a_lo = std::min(a_lo, base + fa[0]);
        a_hi = std::max(a_hi, base + fa[j->n_a]);
    }
    const uint64_t b_lo = j->b_first[0], b_hi = j->b_first[j->n_b];
    const size_t wa = (size_t)(a_hi - a_lo), wb = (size_t)(b_hi - b_lo);
    if (wa == 0 || wb == 0) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> fb(j->n_b + 1);
    for (size_t v = 0; v <= j->n_b; v++) fb[v] = j->b_first[v] - j->b_first[0];
    const size_t fa_bytes = (size_t)j->n_rates * (j->n_a + 1) * sizeof(uint32_t), fb_bytes = fb.size() * sizeof(uint32_t);
    const size_t ska = j->a_skip ? (wa + 3) & ~(size_t)3 : 0, skb = j->b_skip ? wb : 0;
    VDF_HIP(ctx, ctx->align_up.reserve(fa_bytes + fb_bytes + ska + skb + 16));
    char *up = ctx->align_up.as<char>();
    VDF_HIP(ctx, hipMemcpyAsync(up, j->a_first, fa_bytes, hipMemcpyHostToDevice, s));
    VDF_HIP(ctx, hipMemcpyAsync(up + fa_bytes, fb.data(), fb_bytes, hipMemcpyHostToDevice, s));
    if (ska) VDF_HIP(ctx, hipMemcpyAsync(up + fa_bytes + fb_bytes, j->a_skip + a_lo, wa, hipMemcpyHostToDevice, s));
    if (skb) VDF_HIP(ctx, hipMemcpyAsync(up + fa_bytes + fb_bytes + ska, j->b_skip + b_lo, wb, hipMemcpyHostToDevice, s));
    if (int rc = upload(ctx, ctx->up_hashes, j->a_hashes + 16 * (size_t)a_lo, wa * 16 * sizeof(uint64_t), s)) return rc;
    if (int rc = upload(ctx, ctx->up_ref_hashes, j->b_hashes + 16 * (size_t)b_lo, wb * 16 * sizeof(uint64_t), s)) return rc;
    return align_rates_locked(ctx, j, rates, ctx->up_hashes.as<uint64_t>(), ska ? reinterpret_cast<const uint8_t *>(up + fa_bytes + fb_bytes) : nullptr,
                              reinterpret_cast<const uint32_t *>(up), j->a_first, a_lo, ctx->up_ref_hashes.as<uint64_t>(),
                              skb ? reinterpret_cast<const uint8_t *>(up + fa_bytes + fb_bytes + ska) : nullptr,
                              reinterpret_cast<const uint32_t *>(up + fa_bytes), fb.data(), s);
}

// ---- every stretch of a retimed pair, ranked, at up to 8 rates in one call (include/vdf.h: vdf_align_windows_rates_stretches*; DESIGN.md 4.24;
// align_rates_stretch_plan.h) -------------------------------------------------------------------------------------------------------------------
// the align job on a stretches job's arguments: same arrays, rates, tol / min_run, triple mode; out is only tested for null
static vdf_align_rates_job align_rates_stretches_plain_job(const vdf_align_rates_stretches_job *j)
{
    vdf_align_rates_job q{};
    q.a_hashes = j->a_hashes; q.a_first = j->a_first; q.a_rate_first = j->a_rate_first; q.a_skip = j->a_skip; q.n_a = j->n_a;
    q.b_hashes = j->b_hashes; q.b_first = j->b_first; q.b_skip = j->b_skip; q.n_b = j->n_b;
    q.n_rates = j->n_rates; q.rate_num = j->rate_num; q.rate_den = j->rate_den;
    q.tol_int = j->tol_int; q.min_run = j->min_run; q.triples = j->triples; q.n_triples = j->n_triples; q.seed = j->seed; q.exclude_same = j->exclude_same;
    q.out = reinterpret_cast<vdf_alignment_rate *>(j->out); q.capacity = j->capacity; q.n_out = j->n_out; q.stream = j->stream;
    return q;
}

// The checks of the three forms, in the header's order: those of vdf_align_windows_rates* up to and including the list (first arrays on the host,
// or null: the device form before they have come down), max_stretches, guard, the context.
static int align_rates_stretches_checks(vdf_ctx *ctx, const char *name, const vdf_align_rates_stretches_job *sj, const uint32_t *a_first, const uint32_t *b_first,
                                        vdf::AlignSeedRate *rates)
{
    const vdf_align_rates_job j = align_rates_stretches_plain_job(sj);
    const vdf_align_seed_rates_job q = align_rates_seed_job(&j);
    if (int rc = seed_rates_checks(ctx, name, &q, a_first, b_first, rates, false)) return rc;
    if (j.triples) {
        if (j.seed || j.exclude_same) return fail(ctx, VDF_E_INVAL, "a triple list together with seed or exclude_same");
        if (j.n_triples > vdf::kAlignRatesMaxTriples) return fail(ctx, VDF_E_INVAL, "more than 2^27 listed triples in one call");
        size_t at = 0;
        switch (vdf::align_rates_list_check(j.triples, j.n_triples, j.n_a, j.n_b, j.n_rates, &at)) {
        case 1: return fail(ctx, VDF_E_INVAL, "the triple list is not strictly increasing in (rate, a, b) at entry " + std::to_string(at));
        case 2: return fail(ctx, VDF_E_INVAL, "triple " + std::to_string(at) + " of the list names a video that does not exist");
        case 4: return fail(ctx, VDF_E_INVAL, "triple " + std::to_string(at) + " of the list names a rate that is not in the rate list");
        default: break;
        }
    }
    if (int rc = align_stretches_checks(ctx, sj->max_stretches, sj->guard)) return rc;
    if (ctx && !ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, std::string(name) + " takes a single-device context");
    return VDF_OK;
}

static vdf_alignment_rate_stretch rate_stretch_of(const vdf_alignment_rate &r, uint32_t rank)
{
    return vdf_alignment_rate_stretch{r.a, r.b, r.rate, r.first_a, r.first_b, r.n_windows, r.dist_sum, r.n_frames_b, rank};
}

int vdf_align_windows_rates_stretches_host(const vdf_align_rates_stretches_job *sj)
{
    if (!sj) return VDF_E_INVAL;
    vdf::AlignSeedRate rates[VDF_WINDOWS_MAX_RATES];
    if (int rc = align_rates_stretches_checks(nullptr, "vdf_align_windows_rates_stretches_host", sj, sj->a_first, sj->b_first, rates)) return rc;
    const vdf_align_rates_job plain = align_rates_stretches_plain_job(sj), *j = &plain;
    *j->n_out = 0;
    if (j->n_a == 0 || j->n_b == 0 || (j->triples && j->n_triples == 0)) return VDF_OK;
    const uint32_t tol = std::min<uint32_t>(j->tol_int, 1024u);
    size_t found = 0;
    // the definition for one triple: rank k on the matrix masked by the rectangles of ranks 0 ... k - 1
    const auto triple = [&](uint32_t r, uint32_t a, uint32_t b) {
        const uint32_t *fa = j->a_first + (size_t)r * (j->n_a + 1);
        const size_t ra = (j->a_rate_first ? j->a_rate_first[r] : 0) + (size_t)fa[a], rb = j->b_first[b];
        const uint32_t Na = fa[a + 1] - fa[a], Nb = j->b_first[b + 1] - j->b_first[b];
        vdf::AlignRect rects[vdf::kAlignMaxStretches];
        for (uint32_t rank = 0; rank < sj->max_stretches; rank++) {
            vdf_alignment_retimed rec;
            align_retimed_pair_masked_host(j->a_hashes + 16 * ra, Na, j->a_skip ? j->a_skip + ra : nullptr, j->b_hashes + 16 * rb, Nb,
                                           j->b_skip ? j->b_skip + rb : nullptr, rates[r].num, rates[r].den, tol, j->min_run, rects, rank, &rec);
            if (rec.n_windows == 0) return;
            if (found < sj->capacity)
                sj->out[found] = vdf_alignment_rate_stretch{a, b, r, rec.first_a, rec.first_b, rec.n_windows, rec.dist_sum, (rec.n_windows - 1) * rates[r].den + 16u, rank};
            found++;
            rects[rank] = vdf::align_rates_rect_of(rec.first_a, rec.first_b, rec.n_windows, rates[r].num, rates[r].den, sj->guard, Na, Nb);
        }
    };
    if (j->triples) {
        for (size_t i = 0; i < j->n_triples; i++) triple(j->triples[i].rate, j->triples[i].a, j->triples[i].b);
    } else if (j->seed) {
        std::vector<vdf_video_pair_rate> cand(1024);
        size_t n_cand = 0;
        vdf_align_seed_rates_job q = align_rates_seed_job(j);
        for (int pass = 0; pass < 2; pass++) {  // its own capacity growth: the second pass has room for everything the first one counted
            q.out = cand.data(); q.capacity = cand.size(); q.n_out = &n_cand;
            if (int rc = vdf_align_seed_pairs_rates_host(&q)) return rc;
            if (n_cand <= cand.size()) break;
            cand.resize(n_cand);
        }
        for (size_t i = 0; i < n_cand; i++) triple(cand[i].rate, cand[i].a, cand[i].b);
    } else {
        for (uint32_t r = 0; r < j->n_rates; r++)
            for (size_t a = 0; a < j->n_a; a++)
                for (size_t b = 0; b < j->n_b; b++)
                    if (!(j->exclude_same && a == b)) triple(r, (uint32_t)a, (uint32_t)b);
    }
    *sj->n_out = found;
    return VDF_OK;
}

// one round of a chunk: the round's one upload, the band walk (masked from round 1 on) and the reductions; *total = the round's records, of
// which the first min(*total, limit) come down into recs
static int align_rates_run_round(vdf_ctx *ctx, vdf::AlignRatesLaunch L, vdf::AlignRatesRound &round, const vdf::AlignRatesTable &table, size_t limit,
                                 std::vector<vdf_alignment_rate> &recs, uint32_t *total, hipStream_t s)
{
    const size_t n_triples = round.chunk.n_triples(), n_units = round.chunk.n_units();
    const size_t plan_bytes = vdf::align_rates_round_plan_bytes(n_triples, round.n_rects);
    VDF_HIP(ctx, ctx->align_plan.reserve(plan_bytes));
    VDF_HIP(ctx, ctx->align_scratch.reserve(vdf::align_rates_scratch_bytes(n_triples, n_units)));
    VDF_HIP(ctx, hipMemcpyAsync(ctx->align_plan.p, vdf::align_rates_round_seal(round, table), plan_bytes, hipMemcpyHostToDevice, s));
    vdf_alignment_rate *d_dense = nullptr;
    uint32_t *d_total = nullptr;
    L.plan = ctx->align_plan.p;
    L.n_triples = (uint32_t)n_triples; L.n_units = (uint32_t)n_units;
    L.scratch = ctx->align_scratch.p; L.dense_out = &d_dense; L.total_out = &d_total;
    if (round.n_rects) VDF_HIP(ctx, vdf::launch_align_rates_masked_chunk(L, round.n_rects, s));
    else VDF_HIP(ctx, vdf::launch_align_rates_chunk(L, s));
    *total = 0;
    VDF_HIP(ctx, hipMemcpyAsync(total, d_total, sizeof(*total), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipStreamSynchronize(s));  // also: the round's plan is free to change
    if (*total > n_triples) return fail(ctx, VDF_E_HIP, "align rates: more records than triples");
    recs.resize(std::min<size_t>(*total, limit));
    if (!recs.empty()) {
        VDF_HIP(ctx, hipMemcpyAsync(recs.data(), d_dense, recs.size() * sizeof(vdf_alignment_rate), hipMemcpyDeviceToHost, s));
        VDF_HIP(ctx, hipStreamSynchronize(s));
    }
    return VDF_OK;
}

// align_rates_locked with rounds.  Per chunk: round 0 is the plain launch; round k walks the masked kernel on the triples that had a record in
// round k - 1 (align_rates_stretch_plan.h), until a round has no record or max_stretches rounds have run; the rounds are merged into (rate, a, b,
// rank) order.  Chunks arrive in (rate, a, b) order and each is finished before the next, so the first `capacity` records of the call are the ones
// written.  The seed pass runs once, in front of everything.  The rank is added here, on the host: the rounds scatter vdf_alignment_rate records.
static int align_rates_stretches_locked(vdf_ctx *ctx, const vdf_align_rates_stretches_job *sj, const vdf::AlignSeedRate *rates, const uint64_t *d_a_hashes,
                                        const uint8_t *d_a_skip, const uint32_t *d_a_first, const uint32_t *h_first_a, uint64_t a_shift, const uint64_t *d_b_hashes,
                                        const uint8_t *d_b_skip, const uint32_t *d_b_first, const uint32_t *h_first_b, hipStream_t s)
{
    const vdf_align_rates_job plain = align_rates_stretches_plain_job(sj), *j = &plain;
    std::vector<vdf_video_pair_rate> cand;
    const vdf_video_pair_rate *list = j->triples;
    size_t n_list = j->n_triples;
    if (!list && j->seed) {
        const vdf_align_seed_rates_job q = align_rates_seed_job(j);
        if (int rc = align_seed_rates_locked(ctx, &q, rates, d_a_hashes, d_a_skip, h_first_a, a_shift, d_b_hashes, d_b_skip, h_first_b, 0, s, &cand)) return rc;
        if (cand.empty()) return VDF_OK;
        list = cand.data();
        n_list = cand.size();
    }
    const vdf::AlignRatesTable table = vdf::align_rates_table(rates, j->n_rates, j->a_rate_first, j->n_a, a_shift);
    vdf::AlignRatesLaunch L{};
    L.a_hashes = reinterpret_cast<const uint32_t *>(d_a_hashes); L.a_first = d_a_first; L.a_skip = d_a_skip;
    L.b_hashes = reinterpret_cast<const uint32_t *>(d_b_hashes); L.b_first = d_b_first; L.b_skip = d_b_skip;
    L.tol = std::min<uint32_t>(j->tol_int, 1024u); L.min_run = j->min_run;
    vdf::AlignRatesCursor cur;
    vdf::AlignRatesRound round, next;
    std::vector<std::vector<vdf_alignment_rate>> rounds;
    size_t found = 0, list_at = 0;
    while (list ? vdf::align_rates_next_chunk_triples(h_first_a, j->n_a, h_first_b, list, n_list, rates, list_at, round.chunk)
                : vdf::align_rates_next_chunk(h_first_a, j->n_a, h_first_b, j->n_b, rates, j->n_rates, j->exclude_same != 0, cur, round.chunk)) {
        round.rects.clear();
        round.n_rects = 0;
        rounds.clear();
        size_t uncopied = 0;  // max_stretches == 1: the records behind the capacity are counted, not fetched
        for (uint32_t r = 0;; r++) {
            rounds.emplace_back();
            uint32_t total = 0;
            const bool last = r + 1 >= sj->max_stretches;
            const size_t room = sj->capacity > found ? sj->capacity - found : 0;
            if (int rc = align_rates_run_round(ctx, L, round, table, last && r == 0 ? room : ~(size_t)0, rounds.back(), &total, s)) return rc;
            uncopied = total - rounds.back().size();
            if (!vdf::align_rates_more_rounds(r, total, sj->max_stretches)) break;
            if (!vdf::align_rates_next_round(round, rounds.back().data(), rounds.back().size(), h_first_a, j->n_a, h_first_b, rates, sj->guard, next))
                return fail(ctx, VDF_E_HIP, "align rates: a round's records do not belong to its triples");
            std::swap(round, next);
        }
        std::vector<size_t> at(rounds.size(), 0);
        for (const vdf_alignment_rate &r0 : rounds[0]) {
            if (found < sj->capacity) sj->out[found] = rate_stretch_of(r0, 0);
            found++;
            for (size_t r = 1; r < rounds.size(); r++) {
                if (at[r] == rounds[r].size()) break;
                const vdf_alignment_rate &x = rounds[r][at[r]];
                if (x.rate != r0.rate || x.a != r0.a || x.b != r0.b) break;
                if (found < sj->capacity) sj->out[found] = rate_stretch_of(x, (uint32_t)r);
                found++;
                at[r]++;
            }
        }
        found += uncopied;
    }
    *sj->n_out = found;
    return VDF_OK;
}

int vdf_align_windows_rates_stretches_device(vdf_ctx *ctx, const vdf_align_rates_stretches_job *j)
{
    if (!ctx || !j) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    vdf::AlignSeedRate rates[VDF_WINDOWS_MAX_RATES];
    // everything that can be said without the first arrays - the multi-GPU refusal last; then they come down and are checked
    if (int rc = align_rates_stretches_checks(ctx, "vdf_align_windows_rates_stretches_device", j, nullptr, nullptr, rates)) return rc;
    *j->n_out = 0;
    if (j->n_a == 0 || j->n_b == 0 || (j->triples && j->n_triples == 0)) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = j->stream ? (hipStream_t)j->stream : ctx->stream;
    std::vector<uint32_t> fa((size_t)j->n_rates * (j->n_a + 1)), fb(j->n_b + 1);
    VDF_HIP(ctx, hipMemcpyAsync(fa.data(), j->a_first, fa.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipMemcpyAsync(fb.data(), j->b_first, fb.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipStreamSynchronize(s));
    if (int rc = align_rates_stretches_checks(ctx, "vdf_align_windows_rates_stretches_device", j, fa.data(), fb.data(), rates)) return rc;
    return align_rates_stretches_locked(ctx, j, rates, j->a_hashes, j->a_skip, j->a_first, fa.data(), 0, j->b_hashes, j->b_skip, j->b_first, fb.data(), s);
}

// Host arrays: vdf_align_windows_rates' upload - the rows of A that the blocks span, the rows of B, [first a | first b, rebased | skip a | skip b]
// in align_up - made ONCE, for the seed pass and every round.
int vdf_align_windows_rates_stretches(vdf_ctx *ctx, const vdf_align_rates_stretches_job *j)
{
    if (!ctx || !j) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    vdf::AlignSeedRate rates[VDF_WINDOWS_MAX_RATES];
    if (int rc = align_rates_stretches_checks(ctx, "vdf_align_windows_rates_stretches", j, j->a_first, j->b_first, rates)) return rc;
    *j->n_out = 0;
    if (j->n_a == 0 || j->n_b == 0 || (j->triples && j->n_triples == 0)) return VDF_OK;
    uint64_t a_lo = ~0ull, a_hi = 0;
    for (uint32_t r = 0; r < j->n_rates; r++) {
        const uint32_t *fa = j->a_first + (size_t)r * (j->n_a + 1);
        const uint64_t base = j->a_rate_first ? (uint64_t)j->a_rate_first[r] : 0ull;
        a_lo = std::min(a_lo, base + fa[0]);
        a_hi = std::max(a_hi, base + fa[j->n_a]);
    }
    const uint64_t b_lo = j->b_first[0], b_hi = j->b_first[j->n_b];
    const size_t wa = (size_t)(a_hi - a_lo), wb = (size_t)(b_hi - b_lo);
    if (wa == 0 || wb == 0) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    std::vector<uint32_t> fb(j->n_b + 1);
    for (size_t v = 0; v <= j->n_b; v++) fb[v] = j->b_first[v] - j->b_first[0];
    const size_t fa_bytes = (size_t)j->n_rates * (j->n_a + 1) * sizeof(uint32_t), fb_bytes = fb.size() * sizeof(uint32_t);
    const size_t ska = j->a_skip ? (wa + 3) & ~(size_t)3 : 0, skb = j->b_skip ? wb : 0;
    VDF_HIP(ctx, ctx->align_up.reserve(fa_bytes + fb_bytes + ska + skb + 16));
    char *up = ctx->align_up.as<char>();
    VDF_HIP(ctx, hipMemcpyAsync(up, j->a_first, fa_bytes, hipMemcpyHostToDevice, s));
    VDF_HIP(ctx, hipMemcpyAsync(up + fa_bytes, fb.data(), fb_bytes, hipMemcpyHostToDevice, s));
    if (ska) VDF_HIP(ctx, hipMemcpyAsync(up + fa_bytes + fb_bytes, j->a_skip + a_lo, wa, hipMemcpyHostToDevice, s));
    if (skb) VDF_HIP(ctx, hipMemcpyAsync(up + fa_bytes + fb_bytes + ska, j->b_skip + b_lo, wb, hipMemcpyHostToDevice, s));
    if (int rc = upload(ctx, ctx->up_hashes, j->a_hashes + 16 * (size_t)a_lo, wa * 16 * sizeof(uint64_t), s)) return rc;
    if (int rc = upload(ctx, ctx->up_ref_hashes, j->b_hashes + 16 * (size_t)b_lo, wb * 16 * sizeof(uint64_t), s)) return rc;
    return align_rates_stretches_locked(ctx, j, rates, ctx->up_hashes.as<uint64_t>(), ska ? reinterpret_cast<const uint8_t *>(up + fa_bytes + fb_bytes) : nullptr,
                                        reinterpret_cast<const uint32_t *>(up), j->a_first, a_lo, ctx->up_ref_hashes.as<uint64_t>(),
                                        skb ? reinterpret_cast<const uint8_t *>(up + fa_bytes + fb_bytes + ska) : nullptr,
                                        reinterpret_cast<const uint32_t *>(up + fa_bytes), fb.data(), s);
}

size_t vdf_hash_window_count(uint32_t frames_per_clip, uint32_t window_stride) { return vdf::window_count(frames_per_clip, window_stride); }

int vdf_hash_windows_u8_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h,
                               size_t frame_stride, size_t clip_stride, uint32_t window_stride, uint64_t *d_out_hashes,
                               uint32_t *d_out_dontcare, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool run;
    if (int rc = windows_checks(ctx, d_frames, n_clips, frames_per_clip, w, h, frame_stride, window_stride, d_out_hashes, &run)) return rc;
    if (!run) return VDF_OK;
    return hash_windows_locked(ctx, d_frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride, window_stride, d_out_hashes, d_out_dontcare,
                               stream ? (hipStream_t)stream : ctx->stream);
}

// Host arrays: the frames go up through the context's staging buffer in one piece, the device form runs on it, the results come down.
int vdf_hash_windows_u8(vdf_ctx *ctx, const uint8_t *frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h,
                        size_t frame_stride, size_t clip_stride, uint32_t window_stride, uint64_t *out_hashes, uint32_t *out_dontcare)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool run;
    if (int rc = windows_checks(ctx, frames, n_clips, frames_per_clip, w, h, frame_stride, window_stride, out_hashes, &run)) return rc;
    if (!run) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n_out = n_clips * vdf::window_count(frames_per_clip, window_stride);
    size_t clips_span = 0, frames_span = 0, bytes = 0;  // first byte of clip 0 to the last byte of the last clip's last frame, in size_t
    if (__builtin_mul_overflow(n_clips - 1, clip_stride, &clips_span) || __builtin_mul_overflow((size_t)(frames_per_clip - 1), frame_stride, &frames_span) ||
        __builtin_add_overflow(clips_span, frames_span, &bytes) || __builtin_add_overflow(bytes, (size_t)w * h, &bytes))
        return fail(ctx, VDF_E_INVAL, "the clips' extent does not fit size_t");
    if (int rc = upload(ctx, ctx->frames, frames, bytes, ctx->stream)) return rc;
    VDF_HIP(ctx, ctx->out_hashes.reserve(n_out * VDF_HASH_WORDS * sizeof(uint64_t)));
    if (out_dontcare) VDF_HIP(ctx, ctx->out_dc.reserve(n_out * sizeof(uint32_t)));
    uint32_t *d_dc = out_dontcare ? ctx->out_dc.as<uint32_t>() : nullptr;
    if (int rc = hash_windows_locked(ctx, ctx->frames.as<uint8_t>(), n_clips, frames_per_clip, w, h, frame_stride, clip_stride, window_stride,
                                     ctx->out_hashes.as<uint64_t>(), d_dc, ctx->stream))
        return rc;
    VDF_HIP(ctx, hipMemcpyAsync(out_hashes, ctx->out_hashes.p, n_out * VDF_HASH_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (out_dontcare) VDF_HIP(ctx, hipMemcpyAsync(out_dontcare, d_dc, n_out * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VDF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VDF_OK;
}

// ---- retimed window hashes (include/vdf.h: vdf_hash_windows_u8_retimed[_device]) ----------------------------------------------
size_t vdf_hash_window_count_retimed(uint32_t frames_per_clip, uint32_t window_stride, uint32_t rate_num, uint32_t rate_den)
{
    return vdf::retimed_window_count(frames_per_clip, window_stride, rate_num, rate_den);
}

int vdf_hash_windows_u8_retimed_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h,
                                       size_t frame_stride, size_t clip_stride, uint32_t window_stride, uint32_t rate_num, uint32_t rate_den,
                                       uint64_t *d_out_hashes, uint32_t *d_out_dontcare, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool run;
    if (int rc = windows_checks(ctx, d_frames, n_clips, frames_per_clip, w, h, frame_stride, window_stride, d_out_hashes, &run)) return rc;
    if (int rc = windows_retimed_checks(ctx, frames_per_clip, rate_num, rate_den)) return rc;
    if (!run) return VDF_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (vdf::retimed_is_plain(rate_num, rate_den))  // the taps are 0 ... 15: the plain call, its route and its words
        return hash_windows_locked(ctx, d_frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride, window_stride, d_out_hashes, d_out_dontcare, s);
    const vdf::WindowsRetimedPlan rp = vdf::plan_windows_retimed(frames_per_clip, window_stride, rate_num, rate_den);
    return hash_windows_locked(ctx, d_frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride, window_stride, d_out_hashes, d_out_dontcare, s, nullptr,
                               &rp);
}

// Host arrays: as vdf_hash_windows_u8 - one upload through the context's staging buffer, the device form's work on it, the results come down.
int vdf_hash_windows_u8_retimed(vdf_ctx *ctx, const uint8_t *frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h,
                                size_t frame_stride, size_t clip_stride, uint32_t window_stride, uint32_t rate_num, uint32_t rate_den,
                                uint64_t *out_hashes, uint32_t *out_dontcare)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool run;
    if (int rc = windows_checks(ctx, frames, n_clips, frames_per_clip, w, h, frame_stride, window_stride, out_hashes, &run)) return rc;
    if (int rc = windows_retimed_checks(ctx, frames_per_clip, rate_num, rate_den)) return rc;
    if (!run) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n_out = n_clips * vdf::retimed_window_count(frames_per_clip, window_stride, rate_num, rate_den);
    size_t clips_span = 0, frames_span = 0, bytes = 0;  // as vdf_hash_windows_u8: first byte of clip 0 to the last byte of the last clip's last frame
    if (__builtin_mul_overflow(n_clips - 1, clip_stride, &clips_span) || __builtin_mul_overflow((size_t)(frames_per_clip - 1), frame_stride, &frames_span) ||
        __builtin_add_overflow(clips_span, frames_span, &bytes) || __builtin_add_overflow(bytes, (size_t)w * h, &bytes))
        return fail(ctx, VDF_E_INVAL, "the clips' extent does not fit size_t");
    if (int rc = upload(ctx, ctx->frames, frames, bytes, ctx->stream)) return rc;
    VDF_HIP(ctx, ctx->out_hashes.reserve(n_out * VDF_HASH_WORDS * sizeof(uint64_t)));
    if (out_dontcare) VDF_HIP(ctx, ctx->out_dc.reserve(n_out * sizeof(uint32_t)));
    uint32_t *d_dc = out_dontcare ? ctx->out_dc.as<uint32_t>() : nullptr;
    const vdf::WindowsRetimedPlan rp = vdf::plan_windows_retimed(frames_per_clip, window_stride, rate_num, rate_den);
    if (int rc = hash_windows_locked(ctx, ctx->frames.as<uint8_t>(), n_clips, frames_per_clip, w, h, frame_stride, clip_stride, window_stride,
                                     ctx->out_hashes.as<uint64_t>(), d_dc, ctx->stream, nullptr, vdf::retimed_is_plain(rate_num, rate_den) ? nullptr : &rp))
        return rc;
    VDF_HIP(ctx, hipMemcpyAsync(out_hashes, ctx->out_hashes.p, n_out * VDF_HASH_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (out_dontcare) VDF_HIP(ctx, hipMemcpyAsync(out_dontcare, d_dc, n_out * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VDF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VDF_OK;
}

// ---- retimed window hashes at several rates from one read of the frames (include/vdf.h: vdf_hash_windows_u8_rates[_device]) -------
size_t vdf_hash_window_count_rates(size_t n_clips, uint32_t frames_per_clip, uint32_t window_stride, uint32_t n_rates, const uint32_t *rate_num,
                                   const uint32_t *rate_den, size_t *rate_first)
{
    const vdf::WindowsRatesPlan p = vdf::plan_windows_rates(n_clips, frames_per_clip, window_stride, n_rates, rate_num, rate_den);
    if (rate_first && n_rates >= 1 && n_rates <= VDF_WINDOWS_MAX_RATES) {
        for (uint32_t r = 0; r < n_rates; r++) rate_first[r] = p.ok ? (size_t)p.a.out_first[r] : 0;
        rate_first[n_rates] = p.ok ? (size_t)p.n_out : 0;
    }
    return p.ok ? (size_t)p.n_out : 0;
}

// the checks of both forms, in the order their codes are reported (include/vdf.h); *run: there is something to hash, and *plan says what
static int windows_rates_checks(vdf_ctx *ctx, const vdf_windows_rates_job *job, bool *run, vdf::WindowsRatesPlan *plan)
{
    bool some;
    *run = false;
    if (int rc = windows_checks(ctx, job->frames, job->n_clips, job->frames_per_clip, job->w, job->h, job->frame_stride, job->window_stride, job->out_hashes,
                                &some))
        return rc;
    if (job->n_rates == 0 || job->n_rates > VDF_WINDOWS_MAX_RATES) return fail(ctx, VDF_E_INVAL, "n_rates outside 1 ... 8");
    if (!job->rate_num || !job->rate_den) return fail(ctx, VDF_E_INVAL, "null rate array");
    for (uint32_t r = 0; r < job->n_rates; r++)
        if (!vdf::retimed_rate_ok(job->rate_num[r], job->rate_den[r]))
            return fail(ctx, VDF_E_INVAL, "rate outside 1 <= den <= num <= 2 den, num <= 65535 (rate " + std::to_string(r) + ")");
    for (uint32_t r = 0; r < job->n_rates; r++)
        if (job->frames_per_clip < vdf::retimed_span(job->rate_num[r], job->rate_den[r]))
            return fail(ctx, VDF_E_NOT_ENOUGH_FRAMES, "fewer frames per clip than a retimed window spans (rate " + std::to_string(r) + ")");
    *plan = vdf::plan_windows_rates(job->n_clips, job->frames_per_clip, job->window_stride, job->n_rates, job->rate_num, job->rate_den);
    if (!plan->ok) return fail(ctx, VDF_E_INVAL, "internal: a list of rates that passed the checks was not planned");
    if (plan->n_out > 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "2^32 windows or more in one call");
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "the windows calls take a single-device context");
    *run = some;
    return VDF_OK;
}

// windows_rates_checks has passed: hash_windows_locked's resize stage once, then every rate's windows from one launch
static int hash_windows_rates_locked(vdf_ctx *ctx, const uint8_t *d_frames, const vdf_windows_rates_job *job, const vdf::WindowsRatesPlan &plan, uint64_t *d_out,
                                     uint32_t *d_dc, hipStream_t stream)
{
    vdf::WindowsFrames wf{};
    if (int rc = windows_frames_locked(ctx, d_frames, job->n_clips, job->frames_per_clip, job->w, job->h, job->frame_stride, job->clip_stride, stream, &wf))
        return rc;
    VDF_HIP(ctx, vdf::launch_dct_hash_windows_rates(wf, job->n_clips, plan, ctx->cos_table.as<double>(), d_out, d_dc, stream));
    return VDF_OK;
}

int vdf_hash_windows_u8_rates_device(vdf_ctx *ctx, const vdf_windows_rates_job *job)
{
    if (!ctx || !job) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool run;
    vdf::WindowsRatesPlan plan;  // the rates travel to the kernel inside it, by value: the caller's arrays are not read after the checks
    if (int rc = windows_rates_checks(ctx, job, &run, &plan)) return rc;
    if (!run) return VDF_OK;
    return hash_windows_rates_locked(ctx, job->frames, job, plan, job->out_hashes, job->out_dontcare, job->stream ? (hipStream_t)job->stream : ctx->stream);
}

// Host arrays: as vdf_hash_windows_u8_retimed - ONE upload through the context's staging buffer, the device form's work on it, all blocks come down.
int vdf_hash_windows_u8_rates(vdf_ctx *ctx, const vdf_windows_rates_job *job)
{
    if (!ctx || !job) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool run;
    vdf::WindowsRatesPlan plan;
    if (int rc = windows_rates_checks(ctx, job, &run, &plan)) return rc;
    if (!run) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n_out = (size_t)plan.n_out;
    size_t clips_span = 0, frames_span = 0, bytes = 0;  // as vdf_hash_windows_u8: first byte of clip 0 to the last byte of the last clip's last frame
    if (__builtin_mul_overflow(job->n_clips - 1, job->clip_stride, &clips_span) ||
        __builtin_mul_overflow((size_t)(job->frames_per_clip - 1), job->frame_stride, &frames_span) || __builtin_add_overflow(clips_span, frames_span, &bytes) ||
        __builtin_add_overflow(bytes, (size_t)job->w * job->h, &bytes))
        return fail(ctx, VDF_E_INVAL, "the clips' extent does not fit size_t");
    if (int rc = upload(ctx, ctx->frames, job->frames, bytes, ctx->stream)) return rc;
    VDF_HIP(ctx, ctx->out_hashes.reserve(n_out * VDF_HASH_WORDS * sizeof(uint64_t)));
    if (job->out_dontcare) VDF_HIP(ctx, ctx->out_dc.reserve(n_out * sizeof(uint32_t)));
    uint32_t *d_dc = job->out_dontcare ? ctx->out_dc.as<uint32_t>() : nullptr;
    if (int rc = hash_windows_rates_locked(ctx, ctx->frames.as<uint8_t>(), job, plan, ctx->out_hashes.as<uint64_t>(), d_dc, ctx->stream)) return rc;
    VDF_HIP(ctx, hipMemcpyAsync(job->out_hashes, ctx->out_hashes.p, n_out * VDF_HASH_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (job->out_dontcare) VDF_HIP(ctx, hipMemcpyAsync(job->out_dontcare, d_dc, n_out * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VDF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VDF_OK;
}

int vdf_cropdetect_letterbox_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                                    uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride, uint32_t *d_crops,
                                    void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    if (frames_per_clip == 0) return fail(ctx, VDF_E_NOT_ENOUGH_FRAMES, "no frames to detect a crop on");
    if (w == 0 || h == 0) return fail(ctx, VDF_E_BAD_DIMS, "zero frame dimension");
    if (n_clips == 0) return VDF_OK;
    if (!d_frames || !d_crops) return fail(ctx, VDF_E_INVAL, "null pointer");
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    VDF_HIP(ctx, ctx->crop_work.reserve(vdf::letterbox_work_bytes(std::min(kMaxClipsPerLaunch, n_clips), frames_per_clip)));
    for (size_t c0 = 0; c0 < n_clips; c0 += kMaxClipsPerLaunch)
        VDF_HIP(ctx, vdf::launch_letterbox(d_frames + c0 * clip_stride, std::min(kMaxClipsPerLaunch, n_clips - c0),
                                           frames_per_clip, w, h, frame_stride, clip_stride, d_crops + 4 * c0, ctx->crop_work.as<uint32_t>(),
                                           stream ? (hipStream_t)stream : ctx->stream, ctx->lb_side_strips));
    return VDF_OK;
}

int vdf_hash_frames_u8_cropped_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                                      uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride,
                                      const uint32_t *crops, uint64_t *d_out_hashes, uint32_t *d_out_dontcare,
                                      void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    return hash_cropped_locked(ctx, d_frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride, crops,
                               d_out_hashes, d_out_dontcare, stream ? (hipStream_t)stream : ctx->stream);
}

int vdf_hash_clips_u8_device(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips, uint32_t frames_per_clip,
                             uint64_t *d_out_hashes, uint32_t *d_out_dontcare, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    return hash_clips_locked(ctx, d_buf, buf_bytes, clips, n_clips, frames_per_clip, d_out_hashes, d_out_dontcare, stream ? (hipStream_t)stream : ctx->stream);
}

int vdf_hash_clips_u8(vdf_ctx *ctx, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips, uint32_t frames_per_clip,
                      uint64_t *out_hashes, uint32_t *out_dontcare)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "vdf_hash_clips_u8 takes a single-device context");
    return hash_clips_host_locked(ctx, buf, buf_bytes, clips, n_clips, frames_per_clip, out_hashes, out_dontcare);
}

// ---- the zero plane and the flipped hashes (include/vdf.h) -------------------------------------------------------------
// The derivation rests on the resize table of every axis the call resizes being its own mirror image: asked once per size, refused otherwise.
static int planes_axis_ok(vdf_ctx *ctx, uint32_t size)
{
    auto it = ctx->axis_symmetric.find(size);
    if (it == ctx->axis_symmetric.end()) it = ctx->axis_symmetric.emplace(size, vdf::axis_table_mirror_symmetric(size)).first;
    if (it->second) return VDF_OK;
    return fail(ctx, VDF_E_BAD_DIMS, "the resize table of axis size " + std::to_string(size) + " is not mirror-symmetric: no zero plane for this size");
}

// the plain call's checks in the plain call's order, then the plane's own; *run: there is something to hash
static int planes_frames_checks(vdf_ctx *ctx, const void *frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h, size_t frame_stride,
                                const void *out_hashes, const void *out_zero, bool *run)
{
    *run = false;
    if (frames_per_clip < VDF_DCT_SIZE) return fail(ctx, VDF_E_NOT_ENOUGH_FRAMES, "fewer than 16 frames per clip");
    if (w == 0 || h == 0) return fail(ctx, VDF_E_BAD_DIMS, "zero frame dimension");
    if (frame_stride < (size_t)w * h) return fail(ctx, VDF_E_INVAL, "frame_stride smaller than a frame");
    if (n_clips == 0) return VDF_OK;
    if (!frames || !out_hashes || !out_zero) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (int rc = planes_axis_ok(ctx, w)) return rc;
    if (int rc = planes_axis_ok(ctx, h)) return rc;
    *run = true;
    return VDF_OK;
}

static int planes_clips_checks(vdf_ctx *ctx, const void *buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips, uint32_t frames_per_clip,
                               const void *out_hashes, const void *out_zero, bool *run)
{
    *run = false;
    if (n_clips && !clips) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (n_clips > 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "more than 2^32 - 1 clips in one call");
    const vdf::MixedCheck chk = vdf::check_mixed(reinterpret_cast<const vdf::MixedClip *>(clips), n_clips, frames_per_clip, buf_bytes);
    if (chk.error != vdf::MixedError::kNone) return mixed_check_failed(ctx, chk);
    if (n_clips == 0) return VDF_OK;
    if (!buf || !out_hashes || !out_zero) return fail(ctx, VDF_E_INVAL, "null pointer");
    for (size_t i = 0; i < n_clips; i++) {  // the BOX is what is resized (check_mixed: it leaves pixels)
        if (int rc = planes_axis_ok(ctx, clips[i].w - clips[i].crop_left - clips[i].crop_right)) return rc;
        if (int rc = planes_axis_ok(ctx, clips[i].h - clips[i].crop_top - clips[i].crop_bottom)) return rc;
    }
    *run = true;
    return VDF_OK;
}

int vdf_hash_frames_u8_planes_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                                     uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride, uint64_t *d_out_hashes,
                                     uint32_t *d_out_dontcare, uint64_t *d_out_zero, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    bool run;
    if (int rc = planes_frames_checks(ctx, d_frames, n_clips, frames_per_clip, w, h, frame_stride, d_out_hashes, d_out_zero, &run)) return rc;
    if (!run) return VDF_OK;
    return hash_device_locked(ctx, d_frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride, d_out_hashes, d_out_dontcare,
                              stream ? (hipStream_t)stream : ctx->stream, d_out_zero);
}

int vdf_hash_frames_u8_planes(vdf_ctx *ctx, const uint8_t *frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w,
                              uint32_t h, size_t frame_stride, size_t clip_stride, uint64_t *out_hashes,
                              uint32_t *out_dontcare, uint64_t *out_zero)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "vdf_hash_frames_u8_planes takes a single-device context");
    bool run;
    if (int rc = planes_frames_checks(ctx, frames, n_clips, frames_per_clip, w, h, frame_stride, out_hashes, out_zero, &run)) return rc;
    if (!run) return VDF_OK;
    return hash_host_locked(ctx, frames, n_clips, w, h, frame_stride, clip_stride, 0, out_hashes, nullptr, out_dontcare, out_zero);
}

int vdf_hash_clips_u8_planes_device(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips,
                                    uint32_t frames_per_clip, uint64_t *d_out_hashes, uint32_t *d_out_dontcare,
                                    uint64_t *d_out_zero, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    bool run;
    if (int rc = planes_clips_checks(ctx, d_buf, buf_bytes, clips, n_clips, frames_per_clip, d_out_hashes, d_out_zero, &run)) return rc;
    if (!run) return VDF_OK;
    return hash_clips_locked(ctx, d_buf, buf_bytes, clips, n_clips, frames_per_clip, d_out_hashes, d_out_dontcare, stream ? (hipStream_t)stream : ctx->stream,
                             d_out_zero);
}

int vdf_hash_clips_u8_planes(vdf_ctx *ctx, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips,
                             uint32_t frames_per_clip, uint64_t *out_hashes, uint32_t *out_dontcare, uint64_t *out_zero)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "vdf_hash_clips_u8_planes takes a single-device context");
    bool run;
    if (int rc = planes_clips_checks(ctx, buf, buf_bytes, clips, n_clips, frames_per_clip, out_hashes, out_zero, &run)) return rc;
    if (!run) return VDF_OK;
    return hash_clips_host_locked(ctx, buf, buf_bytes, clips, n_clips, frames_per_clip, out_hashes, out_dontcare, 0, nullptr, out_zero);
}

// ---- zero planes of window hashes, the variant of a set of them, alignment against the variants (include/vdf.h) ---------------
// windows_checks' checks in windows_checks' order with out_zero among the null pointers, then the plane's own, the context last
static int windows_planes_checks(vdf_ctx *ctx, const void *frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h, size_t frame_stride,
                                 uint32_t window_stride, const void *out_hashes, const void *out_zero, bool *run)
{
    *run = false;
    if (frames_per_clip < VDF_DCT_SIZE) return fail(ctx, VDF_E_NOT_ENOUGH_FRAMES, "fewer than 16 frames per clip");
    if (w == 0 || h == 0) return fail(ctx, VDF_E_BAD_DIMS, "zero frame dimension");
    if (frame_stride < (size_t)w * h) return fail(ctx, VDF_E_INVAL, "frame_stride smaller than a frame");
    if (window_stride == 0) return fail(ctx, VDF_E_INVAL, "window_stride of zero");
    const size_t n_win = vdf::window_count(frames_per_clip, window_stride);
    if (frames_per_clip > 0xFFFFFFC0u || (n_clips && n_win > 0xFFFFFFFFull / n_clips)) return fail(ctx, VDF_E_INVAL, "2^32 windows or more in one call");
    if (n_clips == 0) return VDF_OK;
    if (!frames || !out_hashes || !out_zero) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (int rc = planes_axis_ok(ctx, w)) return rc;
    if (int rc = planes_axis_ok(ctx, h)) return rc;
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "the windows calls take a single-device context");
    *run = true;
    return VDF_OK;
}

int vdf_hash_windows_u8_planes_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h,
                                      size_t frame_stride, size_t clip_stride, uint32_t window_stride, uint64_t *d_out_hashes, uint32_t *d_out_dontcare,
                                      uint64_t *d_out_zero, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool run;
    if (int rc = windows_planes_checks(ctx, d_frames, n_clips, frames_per_clip, w, h, frame_stride, window_stride, d_out_hashes, d_out_zero, &run)) return rc;
    if (!run) return VDF_OK;
    return hash_windows_locked(ctx, d_frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride, window_stride, d_out_hashes, d_out_dontcare,
                               stream ? (hipStream_t)stream : ctx->stream, d_out_zero);
}

int vdf_hash_windows_u8_planes(vdf_ctx *ctx, const uint8_t *frames, size_t n_clips, uint32_t frames_per_clip, uint32_t w, uint32_t h, size_t frame_stride,
                               size_t clip_stride, uint32_t window_stride, uint64_t *out_hashes, uint32_t *out_dontcare, uint64_t *out_zero)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool run;
    if (int rc = windows_planes_checks(ctx, frames, n_clips, frames_per_clip, w, h, frame_stride, window_stride, out_hashes, out_zero, &run)) return rc;
    if (!run) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n_out = n_clips * vdf::window_count(frames_per_clip, window_stride), hash_bytes = n_out * VDF_HASH_WORDS * sizeof(uint64_t);
    size_t clips_span = 0, frames_span = 0, bytes = 0;  // as vdf_hash_windows_u8: first byte of clip 0 to the last byte of the last clip's last frame
    if (__builtin_mul_overflow(n_clips - 1, clip_stride, &clips_span) || __builtin_mul_overflow((size_t)(frames_per_clip - 1), frame_stride, &frames_span) ||
        __builtin_add_overflow(clips_span, frames_span, &bytes) || __builtin_add_overflow(bytes, (size_t)w * h, &bytes))
        return fail(ctx, VDF_E_INVAL, "the clips' extent does not fit size_t");
    if (int rc = upload(ctx, ctx->frames, frames, bytes, ctx->stream)) return rc;
    VDF_HIP(ctx, ctx->out_hashes.reserve(hash_bytes));
    VDF_HIP(ctx, ctx->out_zero.reserve(hash_bytes));
    if (out_dontcare) VDF_HIP(ctx, ctx->out_dc.reserve(n_out * sizeof(uint32_t)));
    uint32_t *d_dc = out_dontcare ? ctx->out_dc.as<uint32_t>() : nullptr;
    if (int rc = hash_windows_locked(ctx, ctx->frames.as<uint8_t>(), n_clips, frames_per_clip, w, h, frame_stride, clip_stride, window_stride,
                                     ctx->out_hashes.as<uint64_t>(), d_dc, ctx->stream, ctx->out_zero.as<uint64_t>()))
        return rc;
    VDF_HIP(ctx, hipMemcpyAsync(out_hashes, ctx->out_hashes.p, hash_bytes, hipMemcpyDeviceToHost, ctx->stream));
    VDF_HIP(ctx, hipMemcpyAsync(out_zero, ctx->out_zero.p, hash_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (out_dontcare) VDF_HIP(ctx, hipMemcpyAsync(out_dontcare, d_dc, n_out * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VDF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VDF_OK;
}

// ---- window hashes of videos of different sizes and lengths in one call (include/vdf.h: vdf_hash_windows_clips_u8*) -----------
int vdf_hash_windows_clips_first(const uint32_t *n_frames, size_t n_videos, uint32_t window_stride, uint32_t *first)
{
    if (!first || (n_videos && !n_frames) || window_stride == 0 || n_videos >= 0xFFFFFFFFull) return VDF_E_INVAL;
    for (size_t i = 0; i < n_videos; i++)
        if (n_frames[i] < VDF_DCT_SIZE) return VDF_E_NOT_ENOUGH_FRAMES;
    return vdf::windows_first(n_frames, n_videos, window_stride, first) ? VDF_OK : VDF_E_INVAL;
}

// does the table of one box axis fit the i8 split?  A single-device context fetches it (it is about to be used); a multi-GPU context - refused
// last, after this check - asks the host-side builder and touches no device.
static int windows_clips_table_fits(vdf_ctx *ctx, uint32_t size, int layout, hipStream_t stream, bool *fits)
{
    if (!ctx->subs.empty()) {
        vdf::MfmaAxisTable t;
        *fits = vdf::build_mfma_axis_table(size, layout, t) && t.ok;
        return VDF_OK;
    }
    int rc = VDF_OK;
    const DeviceMfmaTable *t = mfma_table(ctx, size, layout, stream, &rc);
    if (rc) return rc;
    *fits = t->host.ok;
    return VDF_OK;
}

// The argument checks of the mixed windows calls over ALL videos, in the order their codes are reported; *run: there is something to hash.
static int windows_clips_checks(vdf_ctx *ctx, const void *buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames, size_t n_videos,
                                uint32_t window_stride, const void *out_hashes, const void *out_zero, bool planes, hipStream_t stream, bool *run)
{
    *run = false;
    if (n_videos && (!clips || !n_frames)) return fail(ctx, VDF_E_INVAL, "null pointer");  // (nothing to check the videos by)
    if (n_videos >= 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "more than 2^32 - 2 videos in one call");
    const vdf::MixedClip *mc = reinterpret_cast<const vdf::MixedClip *>(clips);
    const vdf::WindowsMixedCheck chk = vdf::check_windows_mixed(mc, n_frames, n_videos, window_stride, buf_bytes);
    const std::string at = " (video " + std::to_string(chk.video) + ")";
    switch (chk.error) {
    case vdf::WindowsMixedError::kNotEnoughFrames: return fail(ctx, VDF_E_NOT_ENOUGH_FRAMES, "fewer than 16 frames" + at);
    case vdf::WindowsMixedError::kZeroDim: return fail(ctx, VDF_E_BAD_DIMS, "zero frame dimension" + at);
    case vdf::WindowsMixedError::kStrideBelowFrame: return fail(ctx, VDF_E_INVAL, "frame_stride smaller than a frame" + at);
    case vdf::WindowsMixedError::kEmptyBox: return fail(ctx, VDF_E_INVAL, "crop box leaves no pixels" + at);
    case vdf::WindowsMixedError::kOutOfBuffer: return fail(ctx, VDF_E_INVAL, "video reaches past the end of the buffer" + at);
    case vdf::WindowsMixedError::kZeroWindowStride: return fail(ctx, VDF_E_INVAL, "window_stride of zero");
    case vdf::WindowsMixedError::kFrameCount: return fail(ctx, VDF_E_INVAL, "frame count within 64 of 2^32" + at);
    case vdf::WindowsMixedError::kTooManyWindows: return fail(ctx, VDF_E_INVAL, "2^32 windows or more in one call" + at);
    case vdf::WindowsMixedError::kNone: break;
    }
    if (n_videos == 0) return VDF_OK;
    if (!buf || !out_hashes || (planes && !out_zero)) return fail(ctx, VDF_E_INVAL, "null pointer");
    for (size_t i = 0; i < n_videos; i++) {  // the BOX is what is resized (check_windows_mixed: it leaves pixels)
        const uint32_t bw = clips[i].w - clips[i].crop_left - clips[i].crop_right, bh = clips[i].h - clips[i].crop_top - clips[i].crop_bottom;
        const int layout_v = vdf::windows_mixed_part_of(clips[i].w) == vdf::MixedPart::kWideLines ? vdf::kMfmaLayoutVerticalWide : vdf::kMfmaLayoutVertical;
        bool fits_h = false, fits_v = false;
        if (int rc = windows_clips_table_fits(ctx, bw, vdf::kMfmaLayoutHorizontal, stream, &fits_h)) return rc;
        if (int rc = windows_clips_table_fits(ctx, bh, layout_v, stream, &fits_v)) return rc;
        if (!fits_h || !fits_v) return fail(ctx, VDF_E_BAD_DIMS, "box size whose coefficients do not fit the i8 split (video " + std::to_string(i) + ")");
    }
    if (planes)
        for (size_t i = 0; i < n_videos; i++) {
            if (int rc = planes_axis_ok(ctx, clips[i].w - clips[i].crop_left - clips[i].crop_right)) return rc;
            if (int rc = planes_axis_ok(ctx, clips[i].h - clips[i].crop_top - clips[i].crop_bottom)) return rc;
        }
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "the windows calls take a single-device context");
    *run = true;
    return VDF_OK;
}

// What the mixed windows calls do in front of their windows kernel (plan: a WindowsMixedPlan or WindowsMixedRetimedPlan of kind kMixed): descriptors,
// table entries, the videos' records and the segment table go up in ONE copy through the pinned staging, and the mixed whole-line kernels write every
// pseudo-clip's 16 x 16 frames to `small`.  *d_videos / *d_seg_first: the device copies the windows kernel reads; *launched: the launches' error so far -
// the caller launches its kernel if that is hipSuccess and ends with windows_clips_staged_end either way.  (A template: C++ linkage inside the C block.)
extern "C++" {
template <class Plan>
static int windows_clips_stage(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const Plan &plan, size_t n_videos, hipStream_t stream,
                               const vdf::WindowsVideoRecord **d_videos, const uint32_t **d_seg_first, hipError_t *launched,
                               const void *extra = nullptr, size_t extra_bytes = 0, const void **d_extra = nullptr)
{
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure_cos_table(ctx, stream);
    if (rc) return rc;
    const auto pad64 = [](size_t b) { return (b + 63) & ~size_t(63); };
    const size_t n_desc = plan.descs.size(), max_entries = 2 * ((size_t)plan.max_w + plan.max_h + 2);
    const size_t off_tab = pad64(n_desc * sizeof(vdf::MixedClipDesc)), off_vid = off_tab + pad64(max_entries * sizeof(vdf::CropTableEntry)),
                 off_seg = off_vid + pad64(n_videos * sizeof(vdf::WindowsVideoRecord)), off_extra = off_seg + pad64((n_videos + 1) * sizeof(uint32_t)),
                 blob = off_extra + pad64(extra_bytes);  // extra: a trailing piece of the caller's in the same copy (none: the blob as it always was)
    if (!ctx->pin_desc.reserve(blob)) return fail(ctx, VDF_E_OOM, "host staging for the video descriptors");
    char *stage = ctx->pin_desc.as<char>();
    vdf::MixedClipDesc *dsc = reinterpret_cast<vdf::MixedClipDesc *>(stage);
    vdf::CropTableEntry *ent = reinterpret_cast<vdf::CropTableEntry *>(stage + off_tab);
    // two sets, as hash_mixed_launch: the wide-line part reads its vertical tables in another k order
    LaunchTables plain(plan.max_w, plan.max_h, vdf::kMfmaLayoutHorizontal, vdf::kMfmaLayoutVertical), wide(plan.max_w, plan.max_h, vdf::kMfmaLayoutHorizontal, vdf::kMfmaLayoutVerticalWide);
    for (const vdf::MixedLaunch &l : plan.launches) {
        LaunchTables &tabs = l.part == vdf::MixedPart::kWideLines ? wide : plain;
        for (size_t i = l.first; i < l.first + l.count; i++) {
            vdf::MixedClipDesc d = plan.descs[i];
            const int32_t ih = tabs.entry(ctx, d.bw, false, stream, &rc), iv = ih < 0 ? -1 : tabs.entry(ctx, d.bh, true, stream, &rc);
            if (iv < 0) return rc ? rc : fail(ctx, VDF_E_BAD_DIMS, "box size whose coefficients do not fit the i8 split (video " + std::to_string(d.out_index) + ")");
            d.h_table = (uint32_t)ih; d.v_table = (uint32_t)iv;
            dsc[i] = d;
        }
    }
    const size_t n_plain = plain.used.size(), n_entries = n_plain + wide.used.size();
    if (n_entries > max_entries) return fail(ctx, VDF_E_INVAL, "table index of a mixed windows call outgrew its staging");  // (cannot happen: one entry per size and axis)
    for (size_t i = 0; i < n_plain; i++) ent[i] = plain.crop_entry(i);
    for (size_t i = n_plain; i < n_entries; i++) ent[i] = wide.crop_entry(i - n_plain);
    for (const vdf::MixedLaunch &l : plan.launches)
        for (size_t i = l.first; i < l.first + l.count; i++) {
            if (l.part == vdf::MixedPart::kWideLines) { dsc[i].h_table += (uint32_t)n_plain; dsc[i].v_table += (uint32_t)n_plain; }
            if (dsc[i].h_table >= n_entries || dsc[i].v_table >= n_entries) return fail(ctx, VDF_E_INVAL, "descriptor names a table that is not there");
        }
    std::memcpy(stage + off_vid, plan.videos.data(), n_videos * sizeof(vdf::WindowsVideoRecord));
    std::memcpy(stage + off_seg, plan.seg_first.data(), (n_videos + 1) * sizeof(uint32_t));
    if (extra_bytes) std::memcpy(stage + off_extra, extra, extra_bytes);
    VDF_HIP(ctx, ctx->small.reserve(std::max<size_t>(plan.small_bytes, 4096)));
    if ((rc = upload(ctx, ctx->crop_desc2, stage, blob, stream))) return rc;
    VDF_HIP(ctx, hipEventRecord(ctx->ev_mid, stream));
    const char *d_blob = ctx->crop_desc2.as<char>();
    const vdf::MixedClipDesc *d_desc = reinterpret_cast<const vdf::MixedClipDesc *>(d_blob);
    const vdf::CropTableEntry *d_tab = reinterpret_cast<const vdf::CropTableEntry *>(d_blob + off_tab);
    uint8_t *small = ctx->small.as<uint8_t>();
    hipError_t e = hipSuccess;
    for (const vdf::MixedLaunch &l : plan.launches) {
        if (e != hipSuccess) break;
        e = vdf::launch_mixed_frames(d_buf, d_buf + buf_bytes, d_desc + l.first, l.count, d_tab, l.part == vdf::MixedPart::kWideLines, small + l.first * 4096, stream);
    }
    *d_videos = reinterpret_cast<const vdf::WindowsVideoRecord *>(d_blob + off_vid);
    *d_seg_first = reinterpret_cast<const uint32_t *>(d_blob + off_seg);
    if (d_extra) *d_extra = d_blob + off_extra;
    *launched = e;
    return VDF_OK;
}
}  // extern "C++"

// the staging is read by the copy: it must have run before the next call on this context rewrites it (the kernels stay queued)
static int windows_clips_staged_end(vdf_ctx *ctx, hipError_t e, const char *what)
{
    const hipError_t ew = hipEventSynchronize(ctx->ev_mid);
    if (e != hipSuccess) return fail_hip(ctx, e, what);
    VDF_HIP(ctx, ew);
    return VDF_OK;
}

// windows_clips_checks has passed.  Uniform input: the uniform call.  Otherwise descriptors, table entries, the videos' records and the segment
// table go up in ONE copy through the pinned staging, the mixed whole-line kernels write every pseudo-clip's 16 x 16 frames to `small`, and
// dct_hash_windows_mixed_kernel hashes the windows from there to the rows first[i] + k.
static int hash_windows_clips_locked(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames, size_t n_videos,
                                     uint32_t window_stride, uint64_t *d_out, uint32_t *d_dc, hipStream_t stream, uint64_t *d_zero)
{
    const vdf::MixedClip *mc = reinterpret_cast<const vdf::MixedClip *>(clips);
    const vdf::WindowsMixedPlan plan = vdf::plan_windows_mixed(mc, n_frames, n_videos, window_stride);
    if (plan.kind == vdf::WindowsMixedPlan::kUniform)
        return hash_windows_locked(ctx, d_buf + plan.offset0, n_videos, n_frames[0], mc[0].w, mc[0].h, (size_t)mc[0].frame_stride, (size_t)plan.clip_stride,
                                   window_stride, d_out, d_dc, stream, d_zero);
    const vdf::WindowsVideoRecord *d_videos = nullptr;
    const uint32_t *d_seg_first = nullptr;
    hipError_t e = hipSuccess;
    if (int rc = windows_clips_stage(ctx, d_buf, buf_bytes, plan, n_videos, stream, &d_videos, &d_seg_first, &e)) return rc;
    if (e == hipSuccess)
        e = vdf::launch_dct_hash_windows_mixed(ctx->small.as<uint8_t>(), d_videos, d_seg_first, (uint32_t)n_videos, plan.seg_first[n_videos], window_stride, plan.per_seg,
                                               ctx->cos_table.as<double>(), d_out, d_dc, stream, d_zero);
    return windows_clips_staged_end(ctx, e, "mixed windows launch");
}

static int hash_windows_clips_device_impl(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames, size_t n_videos,
                                          uint32_t window_stride, uint64_t *d_out_hashes, uint32_t *d_out_dontcare, uint64_t *d_out_zero, bool planes,
                                          void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    bool run;
    if (int rc = windows_clips_checks(ctx, d_buf, buf_bytes, clips, n_frames, n_videos, window_stride, d_out_hashes, d_out_zero, planes, s, &run)) return rc;
    if (!run) return VDF_OK;
    return hash_windows_clips_locked(ctx, d_buf, buf_bytes, clips, n_frames, n_videos, window_stride, d_out_hashes, d_out_dontcare, s, planes ? d_out_zero : nullptr);
}

// Host arrays: the buffer goes up through the context's staging buffer in one piece, the device form runs on it, the results come down.
static int hash_windows_clips_host_impl(vdf_ctx *ctx, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames, size_t n_videos,
                                        uint32_t window_stride, uint64_t *out_hashes, uint32_t *out_dontcare, uint64_t *out_zero, bool planes)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool run;
    if (int rc = windows_clips_checks(ctx, buf, buf_bytes, clips, n_frames, n_videos, window_stride, out_hashes, out_zero, planes, ctx->stream, &run)) return rc;
    if (!run) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    size_t n_out = 0;
    for (size_t i = 0; i < n_videos; i++) n_out += vdf::window_count(n_frames[i], window_stride);
    const size_t hash_bytes = n_out * VDF_HASH_WORDS * sizeof(uint64_t);
    if (int rc = upload(ctx, ctx->frames, buf, buf_bytes, ctx->stream)) return rc;
    VDF_HIP(ctx, ctx->out_hashes.reserve(hash_bytes));
    if (planes) VDF_HIP(ctx, ctx->out_zero.reserve(hash_bytes));
    if (out_dontcare) VDF_HIP(ctx, ctx->out_dc.reserve(n_out * sizeof(uint32_t)));
    uint32_t *d_dc = out_dontcare ? ctx->out_dc.as<uint32_t>() : nullptr;
    if (int rc = hash_windows_clips_locked(ctx, ctx->frames.as<uint8_t>(), buf_bytes, clips, n_frames, n_videos, window_stride, ctx->out_hashes.as<uint64_t>(), d_dc,
                                           ctx->stream, planes ? ctx->out_zero.as<uint64_t>() : nullptr))
        return rc;
    VDF_HIP(ctx, hipMemcpyAsync(out_hashes, ctx->out_hashes.p, hash_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (planes) VDF_HIP(ctx, hipMemcpyAsync(out_zero, ctx->out_zero.p, hash_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (out_dontcare) VDF_HIP(ctx, hipMemcpyAsync(out_dontcare, d_dc, n_out * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VDF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VDF_OK;
}

int vdf_hash_windows_clips_u8_device(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames, size_t n_videos,
                                     uint32_t window_stride, uint64_t *d_out_hashes, uint32_t *d_out_dontcare, void *stream)
{
    return hash_windows_clips_device_impl(ctx, d_buf, buf_bytes, clips, n_frames, n_videos, window_stride, d_out_hashes, d_out_dontcare, nullptr, false, stream);
}

int vdf_hash_windows_clips_u8(vdf_ctx *ctx, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames, size_t n_videos,
                              uint32_t window_stride, uint64_t *out_hashes, uint32_t *out_dontcare)
{
    return hash_windows_clips_host_impl(ctx, buf, buf_bytes, clips, n_frames, n_videos, window_stride, out_hashes, out_dontcare, nullptr, false);
}

int vdf_hash_windows_clips_u8_planes_device(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames,
                                            size_t n_videos, uint32_t window_stride, uint64_t *d_out_hashes, uint32_t *d_out_dontcare, uint64_t *d_out_zero,
                                            void *stream)
{
    return hash_windows_clips_device_impl(ctx, d_buf, buf_bytes, clips, n_frames, n_videos, window_stride, d_out_hashes, d_out_dontcare, d_out_zero, true, stream);
}

int vdf_hash_windows_clips_u8_planes(vdf_ctx *ctx, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames, size_t n_videos,
                                     uint32_t window_stride, uint64_t *out_hashes, uint32_t *out_dontcare, uint64_t *out_zero)
{
    return hash_windows_clips_host_impl(ctx, buf, buf_bytes, clips, n_frames, n_videos, window_stride, out_hashes, out_dontcare, out_zero, true);
}

// ---- retimed window hashes of a whole library in one call (include/vdf.h: vdf_hash_windows_clips_u8_retimed*) --------------------
int vdf_hash_windows_clips_first_retimed(const uint32_t *n_frames, size_t n_videos, uint32_t window_stride, uint32_t rate_num, uint32_t rate_den,
                                         uint32_t *first)
{
    if (!first || (n_videos && !n_frames) || window_stride == 0 || n_videos >= 0xFFFFFFFFull) return VDF_E_INVAL;
    for (size_t i = 0; i < n_videos; i++)
        if (n_frames[i] < VDF_DCT_SIZE) return VDF_E_NOT_ENOUGH_FRAMES;
    switch (vdf::check_windows_mixed_retimed(n_frames, n_videos, rate_num, rate_den).error) {
    case vdf::WindowsMixedRetimedError::kBadRate: return VDF_E_INVAL;
    case vdf::WindowsMixedRetimedError::kShorterThanSpan: return VDF_E_NOT_ENOUGH_FRAMES;
    case vdf::WindowsMixedRetimedError::kNone: break;
    }
    return vdf::windows_first_retimed(n_frames, n_videos, window_stride, rate_num, rate_den, first) ? VDF_OK : VDF_E_INVAL;
}

// the rate checks of the library call, behind windows_clips_checks' (whose window counts are the plain ones: upper bounds of the retimed ones)
static int windows_clips_retimed_checks(vdf_ctx *ctx, const uint32_t *n_frames, size_t n_videos, uint32_t rate_num, uint32_t rate_den)
{
    const vdf::WindowsMixedRetimedCheck chk = vdf::check_windows_mixed_retimed(n_frames, n_videos, rate_num, rate_den);
    switch (chk.error) {
    case vdf::WindowsMixedRetimedError::kBadRate: return fail(ctx, VDF_E_INVAL, "rate outside 1 <= den <= num <= 2 den, num <= 65535");
    case vdf::WindowsMixedRetimedError::kShorterThanSpan:
        return fail(ctx, VDF_E_NOT_ENOUGH_FRAMES, "fewer frames than a retimed window spans (video " + std::to_string(chk.video) + ")");
    case vdf::WindowsMixedRetimedError::kNone: break;
    }
    return VDF_OK;
}

// windows_clips_checks and windows_clips_retimed_checks have passed.  Plain taps: the plain mixed call.  Uniform input: the uniform retimed call.
// Otherwise hash_windows_clips_locked's steps - the one blob through the pinned staging, the mixed whole-line kernels into `small`, the event wait
// on the staging - with dct_hash_windows_mixed_retimed_kernel hashing the retimed windows from there to the rows first[i] + k.
static int hash_windows_clips_retimed_locked(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames,
                                             size_t n_videos, uint32_t window_stride, uint32_t rate_num, uint32_t rate_den, uint64_t *d_out, uint32_t *d_dc,
                                             hipStream_t stream)
{
    const vdf::MixedClip *mc = reinterpret_cast<const vdf::MixedClip *>(clips);
    const vdf::WindowsMixedRetimedPlan plan = vdf::plan_windows_mixed_retimed(mc, n_frames, n_videos, window_stride, rate_num, rate_den);
    if (plan.kind == vdf::WindowsMixedRetimedPlan::kPlain)
        return hash_windows_clips_locked(ctx, d_buf, buf_bytes, clips, n_frames, n_videos, window_stride, d_out, d_dc, stream, nullptr);
    if (plan.kind == vdf::WindowsMixedRetimedPlan::kUniform)
        return hash_windows_locked(ctx, d_buf + plan.offset0, n_videos, n_frames[0], mc[0].w, mc[0].h, (size_t)mc[0].frame_stride, (size_t)plan.clip_stride,
                                   window_stride, d_out, d_dc, stream, nullptr, &plan.rate);
    const vdf::WindowsVideoRecord *d_videos = nullptr;
    const uint32_t *d_seg_first = nullptr;
    hipError_t e = hipSuccess;
    if (int rc = windows_clips_stage(ctx, d_buf, buf_bytes, plan, n_videos, stream, &d_videos, &d_seg_first, &e)) return rc;
    if (e == hipSuccess)
        e = vdf::launch_dct_hash_windows_mixed_retimed(ctx->small.as<uint8_t>(), d_videos, d_seg_first, (uint32_t)n_videos, plan.seg_first[n_videos], plan.rate,
                                                       ctx->cos_table.as<double>(), d_out, d_dc, stream);
    return windows_clips_staged_end(ctx, e, "mixed retimed windows launch");
}

int vdf_hash_windows_clips_u8_retimed_device(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames,
                                             size_t n_videos, uint32_t window_stride, uint32_t rate_num, uint32_t rate_den, uint64_t *d_out_hashes,
                                             uint32_t *d_out_dontcare, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    bool run;
    if (int rc = windows_clips_checks(ctx, d_buf, buf_bytes, clips, n_frames, n_videos, window_stride, d_out_hashes, nullptr, false, s, &run)) return rc;
    if (int rc = windows_clips_retimed_checks(ctx, n_frames, n_videos, rate_num, rate_den)) return rc;
    if (!run) return VDF_OK;
    return hash_windows_clips_retimed_locked(ctx, d_buf, buf_bytes, clips, n_frames, n_videos, window_stride, rate_num, rate_den, d_out_hashes, d_out_dontcare, s);
}

// Host arrays: as hash_windows_clips_host_impl - the buffer goes up in one piece, the device form's work runs on it, the results come down.
int vdf_hash_windows_clips_u8_retimed(vdf_ctx *ctx, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, const uint32_t *n_frames, size_t n_videos,
                                      uint32_t window_stride, uint32_t rate_num, uint32_t rate_den, uint64_t *out_hashes, uint32_t *out_dontcare)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool run;
    if (int rc = windows_clips_checks(ctx, buf, buf_bytes, clips, n_frames, n_videos, window_stride, out_hashes, nullptr, false, ctx->stream, &run)) return rc;
    if (int rc = windows_clips_retimed_checks(ctx, n_frames, n_videos, rate_num, rate_den)) return rc;
    if (!run) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    size_t n_out = 0;
    for (size_t i = 0; i < n_videos; i++) n_out += vdf::retimed_window_count(n_frames[i], window_stride, rate_num, rate_den);
    const size_t hash_bytes = n_out * VDF_HASH_WORDS * sizeof(uint64_t);
    if (int rc = upload(ctx, ctx->frames, buf, buf_bytes, ctx->stream)) return rc;
    VDF_HIP(ctx, ctx->out_hashes.reserve(hash_bytes));
    if (out_dontcare) VDF_HIP(ctx, ctx->out_dc.reserve(n_out * sizeof(uint32_t)));
    uint32_t *d_dc = out_dontcare ? ctx->out_dc.as<uint32_t>() : nullptr;
    if (int rc = hash_windows_clips_retimed_locked(ctx, ctx->frames.as<uint8_t>(), buf_bytes, clips, n_frames, n_videos, window_stride, rate_num, rate_den,
                                                   ctx->out_hashes.as<uint64_t>(), d_dc, ctx->stream))
        return rc;
    VDF_HIP(ctx, hipMemcpyAsync(out_hashes, ctx->out_hashes.p, hash_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (out_dontcare) VDF_HIP(ctx, hipMemcpyAsync(out_dontcare, d_dc, n_out * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VDF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VDF_OK;
}

// ---- retimed window hashes of a mixed library at several rates in one call (include/vdf.h: vdf_hash_windows_clips_u8_rates*) ------
int vdf_hash_windows_clips_first_rates(const uint32_t *n_frames, size_t n_videos, uint32_t window_stride, uint32_t n_rates, const uint32_t *rate_num,
                                       const uint32_t *rate_den, uint32_t *first, size_t *rate_first)
{
    if (!first || (n_videos && !n_frames) || window_stride == 0 || n_videos >= 0xFFFFFFFFull) return VDF_E_INVAL;
    if (n_rates == 0 || n_rates > VDF_WINDOWS_MAX_RATES || !rate_num || !rate_den) return VDF_E_INVAL;
    for (size_t i = 0; i < n_videos; i++)
        if (n_frames[i] < VDF_DCT_SIZE) return VDF_E_NOT_ENOUGH_FRAMES;
    switch (vdf::check_windows_mixed_rates(n_frames, n_videos, window_stride, n_rates, rate_num, rate_den).error) {
    case vdf::WindowsMixedRatesError::kRateCount:
    case vdf::WindowsMixedRatesError::kBadRate:
    case vdf::WindowsMixedRatesError::kTooManyRows: return VDF_E_INVAL;
    case vdf::WindowsMixedRatesError::kShorterThanSpan: return VDF_E_NOT_ENOUGH_FRAMES;
    case vdf::WindowsMixedRatesError::kNone: break;
    }
    uint64_t rf[VDF_WINDOWS_MAX_RATES + 1];
    if (!vdf::windows_first_rates(n_frames, n_videos, window_stride, n_rates, rate_num, rate_den, first, rf)) return VDF_E_INVAL;
    for (uint32_t r = 0; rate_first && r <= n_rates; r++) rate_first[r] = (size_t)rf[r];
    return VDF_OK;
}

// the rate checks of the several-rates library call, behind windows_clips_checks' (whose window counts are the plain ones, per block)
static int windows_clips_rates_checks(vdf_ctx *ctx, const vdf_windows_clips_rates_job *job)
{
    const vdf::WindowsMixedRatesCheck chk =
        vdf::check_windows_mixed_rates(job->n_frames, job->n_videos, job->window_stride, job->n_rates, job->rate_num, job->rate_den);
    switch (chk.error) {
    case vdf::WindowsMixedRatesError::kRateCount:
        return fail(ctx, VDF_E_INVAL, job->n_rates == 0 || job->n_rates > VDF_WINDOWS_MAX_RATES ? "n_rates outside 1 ... 8" : "null rate array");
    case vdf::WindowsMixedRatesError::kBadRate:
        return fail(ctx, VDF_E_INVAL, "rate outside 1 <= den <= num <= 2 den, num <= 65535 (rate " + std::to_string(chk.rate) + ")");
    case vdf::WindowsMixedRatesError::kShorterThanSpan:
        return fail(ctx, VDF_E_NOT_ENOUGH_FRAMES,
                    "fewer frames than a retimed window spans (rate " + std::to_string(chk.rate) + ", video " + std::to_string(chk.video) + ")");
    case vdf::WindowsMixedRatesError::kTooManyRows: return fail(ctx, VDF_E_INVAL, "2^32 windows or more in one call");
    case vdf::WindowsMixedRatesError::kNone: break;
    }
    return VDF_OK;
}

// windows_clips_checks and windows_clips_rates_checks have passed.  Uniform input: the uniform rates call, whose rows coincide.  Otherwise
// hash_windows_clips_retimed_locked's steps - the one blob through the pinned staging, here with the row table behind the segment table, the mixed
// whole-line kernels into `small`, the event wait on the staging - with dct_hash_windows_mixed_rates_kernel hashing every rate's windows from there.
static int hash_windows_clips_rates_locked(vdf_ctx *ctx, const uint8_t *d_buf, const vdf_windows_clips_rates_job *job, const vdf::WindowsMixedRatesPlan &plan,
                                           uint64_t *d_out, uint32_t *d_dc, hipStream_t stream)
{
    const size_t n_videos = job->n_videos;
    if (plan.kind == vdf::WindowsMixedRatesPlan::kUniform) {
        vdf_windows_rates_job u{};
        u.frames = d_buf + plan.offset0;
        u.n_clips = n_videos;
        u.frames_per_clip = job->n_frames[0];
        u.w = job->clips[0].w;
        u.h = job->clips[0].h;
        u.frame_stride = (size_t)job->clips[0].frame_stride;
        u.clip_stride = (size_t)plan.clip_stride;
        u.window_stride = job->window_stride;
        if (!plan.uniform.ok) return fail(ctx, VDF_E_INVAL, "internal: a list of rates that passed the checks was not planned");
        return hash_windows_rates_locked(ctx, u.frames, &u, plan.uniform, d_out, d_dc, stream);
    }
    const vdf::WindowsVideoRecord *d_videos = nullptr;
    const uint32_t *d_seg_first = nullptr;
    const void *d_row0 = nullptr;
    hipError_t e = hipSuccess;
    if (int rc = windows_clips_stage(ctx, d_buf, job->buf_bytes, plan, n_videos, stream, &d_videos, &d_seg_first, &e, plan.row0.data(),
                                     plan.row0.size() * sizeof(uint32_t), &d_row0))
        return rc;
    if (e == hipSuccess)
        e = vdf::launch_dct_hash_windows_mixed_rates(ctx->small.as<uint8_t>(), d_videos, d_seg_first, static_cast<const uint32_t *>(d_row0), (uint32_t)n_videos,
                                                     plan.seg_first[n_videos], plan.stride, plan.per_seg, plan.a, ctx->cos_table.as<double>(), d_out, d_dc, stream);
    return windows_clips_staged_end(ctx, e, "mixed rates windows launch");
}

int vdf_hash_windows_clips_u8_rates_device(vdf_ctx *ctx, const vdf_windows_clips_rates_job *job)
{
    if (!ctx || !job) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const hipStream_t s = job->stream ? (hipStream_t)job->stream : ctx->stream;
    bool run;
    if (int rc = windows_clips_checks(ctx, job->buf, job->buf_bytes, job->clips, job->n_frames, job->n_videos, job->window_stride, job->out_hashes, nullptr, false, s,
                                      &run))
        return rc;
    if (int rc = windows_clips_rates_checks(ctx, job)) return rc;
    if (!run) return VDF_OK;
    // the rates travel to the kernel inside the plan, by value, and the row table through the staging: the caller's arrays are not read after this
    const vdf::WindowsMixedRatesPlan plan = vdf::plan_windows_mixed_rates(reinterpret_cast<const vdf::MixedClip *>(job->clips), job->n_frames, job->n_videos,
                                                                          job->window_stride, job->n_rates, job->rate_num, job->rate_den);
    return hash_windows_clips_rates_locked(ctx, job->buf, job, plan, job->out_hashes, job->out_dontcare, s);
}

// Host arrays: as vdf_hash_windows_clips_u8_retimed - the buffer goes up ONCE, the device form's work runs on it, all blocks come down.
int vdf_hash_windows_clips_u8_rates(vdf_ctx *ctx, const vdf_windows_clips_rates_job *job)
{
    if (!ctx || !job) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    bool run;
    if (int rc = windows_clips_checks(ctx, job->buf, job->buf_bytes, job->clips, job->n_frames, job->n_videos, job->window_stride, job->out_hashes, nullptr, false,
                                      ctx->stream, &run))
        return rc;
    if (int rc = windows_clips_rates_checks(ctx, job)) return rc;
    if (!run) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    const vdf::WindowsMixedRatesPlan plan = vdf::plan_windows_mixed_rates(reinterpret_cast<const vdf::MixedClip *>(job->clips), job->n_frames, job->n_videos,
                                                                          job->window_stride, job->n_rates, job->rate_num, job->rate_den);
    const size_t n_out = (size_t)plan.rate_first[job->n_rates];
    const size_t hash_bytes = n_out * VDF_HASH_WORDS * sizeof(uint64_t);
    if (int rc = upload(ctx, ctx->frames, job->buf, job->buf_bytes, ctx->stream)) return rc;
    VDF_HIP(ctx, ctx->out_hashes.reserve(hash_bytes));
    if (job->out_dontcare) VDF_HIP(ctx, ctx->out_dc.reserve(n_out * sizeof(uint32_t)));
    uint32_t *d_dc = job->out_dontcare ? ctx->out_dc.as<uint32_t>() : nullptr;
    if (int rc = hash_windows_clips_rates_locked(ctx, ctx->frames.as<uint8_t>(), job, plan, ctx->out_hashes.as<uint64_t>(), d_dc, ctx->stream)) return rc;
    VDF_HIP(ctx, hipMemcpyAsync(job->out_hashes, ctx->out_hashes.p, hash_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (job->out_dontcare) VDF_HIP(ctx, hipMemcpyAsync(job->out_dontcare, d_dc, n_out * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VDF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VDF_OK;
}

// the argument checks both window-variant forms share, in the order their messages are reported; first on the host (null: not checked here)
static int window_variants_checks(vdf_ctx *ctx, const void *hashes, const void *zero, const void *first_ptr, const uint32_t *first, size_t n_videos,
                                  const void *skip, uint32_t variant, const void *out_hashes, const void *out_skip)
{
    if (variant == 0 || variant >= vdf::kHashVariants) return fail(ctx, VDF_E_INVAL, "variant outside 1 ... 7");
    if (n_videos == 0) return VDF_OK;
    if (!hashes || !zero || !first_ptr || !out_hashes || (skip == nullptr) != (out_skip == nullptr)) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (out_hashes == hashes || out_hashes == zero || (skip && out_skip == skip)) return fail(ctx, VDF_E_INVAL, "the variants are not made in place");
    if (n_videos >= 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "more than 2^32-2 videos");
    for (size_t v = 0; first && v < n_videos; v++)
        if (first[v + 1] < first[v]) return fail(ctx, VDF_E_INVAL, "the first array decreases at video " + std::to_string(v));
    return VDF_OK;
}

// rows [first[0], first[n_videos]) of out from hashes / zero / skip: the kernel's rule (window_variant.h) in plain C++
static void window_variants_rows_host(const uint64_t *hashes, const uint64_t *zero, const uint32_t *first, size_t n_videos, const uint8_t *skip,
                                      uint32_t variant, uint64_t *out_hashes, uint8_t *out_skip)
{
    for (uint32_t row = first[0]; row < first[n_videos]; row++) {
        const uint32_t src = vdf::window_variant_source(first, (uint32_t)n_videos, row, variant);
        for (int k = 0; k < VDF_HASH_WORDS; k++)
            out_hashes[(size_t)row * 16 + k] = (hashes[(size_t)src * 16 + k] ^ vdf::kVariantMasks.m[variant][k]) & ~zero[(size_t)src * 16 + k];
        if (skip) out_skip[row] = skip[src];
    }
}

int vdf_window_variants_host(const uint64_t *hashes, const uint64_t *zero, const uint32_t *first, size_t n_videos, const uint8_t *skip, uint32_t variant,
                             uint64_t *out_hashes, uint8_t *out_skip)
{
    if (int rc = window_variants_checks(nullptr, hashes, zero, first, first, n_videos, skip, variant, out_hashes, out_skip)) return rc;
    if (n_videos) window_variants_rows_host(hashes, zero, first, n_videos, skip, variant, out_hashes, out_skip);
    return VDF_OK;
}

int vdf_window_variants_device(vdf_ctx *ctx, const uint64_t *d_hashes, const uint64_t *d_zero, const uint32_t *d_first, size_t n_videos,
                               const uint8_t *d_skip, uint32_t variant, uint64_t *d_out_hashes, uint8_t *d_out_skip, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int rc = window_variants_checks(ctx, d_hashes, d_zero, d_first, nullptr, n_videos, d_skip, variant, d_out_hashes, d_out_skip)) return rc;
    if (n_videos == 0) return VDF_OK;
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "vdf_window_variants_device takes a single-device context");
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    std::vector<uint32_t> first(n_videos + 1);
    VDF_HIP(ctx, hipMemcpyAsync(first.data(), d_first, first.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipStreamSynchronize(s));
    if (int rc = window_variants_checks(ctx, d_hashes, d_zero, d_first, first.data(), n_videos, d_skip, variant, d_out_hashes, d_out_skip)) return rc;
    VDF_HIP(ctx, vdf::launch_window_variants(d_hashes, d_zero, d_first, (uint32_t)n_videos, d_skip, variant, first[0], first[n_videos] - first[0], d_out_hashes,
                                             d_out_skip, s));
    return VDF_OK;
}

// behind align_checks: the mask, then the zero plane of the side that is flipped
static int align_variants_checks(vdf_ctx *ctx, uint32_t variant_mask, size_t n_flipped, const void *zero)
{
    if ((variant_mask & ~0xFEu) != 0) return fail(ctx, VDF_E_INVAL, "variant_mask takes bits 1 ... 7");
    if (n_flipped && !zero) return fail(ctx, VDF_E_INVAL, "the flipped side has no zero plane");
    return VDF_OK;
}

static vdf_alignment_variant alignment_of_variant(const vdf_alignment &r, uint32_t variant)
{
    return vdf_alignment_variant{r.a, r.b, r.offset, r.start_a, r.n_windows, r.dist_sum, variant};
}

int vdf_align_windows_variants_host(const uint64_t *a_hashes, const uint64_t *a_zero, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                    const uint64_t *b_hashes, const uint64_t *b_zero, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                                    uint32_t tol_int, uint32_t min_run, uint32_t variant_mask, vdf_alignment_variant *out, size_t capacity, size_t *n_out)
{
    if (int rc = align_checks(nullptr, a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first, b_first, min_run, out, capacity, n_out)) return rc;
    const bool self = b_hashes == nullptr;
    if (self) { b_hashes = a_hashes; b_zero = a_zero; b_first = a_first; n_b = n_a; b_skip = a_skip; }
    if (int rc = align_variants_checks(nullptr, variant_mask, n_b, b_zero)) return rc;
    *n_out = 0;
    if (n_a == 0 || (self ? n_a < 2 : n_b == 0)) return VDF_OK;
    const uint32_t tol = std::min<uint32_t>(tol_int, 1024u);
    std::vector<uint64_t> derived((size_t)b_first[n_b] * 16);  // one buffer, re-used by every variant; rows below b_first[0] stay unused
    std::vector<uint8_t> derived_skip(b_skip ? b_first[n_b] : 0);
    size_t found = 0;
    for (uint32_t v = 1; v < vdf::kHashVariants; v++) {
        if (!(variant_mask >> v & 1u)) continue;
        window_variants_rows_host(b_hashes, b_zero, b_first, n_b, b_skip, v, derived.data(), b_skip ? derived_skip.data() : nullptr);
        for (size_t a = 0; a < n_a; a++)
            for (size_t b = self ? a + 1 : 0; b < n_b; b++) {
                vdf_alignment r;
                align_pair_host(a_hashes + 16 * (size_t)a_first[a], a_first[a + 1] - a_first[a], a_skip ? a_skip + a_first[a] : nullptr,
                                derived.data() + 16 * (size_t)b_first[b], b_first[b + 1] - b_first[b], b_skip ? derived_skip.data() + b_first[b] : nullptr, tol,
                                min_run, &r);
                if (r.n_windows == 0) continue;
                r.a = (uint32_t)a; r.b = (uint32_t)b;
                if (found < capacity) out[found] = alignment_of_variant(r, v);
                found++;
            }
    }
    *n_out = found;
    return VDF_OK;
}

// One align per requested variant, ascending: the variant set of B derived into the context's scratch (hashes, then skip bytes; all variants re-use
// it), then the align core on (A, derived B).  align_checks and align_variants_checks have passed; every array pointer is a device pointer, the
// first arrays are also on the host.  self: B's pointers are A's.
static int align_variants_locked(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint32_t *d_a_first, const uint32_t *h_first_a, size_t n_a,
                                 const uint8_t *d_a_skip, const uint64_t *d_b_hashes, const uint64_t *d_b_zero, const uint32_t *d_b_first,
                                 const uint32_t *h_first_b, size_t n_b, const uint8_t *d_b_skip, bool self, uint32_t tol_int, uint32_t min_run,
                                 uint32_t variant_mask, vdf_alignment_variant *out, size_t capacity, size_t *n_out, hipStream_t s)
{
    const uint32_t row0 = h_first_b[0], row_end = h_first_b[n_b];
    const size_t hash_bytes = (size_t)row_end * VDF_HASH_WORDS * sizeof(uint64_t);
    VDF_HIP(ctx, ctx->variant_hashes.reserve(hash_bytes + (d_b_skip ? row_end : 0) + 16));
    uint64_t *d_var = ctx->variant_hashes.as<uint64_t>();
    uint8_t *d_var_skip = d_b_skip ? ctx->variant_hashes.as<uint8_t>() + hash_bytes : nullptr;
    const size_t n_pairs = vdf::align_pair_count(n_a, n_b, self);
    std::vector<vdf_alignment> records;
    size_t found = 0;
    for (uint32_t v = 1; v < vdf::kHashVariants; v++) {
        if (!(variant_mask >> v & 1u)) continue;
        VDF_HIP(ctx, vdf::launch_window_variants(d_b_hashes, d_b_zero, d_b_first, (uint32_t)n_b, d_b_skip, v, row0, row_end - row0, d_var, d_var_skip, s));
        records.resize(std::min(capacity > found ? capacity - found : 0, n_pairs));
        size_t n_v = 0;
        if (int rc = align_locked(ctx, d_a_hashes, d_a_first, h_first_a, n_a, d_a_skip, d_var, d_b_first, h_first_b, n_b, d_var_skip, self, tol_int, min_run,
                                  records.data(), records.size(), &n_v, s))
            return rc;
        for (size_t i = 0; i < std::min(n_v, records.size()); i++) out[found + i] = alignment_of_variant(records[i], v);
        found += n_v;
    }
    VDF_HIP(ctx, hipStreamSynchronize(s));  // (a variant without a pair to align leaves only its derive kernel behind)
    *n_out = found;
    return VDF_OK;
}

int vdf_align_windows_variants_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint64_t *d_a_zero, const uint32_t *d_a_first, size_t n_a,
                                      const uint8_t *d_a_skip, const uint64_t *d_b_hashes, const uint64_t *d_b_zero, const uint32_t *d_b_first, size_t n_b,
                                      const uint8_t *d_b_skip, uint32_t tol_int, uint32_t min_run, uint32_t variant_mask, vdf_alignment_variant *out,
                                      size_t capacity, size_t *n_out, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const bool self = d_b_hashes == nullptr;
    const auto late_checks = [&]() -> int {
        if (int rc = align_variants_checks(ctx, variant_mask, self ? n_a : n_b, self ? d_a_zero : d_b_zero)) return rc;
        if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "vdf_align_windows_variants_device takes a single-device context");
        return VDF_OK;
    };
    // as vdf_align_windows_device: everything that can be said without the first arrays; then they come down, are checked, and plan the launch
    if (int rc = align_checks(ctx, d_a_hashes, nullptr, n_a, d_b_hashes, nullptr, n_b, d_a_first, d_b_first, min_run, out, capacity, n_out)) return rc;
    if (n_a == 0 || (self ? n_a < 2 : n_b == 0) || !ctx->subs.empty()) {  // nothing to read back, or no device to read it from
        if (int rc = late_checks()) return rc;
        *n_out = 0;
        return VDF_OK;
    }
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    std::vector<uint32_t> fa(n_a + 1), fb(self ? 0 : n_b + 1);
    VDF_HIP(ctx, hipMemcpyAsync(fa.data(), d_a_first, fa.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (!self) VDF_HIP(ctx, hipMemcpyAsync(fb.data(), d_b_first, fb.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipStreamSynchronize(s));
    if (int rc = align_checks(ctx, d_a_hashes, fa.data(), n_a, d_b_hashes, self ? nullptr : fb.data(), n_b, d_a_first, d_b_first, min_run, out, capacity, n_out))
        return rc;
    if (int rc = late_checks()) return rc;
    *n_out = 0;
    if (self) return align_variants_locked(ctx, d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, d_a_hashes, d_a_zero, d_a_first, fa.data(), n_a, d_a_skip, true,
                                           tol_int, min_run, variant_mask, out, capacity, n_out, s);
    return align_variants_locked(ctx, d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, d_b_hashes, d_b_zero, d_b_first, fb.data(), n_b, d_b_skip, false, tol_int,
                                 min_run, variant_mask, out, capacity, n_out, s);
}

// Host arrays: as vdf_align_windows, and the zero plane of the flipped side goes up beside its hashes.
int vdf_align_windows_variants(vdf_ctx *ctx, const uint64_t *a_hashes, const uint64_t *a_zero, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                               const uint64_t *b_hashes, const uint64_t *b_zero, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, uint32_t tol_int,
                               uint32_t min_run, uint32_t variant_mask, vdf_alignment_variant *out, size_t capacity, size_t *n_out)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int rc = align_checks(ctx, a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first, b_first, min_run, out, capacity, n_out)) return rc;
    const bool self = b_hashes == nullptr;
    const uint64_t *zero = self ? a_zero : b_zero;
    const uint32_t *zero_first = self ? a_first : b_first;
    const size_t n_flipped = self ? n_a : n_b;
    if (int rc = align_variants_checks(ctx, variant_mask, n_flipped, zero)) return rc;
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "vdf_align_windows_variants takes a single-device context");
    *n_out = 0;
    if (n_a == 0 || (self ? n_a < 2 : n_b == 0)) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    AlignUploaded u;
    if (int rc = align_upload(ctx, a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip, self, s, &u)) return rc;
    if (int rc = upload(ctx, ctx->up_zero, zero + 16 * (size_t)zero_first[0], (size_t)(zero_first[n_flipped] - zero_first[0]) * 16 * sizeof(uint64_t), s)) return rc;
    if (self) return align_variants_locked(ctx, ctx->up_hashes.as<uint64_t>(), u.d_fa, u.fa.data(), n_a, u.d_ska, ctx->up_hashes.as<uint64_t>(),
                                           ctx->up_zero.as<uint64_t>(), u.d_fa, u.fa.data(), n_a, u.d_ska, true, tol_int, min_run, variant_mask, out, capacity,
                                           n_out, s);
    return align_variants_locked(ctx, ctx->up_hashes.as<uint64_t>(), u.d_fa, u.fa.data(), n_a, u.d_ska, ctx->up_ref_hashes.as<uint64_t>(),
                                 ctx->up_zero.as<uint64_t>(), u.d_fb, u.fb.data(), n_b, u.d_skb, false, tol_int, min_run, variant_mask, out, capacity, n_out, s);
}

// ---- the flipped alignment, seeded and on a list of (variant, a, b) triples (include/vdf.h) -------------------------------------
// The checks of both calls in the order include/vdf.h gives them.  first arrays on the host, or null (a device form before they have come
// down).  late: the checks behind the first arrays too - the mask, the zero plane of the flipped side, the multi-GPU refusal.
static int align_flipped_seed_checks(vdf_ctx *ctx, const char *name, bool listed, const void *a_hashes, const uint32_t *a_first, size_t n_a,
                                     const void *b_hashes, const uint32_t *b_first, size_t n_b, const void *a_first_ptr, const void *b_first_ptr,
                                     const void *a_zero, const void *b_zero, const vdf_video_pair_variant *triples, size_t n_triples,
                                     uint32_t variant_mask, uint32_t min_run, const void *out, size_t capacity, const size_t *n_out, bool late,
                                     bool device_ctx)
{
    const bool self = b_hashes == nullptr;
    if (listed) {
        if (n_triples && !triples) return fail(ctx, VDF_E_INVAL, "null triple list");
        if (int rc = align_checks(ctx, a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first_ptr, b_first_ptr, min_run, out, capacity, n_out, &n_triples, "triples")) return rc;
        size_t at = 0;
        switch (vdf::align_triple_list_check(triples, n_triples, n_a, n_b, self, &at)) {
        case 1: return fail(ctx, VDF_E_INVAL, "the triple list is not strictly increasing in (variant, a, b) at entry " + std::to_string(at));
        case 4: return fail(ctx, VDF_E_INVAL, "triple " + std::to_string(at) + " of the list has a variant outside 1 ... 7");
        case 2: return fail(ctx, VDF_E_INVAL, "triple " + std::to_string(at) + " of the list names a video that does not exist");
        case 3: return fail(ctx, VDF_E_INVAL, "triple " + std::to_string(at) + " of the list has a >= b in self mode");
        default: break;
        }
    } else if (int rc = align_checks(ctx, a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first_ptr, b_first_ptr, min_run, out, capacity, n_out)) {
        return rc;
    }
    if (!late) return VDF_OK;
    if (int rc = align_variants_checks(ctx, listed ? 0u : variant_mask, self ? n_a : n_b, self ? a_zero : b_zero)) return rc;
    if (device_ctx && !ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, std::string(name) + " takes a single-device context");
    return VDF_OK;
}

static bool align_flipped_seed_trivial(bool listed, size_t n_a, size_t n_b, bool self, size_t n_triples)
{
    return listed ? n_triples == 0 : (n_a == 0 || (self ? n_a < 2 : n_b == 0));
}

// The host forms state the definitions directly: the variant set by the rule of vdf_window_variants_host, then the plain definitions
// (seed_pair_host, align_pair_host) on (A, derived B); in self mode the pairs a < b of A against the derived A.
static int align_flipped_seed_host_impl(bool listed, const uint64_t *a_hashes, const uint64_t *a_zero, const uint32_t *a_first, size_t n_a,
                                        const uint8_t *a_skip, const uint64_t *b_hashes, const uint64_t *b_zero, const uint32_t *b_first, size_t n_b,
                                        const uint8_t *b_skip, const vdf_video_pair_variant *triples, size_t n_triples, uint32_t tol_int, uint32_t min_run,
                                        uint32_t variant_mask, vdf_video_pair_variant *out_pairs, vdf_alignment_variant *out_records, size_t capacity,
                                        size_t *n_out)
{
    const void *o = listed ? (const void *)out_records : (const void *)out_pairs;
    if (int rc = align_flipped_seed_checks(nullptr, "", listed, a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first, b_first, a_zero, b_zero, triples,
                                           n_triples, variant_mask, min_run, o, capacity, n_out, true, false))
        return rc;
    const bool self = b_hashes == nullptr;
    *n_out = 0;
    if (align_flipped_seed_trivial(listed, n_a, n_b, self, n_triples)) return VDF_OK;
    if (self) { b_hashes = a_hashes; b_zero = a_zero; b_first = a_first; n_b = n_a; b_skip = a_skip; }
    const uint32_t tol = std::min<uint32_t>(tol_int, 1024u);
    std::vector<uint64_t> derived((size_t)b_first[n_b] * 16);
    std::vector<uint8_t> derived_skip(b_skip ? b_first[n_b] : 0);
    const auto side_a = [&](size_t a, const uint64_t **h, uint32_t *n, const uint8_t **sk) {
        *h = a_hashes + 16 * (size_t)a_first[a]; *n = a_first[a + 1] - a_first[a]; *sk = a_skip ? a_skip + a_first[a] : nullptr;
    };
    const auto side_b = [&](size_t b, const uint64_t **h, uint32_t *n, const uint8_t **sk) {
        *h = derived.data() + 16 * (size_t)b_first[b]; *n = b_first[b + 1] - b_first[b]; *sk = b_skip ? derived_skip.data() + b_first[b] : nullptr;
    };
    size_t found = 0, at = 0;
    for (uint32_t v = 1; v < vdf::kHashVariants; v++) {
        size_t end = at;
        if (listed) {
            while (end < n_triples && triples[end].variant == v) end++;
            if (end == at) continue;
        } else if (!(variant_mask >> v & 1u)) {
            continue;
        }
        window_variants_rows_host(b_hashes, b_zero, b_first, n_b, b_skip, v, derived.data(), b_skip ? derived_skip.data() : nullptr);
        const uint64_t *ha, *hb;
        const uint8_t *ska, *skb;
        uint32_t Na, Nb;
        if (listed) {
            for (; at < end; at++) {
                side_a(triples[at].a, &ha, &Na, &ska);
                side_b(triples[at].b, &hb, &Nb, &skb);
                vdf_alignment r;
                align_pair_host(ha, Na, ska, hb, Nb, skb, tol, min_run, &r);
                if (r.n_windows == 0) continue;
                r.a = triples[at].a; r.b = triples[at].b;
                if (found < capacity) out_records[found] = alignment_of_variant(r, v);
                found++;
            }
            continue;
        }
        for (size_t a = 0; a < n_a; a++)
            for (size_t b = self ? a + 1 : 0; b < n_b; b++) {
                side_a(a, &ha, &Na, &ska);
                side_b(b, &hb, &Nb, &skb);
                if (!seed_pair_host(ha, Na, ska, hb, Nb, skb, tol, min_run)) continue;
                if (found < capacity) out_pairs[found] = vdf_video_pair_variant{(uint32_t)a, (uint32_t)b, v};
                found++;
            }
    }
    *n_out = found;
    return VDF_OK;
}

// The seed pass against the variants.  The checks have passed on the host copies of the first arrays; every array pointer of `in` and d_b_zero
// (the zero plane that goes with in.d_b_hashes) is a device pointer.  Seeds and rows go into their class-major form, the bitmap's requested
// slots are cleared on the call's stream, ONE seed kernel marks every requested variant, count + scan give the total; the host reads it, then
// the first min(total, capacity) triples.
static int align_seed_variants_locked(vdf_ctx *ctx, const AlignSides &in, const uint64_t *d_b_zero, uint32_t tol_int, uint32_t min_run,
                                      uint32_t variant_mask, vdf_video_pair_variant *out, size_t capacity, size_t *n_out, hipStream_t s)
{
    *n_out = 0;
    const uint32_t n_slots = (uint32_t)__builtin_popcount(variant_mask);
    vdf::AlignSeedPlan plan;
    vdf::align_seed_plan(in.h_first_a, in.n_a, in.h_first_b, in.n_b, in.self, min_run, plan, vdf::kSeedVariantsTileRows);
    if (n_slots == 0 || plan.n_units() == 0) return VDF_OK;
    const uint64_t n_bits = (uint64_t)n_slots * in.n_a * in.n_b;  // <= 7 (2^25 + 2^13): align_checks
    const uint32_t n_words = (uint32_t)((n_bits + 31) / 32);
    const size_t n_seeds = plan.n_seeds(), n_chunks = plan.n_chunks();
    const size_t at_video = n_seeds * 4, at_row = at_video + n_seeds * 4, at_tile = at_row + (size_t)plan.n_rows * 4;
    const size_t at_unit = (at_tile + n_chunks * 4 + 7) & ~(size_t)7, plan_bytes = at_unit + (n_chunks + 1) * 8;
    const size_t seed_bytes = n_seeds * vdf::kClassSeedStride * 4, row_bytes = (size_t)plan.n_rows * vdf::kClassRowStride * 4;  // multiples of 16
    VDF_HIP(ctx, ctx->seed_bitmap.reserve((size_t)n_words * 4));
    VDF_HIP(ctx, ctx->seed_plan.reserve(plan_bytes));
    VDF_HIP(ctx, ctx->seed_classes.reserve(seed_bytes + row_bytes));
    VDF_HIP(ctx, ctx->align_scratch.reserve(vdf::align_seed_scratch_bytes(n_words)));
    char *dp = ctx->seed_plan.as<char>();
    uint32_t *d_seeds = ctx->seed_classes.as<uint32_t>(), *d_rows = d_seeds + n_seeds * vdf::kClassSeedStride;
    VDF_HIP(ctx, hipMemsetAsync(ctx->seed_bitmap.p, 0, (size_t)n_words * 4, s));
    VDF_HIP(ctx, hipMemcpyAsync(dp, plan.seed_window.data(), n_seeds * 4, hipMemcpyHostToDevice, s));
    VDF_HIP(ctx, hipMemcpyAsync(dp + at_video, plan.seed_video.data(), n_seeds * 4, hipMemcpyHostToDevice, s));
    VDF_HIP(ctx, hipMemcpyAsync(dp + at_row, plan.row_video.data(), (size_t)plan.n_rows * 4, hipMemcpyHostToDevice, s));
    VDF_HIP(ctx, hipMemcpyAsync(dp + at_tile, plan.tile_first.data(), n_chunks * 4, hipMemcpyHostToDevice, s));
    VDF_HIP(ctx, hipMemcpyAsync(dp + at_unit, plan.unit_offset.data(), (n_chunks + 1) * 8, hipMemcpyHostToDevice, s));
    VDF_HIP(ctx, vdf::launch_align_class_layout(reinterpret_cast<const uint32_t *>(in.d_a_hashes), nullptr, in.d_a_skip, reinterpret_cast<const uint32_t *>(dp),
                                                reinterpret_cast<const uint32_t *>(dp + at_video), 0, (uint32_t)n_seeds, d_seeds, s));
    VDF_HIP(ctx, vdf::launch_align_class_layout(reinterpret_cast<const uint32_t *>(in.d_b_hashes), reinterpret_cast<const uint32_t *>(d_b_zero), in.d_b_skip,
                                                nullptr, nullptr, plan.row_base, plan.n_rows, d_rows, s));
    uint32_t *d_total = nullptr;
    vdf::AlignSeedVariantsLaunch L{};
    L.seeds = d_seeds; L.n_seeds = (uint32_t)n_seeds;
    L.rows = d_rows; L.row_video = reinterpret_cast<const uint32_t *>(dp + at_row); L.n_rows = plan.n_rows;
    L.unit_offset = reinterpret_cast<const unsigned long long *>(dp + at_unit);
    L.tile_first = reinterpret_cast<const uint32_t *>(dp + at_tile);
    L.n_chunks = (uint32_t)n_chunks; L.n_units = plan.n_units();
    L.tol = std::min<uint32_t>(tol_int, 1024u); L.self_mode = in.self ? 1 : 0; L.variant_mask = variant_mask;
    L.n_a = (uint32_t)in.n_a; L.n_b = (uint32_t)in.n_b;
    L.bitmap = ctx->seed_bitmap.as<uint32_t>(); L.n_words = n_words;
    L.scratch = ctx->align_scratch.p; L.total_out = &d_total;
    VDF_HIP(ctx, vdf::launch_align_seed_variants(L, s));
    uint32_t total = 0;
    VDF_HIP(ctx, hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipStreamSynchronize(s));  // also: the plan arrays are free to go
    if ((uint64_t)total > n_bits) return fail(ctx, VDF_E_HIP, "align seed: more triples than bits");
    const size_t take = std::min<size_t>(total, capacity);
    if (take) {
        VDF_HIP(ctx, ctx->seed_out.reserve(take * sizeof(vdf_video_pair_variant)));
        VDF_HIP(ctx, vdf::launch_align_seed_variants_scatter(L, ctx->seed_out.as<vdf_video_pair_variant>(), (uint32_t)take, s));
        VDF_HIP(ctx, hipMemcpyAsync(out, ctx->seed_out.p, take * sizeof(vdf_video_pair_variant), hipMemcpyDeviceToHost, s));
        VDF_HIP(ctx, hipStreamSynchronize(s));
    }
    *n_out = total;
    return VDF_OK;
}

// align_variants_locked on a checked list: per variant present, ascending, the set is derived and the align core runs on that variant's
// contiguous sublist.
static int align_variants_pairs_locked(vdf_ctx *ctx, const AlignSides &in, const uint64_t *d_b_zero, const vdf_video_pair_variant *triples, size_t n_triples,
                                       uint32_t tol_int, uint32_t min_run, vdf_alignment_variant *out, size_t capacity, size_t *n_out, hipStream_t s)
{
    const uint32_t row0 = in.h_first_b[0], row_end = in.h_first_b[in.n_b];
    const size_t hash_bytes = (size_t)row_end * VDF_HASH_WORDS * sizeof(uint64_t);
    VDF_HIP(ctx, ctx->variant_hashes.reserve(hash_bytes + (in.d_b_skip ? row_end : 0) + 16));
    uint64_t *d_var = ctx->variant_hashes.as<uint64_t>();
    uint8_t *d_var_skip = in.d_b_skip ? ctx->variant_hashes.as<uint8_t>() + hash_bytes : nullptr;
    std::vector<vdf_video_pair> sub;
    std::vector<vdf_alignment> records;
    size_t found = 0;
    for (size_t at = 0; at < n_triples;) {
        const uint32_t v = triples[at].variant;
        sub.clear();
        for (; at < n_triples && triples[at].variant == v; at++) sub.push_back(vdf_video_pair{triples[at].a, triples[at].b});
        VDF_HIP(ctx, vdf::launch_window_variants(in.d_b_hashes, d_b_zero, in.d_b_first, (uint32_t)in.n_b, in.d_b_skip, v, row0, row_end - row0, d_var, d_var_skip, s));
        records.resize(std::min(capacity > found ? capacity - found : 0, sub.size()));
        size_t n_v = 0;
        if (int rc = align_locked(ctx, in.d_a_hashes, in.d_a_first, in.h_first_a, in.n_a, in.d_a_skip, d_var, in.d_b_first, in.h_first_b, in.n_b, d_var_skip,
                                  in.self, tol_int, min_run, records.data(), records.size(), &n_v, s, sub.data(), sub.size()))
            return rc;
        for (size_t i = 0; i < std::min(n_v, records.size()); i++) out[found + i] = alignment_of_variant(records[i], v);
        found += n_v;
    }
    VDF_HIP(ctx, hipStreamSynchronize(s));
    *n_out = found;
    return VDF_OK;
}

static int align_flipped_seed_run(vdf_ctx *ctx, bool listed, const AlignSides &in, const uint64_t *d_b_zero, const vdf_video_pair_variant *triples,
                                  size_t n_triples, uint32_t tol_int, uint32_t min_run, uint32_t variant_mask, vdf_video_pair_variant *out_pairs,
                                  vdf_alignment_variant *out_records, size_t capacity, size_t *n_out, hipStream_t s)
{
    if (listed) return align_variants_pairs_locked(ctx, in, d_b_zero, triples, n_triples, tol_int, min_run, out_records, capacity, n_out, s);
    return align_seed_variants_locked(ctx, in, d_b_zero, tol_int, min_run, variant_mask, out_pairs, capacity, n_out, s);
}

static int align_flipped_seed_device_impl(vdf_ctx *ctx, const char *name, bool listed, const uint64_t *d_a_hashes, const uint64_t *d_a_zero,
                                          const uint32_t *d_a_first, size_t n_a, const uint8_t *d_a_skip, const uint64_t *d_b_hashes,
                                          const uint64_t *d_b_zero, const uint32_t *d_b_first, size_t n_b, const uint8_t *d_b_skip,
                                          const vdf_video_pair_variant *triples, size_t n_triples, uint32_t tol_int, uint32_t min_run, uint32_t variant_mask,
                                          vdf_video_pair_variant *out_pairs, vdf_alignment_variant *out_records, size_t capacity, size_t *n_out, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const void *o = listed ? (const void *)out_records : (const void *)out_pairs;
    const bool self = d_b_hashes == nullptr;
    const auto checks = [&](const uint32_t *fa, const uint32_t *fb, bool late) {
        return align_flipped_seed_checks(ctx, name, listed, d_a_hashes, fa, n_a, d_b_hashes, fb, n_b, d_a_first, d_b_first, d_a_zero, d_b_zero, triples, n_triples,
                                         variant_mask, min_run, o, capacity, n_out, late, true);
    };
    // everything that can be said without the first arrays (the list form: all of it, the multi-GPU refusal last); then they come down and are checked
    if (int rc = checks(nullptr, nullptr, listed)) return rc;
    if (align_flipped_seed_trivial(listed, n_a, n_b, self, n_triples) || !ctx->subs.empty()) {  // nothing to read back, or no device to read it from
        if (int rc = checks(nullptr, nullptr, true)) return rc;
        *n_out = 0;
        return VDF_OK;
    }
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    std::vector<uint32_t> fa, fb;
    if (int rc = align_first_down(ctx, d_a_first, n_a, d_b_first, n_b, self, s, fa, fb)) return rc;
    if (int rc = checks(fa.data(), self ? nullptr : fb.data(), true)) return rc;
    *n_out = 0;
    const AlignSides in = self ? AlignSides{d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, true}
                               : AlignSides{d_a_hashes, d_a_first, fa.data(), n_a, d_a_skip, d_b_hashes, d_b_first, fb.data(), n_b, d_b_skip, false};
    return align_flipped_seed_run(ctx, listed, in, self ? d_a_zero : d_b_zero, triples, n_triples, tol_int, min_run, variant_mask, out_pairs, out_records,
                                  capacity, n_out, s);
}

// Host arrays: as vdf_align_windows_variants - the zero plane of the flipped side goes up beside its hashes.
static int align_flipped_seed_ctx_impl(vdf_ctx *ctx, const char *name, bool listed, const uint64_t *a_hashes, const uint64_t *a_zero, const uint32_t *a_first,
                                       size_t n_a, const uint8_t *a_skip, const uint64_t *b_hashes, const uint64_t *b_zero, const uint32_t *b_first, size_t n_b,
                                       const uint8_t *b_skip, const vdf_video_pair_variant *triples, size_t n_triples, uint32_t tol_int, uint32_t min_run,
                                       uint32_t variant_mask, vdf_video_pair_variant *out_pairs, vdf_alignment_variant *out_records, size_t capacity,
                                       size_t *n_out)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const void *o = listed ? (const void *)out_records : (const void *)out_pairs;
    if (int rc = align_flipped_seed_checks(ctx, name, listed, a_hashes, a_first, n_a, b_hashes, b_first, n_b, a_first, b_first, a_zero, b_zero, triples, n_triples,
                                           variant_mask, min_run, o, capacity, n_out, true, true))
        return rc;
    const bool self = b_hashes == nullptr;
    *n_out = 0;
    if (align_flipped_seed_trivial(listed, n_a, n_b, self, n_triples)) return VDF_OK;
    const uint64_t *zero = self ? a_zero : b_zero;
    const uint32_t *zero_first = self ? a_first : b_first;
    const size_t n_flipped = self ? n_a : n_b;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    AlignUploaded u;
    if (int rc = align_upload(ctx, a_hashes, a_first, n_a, a_skip, b_hashes, b_first, n_b, b_skip, self, s, &u)) return rc;
    if (int rc = upload(ctx, ctx->up_zero, zero + 16 * (size_t)zero_first[0], (size_t)(zero_first[n_flipped] - zero_first[0]) * 16 * sizeof(uint64_t), s)) return rc;
    return align_flipped_seed_run(ctx, listed, align_sides_uploaded(ctx, u, n_a, n_b, self), ctx->up_zero.as<uint64_t>(), triples, n_triples, tol_int, min_run,
                                  variant_mask, out_pairs, out_records, capacity, n_out, s);
}

int vdf_align_seed_pairs_variants_host(const uint64_t *a_hashes, const uint64_t *a_zero, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                       const uint64_t *b_hashes, const uint64_t *b_zero, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                                       uint32_t tol_int, uint32_t min_run, uint32_t variant_mask, vdf_video_pair_variant *out, size_t capacity, size_t *n_out)
{
    return align_flipped_seed_host_impl(false, a_hashes, a_zero, a_first, n_a, a_skip, b_hashes, b_zero, b_first, n_b, b_skip, nullptr, 0, tol_int, min_run,
                                        variant_mask, out, nullptr, capacity, n_out);
}

int vdf_align_seed_pairs_variants(vdf_ctx *ctx, const uint64_t *a_hashes, const uint64_t *a_zero, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                  const uint64_t *b_hashes, const uint64_t *b_zero, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip, uint32_t tol_int,
                                  uint32_t min_run, uint32_t variant_mask, vdf_video_pair_variant *out, size_t capacity, size_t *n_out)
{
    return align_flipped_seed_ctx_impl(ctx, "vdf_align_seed_pairs_variants", false, a_hashes, a_zero, a_first, n_a, a_skip, b_hashes, b_zero, b_first, n_b, b_skip,
                                       nullptr, 0, tol_int, min_run, variant_mask, out, nullptr, capacity, n_out);
}

int vdf_align_seed_pairs_variants_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint64_t *d_a_zero, const uint32_t *d_a_first, size_t n_a,
                                         const uint8_t *d_a_skip, const uint64_t *d_b_hashes, const uint64_t *d_b_zero, const uint32_t *d_b_first, size_t n_b,
                                         const uint8_t *d_b_skip, uint32_t tol_int, uint32_t min_run, uint32_t variant_mask, vdf_video_pair_variant *out,
                                         size_t capacity, size_t *n_out, void *stream)
{
    return align_flipped_seed_device_impl(ctx, "vdf_align_seed_pairs_variants_device", false, d_a_hashes, d_a_zero, d_a_first, n_a, d_a_skip, d_b_hashes, d_b_zero,
                                          d_b_first, n_b, d_b_skip, nullptr, 0, tol_int, min_run, variant_mask, out, nullptr, capacity, n_out, stream);
}

int vdf_align_windows_variants_pairs_host(const uint64_t *a_hashes, const uint64_t *a_zero, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                          const uint64_t *b_hashes, const uint64_t *b_zero, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                                          const vdf_video_pair_variant *triples, size_t n_triples, uint32_t tol_int, uint32_t min_run,
                                          vdf_alignment_variant *out, size_t capacity, size_t *n_out)
{
    return align_flipped_seed_host_impl(true, a_hashes, a_zero, a_first, n_a, a_skip, b_hashes, b_zero, b_first, n_b, b_skip, triples, n_triples, tol_int, min_run,
                                        0, nullptr, out, capacity, n_out);
}

int vdf_align_windows_variants_pairs(vdf_ctx *ctx, const uint64_t *a_hashes, const uint64_t *a_zero, const uint32_t *a_first, size_t n_a, const uint8_t *a_skip,
                                     const uint64_t *b_hashes, const uint64_t *b_zero, const uint32_t *b_first, size_t n_b, const uint8_t *b_skip,
                                     const vdf_video_pair_variant *triples, size_t n_triples, uint32_t tol_int, uint32_t min_run, vdf_alignment_variant *out,
                                     size_t capacity, size_t *n_out)
{
    return align_flipped_seed_ctx_impl(ctx, "vdf_align_windows_variants_pairs", true, a_hashes, a_zero, a_first, n_a, a_skip, b_hashes, b_zero, b_first, n_b, b_skip,
                                       triples, n_triples, tol_int, min_run, 0, nullptr, out, capacity, n_out);
}

int vdf_align_windows_variants_pairs_device(vdf_ctx *ctx, const uint64_t *d_a_hashes, const uint64_t *d_a_zero, const uint32_t *d_a_first, size_t n_a,
                                            const uint8_t *d_a_skip, const uint64_t *d_b_hashes, const uint64_t *d_b_zero, const uint32_t *d_b_first, size_t n_b,
                                            const uint8_t *d_b_skip, const vdf_video_pair_variant *triples, size_t n_triples, uint32_t tol_int, uint32_t min_run,
                                            vdf_alignment_variant *out, size_t capacity, size_t *n_out, void *stream)
{
    return align_flipped_seed_device_impl(ctx, "vdf_align_windows_variants_pairs_device", true, d_a_hashes, d_a_zero, d_a_first, n_a, d_a_skip, d_b_hashes, d_b_zero,
                                          d_b_first, n_b, d_b_skip, triples, n_triples, tol_int, min_run, 0, nullptr, out, capacity, n_out, stream);
}

// ---- the class-major rows themselves (include/vdf.h: vdf_window_class_layout_*): what the seed pass against the variants reads,
// made reachable so that the layout kernel can be compared with its host twin word for word
static int class_layout_checks(vdf_ctx *ctx, const void *hashes, const void *first_ptr, const uint32_t *first, size_t n_videos, uint32_t min_run, const void *out,
                               const size_t *n_rows)
{
    if (!n_rows || (n_videos && (!hashes || !first_ptr))) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (min_run == 0) return fail(ctx, VDF_E_INVAL, "min_run of zero");
    if (n_videos > 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "more than 2^32 - 1 videos");
    for (size_t v = 0; first && v < n_videos; v++)
        if (first[v + 1] < first[v]) return fail(ctx, VDF_E_INVAL, "the first array decreases at video " + std::to_string(v));
    return VDF_OK;
}

// the seeds of a set (zero == null: window first[v] + k min_run of every video v) or its rows [first[0], first[n_videos])
static void class_layout_plan(const uint32_t *first, size_t n_videos, bool seeds, uint32_t min_run, std::vector<uint32_t> &window, std::vector<uint32_t> &video)
{
    window.clear(); video.clear();
    for (size_t v = 0; seeds && v < n_videos; v++)
        for (uint64_t w = first[v]; w < first[v + 1]; w += min_run) { window.push_back((uint32_t)w); video.push_back((uint32_t)v); }
}

int vdf_window_class_layout_host(const uint64_t *hashes, const uint64_t *zero, const uint32_t *first, size_t n_videos, const uint8_t *skip, uint32_t min_run,
                                 uint32_t *out, size_t capacity_rows, size_t *n_rows)
{
    if (int rc = class_layout_checks(nullptr, hashes, first, first, n_videos, min_run, out, n_rows)) return rc;
    *n_rows = 0;
    if (n_videos == 0) return VDF_OK;
    const uint32_t *h32 = reinterpret_cast<const uint32_t *>(hashes), *z32 = reinterpret_cast<const uint32_t *>(zero);
    std::vector<uint32_t> window, video;
    class_layout_plan(first, n_videos, zero == nullptr, min_run, window, video);
    const size_t n = zero ? first[n_videos] - first[0] : window.size();
    *n_rows = n;
    if (n > capacity_rows || (n && !out)) return VDF_E_INVAL;
    for (size_t r = 0; r < n; r++) {
        if (zero) {
            const size_t w = (size_t)first[0] + r;
            for (uint32_t q = 0; q < vdf::kClassRowStride; q++)
                out[r * vdf::kClassRowStride + q] = vdf::window_class_row_dword(h32 + w * 32, z32 + w * 32, skip ? skip[w] : 0u, q);
        } else {
            const size_t w = window[r];
            for (uint32_t q = 0; q < vdf::kClassSeedStride; q++)
                out[r * vdf::kClassSeedStride + q] = vdf::window_class_seed_dword(h32 + w * 32, skip ? skip[w] : 0u, video[r], q);
        }
    }
    return VDF_OK;
}

int vdf_window_class_layout_device(vdf_ctx *ctx, const uint64_t *d_hashes, const uint64_t *d_zero, const uint32_t *d_first, size_t n_videos, const uint8_t *d_skip,
                                   uint32_t min_run, uint32_t *d_out, size_t capacity_rows, size_t *n_rows, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int rc = class_layout_checks(ctx, d_hashes, d_first, nullptr, n_videos, min_run, d_out, n_rows)) return rc;
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "vdf_window_class_layout_device takes a single-device context");
    *n_rows = 0;
    if (n_videos == 0) return VDF_OK;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    std::vector<uint32_t> first(n_videos + 1);
    VDF_HIP(ctx, hipMemcpyAsync(first.data(), d_first, first.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VDF_HIP(ctx, hipStreamSynchronize(s));
    if (int rc = class_layout_checks(ctx, d_hashes, d_first, first.data(), n_videos, min_run, d_out, n_rows)) return rc;
    std::vector<uint32_t> window, video;
    class_layout_plan(first.data(), n_videos, d_zero == nullptr, min_run, window, video);
    const size_t n = d_zero ? first[n_videos] - first[0] : window.size();
    *n_rows = n;
    if (n > 0xFFFFFFFFull || n > capacity_rows || (n && !d_out)) return fail(ctx, VDF_E_INVAL, "the output holds fewer rows than the layout has");
    if (n == 0) return VDF_OK;
    const uint32_t *d_window = nullptr, *d_video = nullptr;
    if (!d_zero) {
        VDF_HIP(ctx, ctx->seed_plan.reserve(2 * n * 4));
        char *dp = ctx->seed_plan.as<char>();
        VDF_HIP(ctx, hipMemcpyAsync(dp, window.data(), n * 4, hipMemcpyHostToDevice, s));
        VDF_HIP(ctx, hipMemcpyAsync(dp + n * 4, video.data(), n * 4, hipMemcpyHostToDevice, s));
        d_window = reinterpret_cast<const uint32_t *>(dp); d_video = reinterpret_cast<const uint32_t *>(dp + n * 4);
    }
    VDF_HIP(ctx, vdf::launch_align_class_layout(reinterpret_cast<const uint32_t *>(d_hashes), reinterpret_cast<const uint32_t *>(d_zero), d_skip, d_window, d_video,
                                                first[0], (uint32_t)n, d_out, s));
    VDF_HIP(ctx, hipStreamSynchronize(s));  // the plan arrays are free to go; the rows are there
    return VDF_OK;
}

int vdf_hash_variant(const uint64_t *hash, const uint64_t *zero, uint32_t variant, uint64_t *out)
{
    if (!hash || !zero || !out || variant >= vdf::kHashVariants) return VDF_E_INVAL;
    for (int k = 0; k < VDF_HASH_WORDS; k++) out[k] = (hash[k] ^ vdf::kVariantMasks.m[variant][k]) & ~zero[k];
    return VDF_OK;
}

int vdf_hash_variants_device(vdf_ctx *ctx, const uint64_t *d_hashes, const uint64_t *d_zero, size_t n, uint32_t variant,
                             uint64_t *d_out, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    if (variant >= vdf::kHashVariants) return fail(ctx, VDF_E_INVAL, "variant above 7");
    if (n == 0) return VDF_OK;
    if (!d_hashes || !d_zero || !d_out) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (d_out == d_hashes || d_out == d_zero) return fail(ctx, VDF_E_INVAL, "the variants are not made in place");
    if (n >= 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "more than 2^32-1 hashes");
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    VDF_HIP(ctx, vdf::launch_hash_variants(d_hashes, d_zero, n, &variant, 1, d_out, stream ? (hipStream_t)stream : ctx->stream));
    return VDF_OK;
}

// One reference search per requested variant: V_v (derived into the context's scratch) against the plain hashes, the same durations on both
// sides; (r, r) dropped on the host, where the hit list is grouped anyway.
static int search_variants_locked(vdf_ctx *ctx, const uint64_t *d_hashes, const uint64_t *d_zero, const uint32_t *d_durations, size_t n,
                                  uint32_t tol_int, uint32_t variant_mask, vdf_groups *out, hipStream_t s)
{
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    VDF_HIP(ctx, ctx->variant_hashes.reserve(n * VDF_HASH_WORDS * 8));
    uint64_t *d_var = ctx->variant_hashes.as<uint64_t>();
    std::vector<vdf_hit> kept;
    for (uint32_t v = 1; v < vdf::kHashVariants; v++) {
        if (!(variant_mask >> v & 1u)) continue;
        VDF_HIP(ctx, vdf::launch_hash_variants(d_hashes, d_zero, n, &v, 1, d_var, s));
        uint64_t n_hits = 0, capacity = ctx->hit_capacity;
        int rc = VDF_OK;
        for (int attempt = 0; attempt < 6; attempt++) {  // every hit is output: size the list up (search_refs_resident)
            rc = search_refs_device_locked(ctx, d_hashes, d_durations, n, d_var, d_durations, n, tol_int, 0, nullptr, capacity, &n_hits, s, &ctx->host_hits);
            if (rc == VDF_E_OVERFLOW && n_hits > capacity) { capacity = n_hits; continue; }
            break;
        }
        if (rc) return rc;
        kept.clear();
        const vdf_hit *hits = ctx->host_hits.data();
        for (uint64_t i = 0; i < n_hits; i++)
            if (hits[i].row != hits[i].col) kept.push_back(hits[i]);
        if ((rc = vdf_groups_from_ref_hits(kept.data(), kept.size(), &out[v]))) return fail(ctx, rc, "grouping the hits of a variant");
    }
    return VDF_OK;
}

static int search_variants_checks(vdf_ctx *ctx, const void *hashes, const void *zero, const void *durations, size_t n, uint32_t variant_mask)
{
    if ((variant_mask & ~0xFEu) != 0) return fail(ctx, VDF_E_INVAL, "variant_mask takes bits 1 ... 7");
    if (n && (!hashes || !zero || !durations)) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (n >= 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "more than 2^32-1 hashes");
    return VDF_OK;
}

static void free_variant_groups(vdf_groups *out)
{
    for (uint32_t v = 0; v < vdf::kHashVariants; v++) vdf_groups_free(&out[v]);
}

int vdf_search_variants_device(vdf_ctx *ctx, const uint64_t *d_hashes, const uint64_t *d_zero, const uint32_t *d_durations,
                               size_t n, uint32_t tol_int, uint32_t variant_mask, vdf_groups *out, void *stream)
{
    if (!ctx || !out) return VDF_E_INVAL;
    std::memset(out, 0, vdf::kHashVariants * sizeof *out);
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    if (int rc = search_variants_checks(ctx, d_hashes, d_zero, d_durations, n, variant_mask)) return rc;
    if (n == 0) return VDF_OK;
    const int rc = search_variants_locked(ctx, d_hashes, d_zero, d_durations, n, tol_int, variant_mask, out, stream ? (hipStream_t)stream : ctx->stream);
    if (rc) free_variant_groups(out);
    return rc;
}

int vdf_search_variants(vdf_ctx *ctx, const uint64_t *hashes, const uint64_t *zero, const uint32_t *durations, size_t n,
                        uint32_t tol_int, uint32_t variant_mask, vdf_groups *out)
{
    if (!ctx || !out) return VDF_E_INVAL;
    std::memset(out, 0, vdf::kHashVariants * sizeof *out);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "vdf_search_variants takes a single-device context");
    if (int rc = search_variants_checks(ctx, hashes, zero, durations, n, variant_mask)) return rc;
    if (n == 0) return VDF_OK;
    if (!is_sorted_u32(durations, n)) return fail(ctx, VDF_E_INVAL, "durations are not ascending: pass the arrays in Search::sort order");
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    int rc = upload(ctx, ctx->up_hashes, hashes, n * VDF_HASH_WORDS * 8, ctx->stream);
    if (rc == VDF_OK) rc = upload(ctx, ctx->up_zero, zero, n * VDF_HASH_WORDS * 8, ctx->stream);
    if (rc == VDF_OK) rc = upload(ctx, ctx->up_dur, durations, n * 4, ctx->stream);
    if (rc == VDF_OK)
        rc = search_variants_locked(ctx, ctx->up_hashes.as<uint64_t>(), ctx->up_zero.as<uint64_t>(), ctx->up_dur.as<uint32_t>(), n, tol_int, variant_mask, out, ctx->stream);
    if (rc) free_variant_groups(out);
    return rc;
}

int vdf_cropdetect_letterbox_clips_device(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips, uint32_t frames_per_clip,
                                          uint32_t *d_crops, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    return cropdetect_clips_locked(ctx, d_buf, buf_bytes, clips, n_clips, frames_per_clip, d_crops, stream ? (hipStream_t)stream : ctx->stream);
}

int vdf_hash_clips_u8_letterbox_device(vdf_ctx *ctx, const uint8_t *d_buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips, uint32_t frames_per_clip,
                                       uint64_t *d_out_hashes, uint32_t *d_out_dontcare, uint32_t *out_crops, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    return letterbox_clips_locked(ctx, d_buf, buf_bytes, clips, n_clips, frames_per_clip, d_out_hashes, d_out_dontcare, out_crops,
                                  stream ? (hipStream_t)stream : ctx->stream);
}

int vdf_hash_clips_u8_letterbox(vdf_ctx *ctx, const uint8_t *buf, size_t buf_bytes, const vdf_clip *clips, size_t n_clips, uint32_t frames_per_clip,
                                uint64_t *out_hashes, uint32_t *out_crops, uint32_t *out_dontcare)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->subs.empty()) return fail(ctx, VDF_E_INVAL, "vdf_hash_clips_u8_letterbox takes a single-device context");
    return hash_clips_host_locked(ctx, buf, buf_bytes, clips, n_clips, frames_per_clip, out_hashes, out_dontcare, 1, out_crops);
}

int vdf_hash_frames_u8_letterbox_device(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                                        uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride,
                                        uint64_t *d_out_hashes, uint32_t *d_out_dontcare, uint32_t *out_crops,
                                        void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    return letterbox_hash_device_locked(ctx, d_frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride,
                                        d_out_hashes, d_out_dontcare, out_crops,
                                        stream ? (hipStream_t)stream : ctx->stream);
}

int vdf_hash_frames_u8_letterbox_device_async(vdf_ctx *ctx, const uint8_t *d_frames, size_t n_clips, uint32_t frames_per_clip,
                                              uint32_t w, uint32_t h, size_t frame_stride, size_t clip_stride,
                                              uint64_t *d_out_hashes, uint32_t *d_out_dontcare, uint32_t *d_out_crops,
                                              void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    return letterbox_hash_device_locked(ctx, d_frames, n_clips, frames_per_clip, w, h, frame_stride, clip_stride,
                                        d_out_hashes, d_out_dontcare, nullptr,
                                        stream ? (hipStream_t)stream : ctx->stream, d_out_crops);
}

int vdf_groups_max_distance(vdf_ctx *ctx, const uint64_t *hashes, size_t n, const uint64_t *ref_hashes, size_t n_ref,
                            const vdf_groups *groups, uint32_t *out_max)
{
    if (!ctx || !groups) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const uint64_t ng = groups->n_groups;
    if (ng == 0) return VDF_OK;
    if (!hashes || !out_max || !groups->offsets || !groups->members) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (ng > 0x7FFFFFFFull) return fail(ctx, VDF_E_INVAL, "too many groups");
    const uint64_t nm = groups->offsets[ng];
    for (uint64_t i = 0; i < nm; i++)
        if (groups->members[i] >= n) return fail(ctx, VDF_E_INVAL, "group member index out of range");
    const bool refs = ref_hashes && groups->ref_index;
    if (refs)
        for (uint64_t g = 0; g < ng; g++)
            if (groups->ref_index[g] >= (int64_t)n_ref) return fail(ctx, VDF_E_INVAL, "reference index out of range");
    // a multi-GPU context runs this small job on its first device (the parent itself owns no stream or scratch)
    vdf_ctx *d = device_ctx(ctx, 0);
    DeviceGuard restore_device;
    VDF_HIP(ctx, hipSetDevice(d->device));
    hipStream_t s = d->stream;
    DevBuf d_off, d_mem, d_ref, d_out;
    int rc = upload(d, d->up_hashes, hashes, n * VDF_HASH_WORDS * 8, s);
    if (rc == VDF_OK && refs) rc = upload(d, d->up_ref_hashes, ref_hashes, n_ref * VDF_HASH_WORDS * 8, s);
    if (rc == VDF_OK) rc = upload(d, d_off, groups->offsets, (ng + 1) * 8, s);
    if (rc == VDF_OK) rc = upload(d, d_mem, groups->members, std::max<uint64_t>(nm, 1) * 8, s);
    if (rc == VDF_OK && refs) rc = upload(d, d_ref, groups->ref_index, ng * 8, s);
    hipError_t e = rc == VDF_OK ? d_out.reserve(ng * 4) : hipSuccess;
    if (rc == VDF_OK && e == hipSuccess)
        e = vdf::launch_group_max_distance(d->up_hashes.as<uint32_t>(), d_off.as<unsigned long long>(),
                                           d_mem.as<unsigned long long>(),
                                           refs ? d->up_ref_hashes.as<uint32_t>() : nullptr,
                                           refs ? d_ref.as<long long>() : nullptr, (uint32_t)ng, d_out.as<uint32_t>(), s);
    if (rc == VDF_OK && e == hipSuccess) e = hipMemcpyAsync(out_max, d_out.p, ng * 4, hipMemcpyDeviceToHost, s);
    if (rc == VDF_OK && e == hipSuccess) e = hipStreamSynchronize(s);
    d_off.release(); d_mem.release(); d_ref.release(); d_out.release();
    if (rc) { if (d != ctx) ctx->err = d->err; return rc; }
    if (e != hipSuccess) return fail_hip(ctx, e, "vdf_groups_max_distance");
    return VDF_OK;
}


int vdf_search_self_device(vdf_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_durations, size_t n,
                           uint32_t tol_int, uint32_t shard_index, uint32_t shard_count, uint32_t row_begin,
                           uint32_t row_end, const uint32_t *d_matched, vdf_hit *hits, uint64_t capacity,
                           uint64_t *n_hits, uint32_t *overflow_row, void *stream)
{
    if (!ctx || !n_hits || !overflow_row || (capacity && !hits)) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    ctx->stats = vdf_search_stats{};
    ctx->timing = vdf_search_timing{};
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    return search_core(ctx, 0, d_hashes, d_durations, n, d_hashes, d_durations, nullptr, n, tol_int, shard_index,
                       shard_count, row_begin, row_end, d_matched, 0, hits, capacity, n_hits, overflow_row, s);
}

namespace {
// the caller's callbacks (include/vdf.h: vdf_shard_exchange) behind the library's exchange interface
struct CallbackExchange final : vdf_impl::ShardExchange {
    const vdf_shard_exchange *x;
    explicit CallbackExchange(const vdf_shard_exchange *x_) : x(x_) {}
    int agree(uint32_t, vdf_ctx *d, bool *all_complete, uint64_t *total_hits) override
    {
        int c = *all_complete ? 1 : 0;
        const int rc = x->agree(x->user, &c, total_hits);
        if (rc) return fail(d, rc, "the shard exchange's agree callback failed");
        *all_complete = c != 0;
        return VDF_OK;
    }
    int or_bitmap(uint32_t, vdf_ctx *d, uint32_t *d_bitmap, size_t n_words, hipStream_t stream) override
    {
        const int rc = x->or_bitmap(x->user, d_bitmap, n_words, (void *)stream);
        if (rc) return fail(d, rc, "the shard exchange's or_bitmap callback failed");
        return VDF_OK;
    }
};
}  // namespace

int vdf_search_self_device_replay(vdf_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_durations, size_t n,
                                  uint32_t tol_int, uint32_t shard_index, uint32_t shard_count, uint32_t row_begin,
                                  uint32_t row_end, const uint32_t *d_matched, vdf_hit *hits, uint64_t capacity,
                                  uint64_t *n_hits, uint32_t *overflow_row, const vdf_shard_exchange *xchg, void *stream)
{
    if (!ctx || !n_hits || !overflow_row || (capacity && !hits)) return VDF_E_INVAL;
    if (xchg && (!xchg->agree || !xchg->or_bitmap)) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    ctx->stats = vdf_search_stats{};
    ctx->timing = vdf_search_timing{};
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    CallbackExchange fx(xchg);
    return search_core(ctx, 0, d_hashes, d_durations, n, d_hashes, d_durations, nullptr, n, tol_int, shard_index,
                       shard_count, row_begin, row_end, d_matched, 0, hits, capacity, n_hits, overflow_row, s,
                       /*replay_only=*/true, nullptr, xchg ? &fx : nullptr);
}

int vdf_bitmap_or_device(vdf_ctx *ctx, uint32_t *d_dst, const uint32_t *d_srcs, size_t n_words, uint32_t n_srcs, void *stream)
{
    // takes no lock and touches no scratch of the context: it is what an or_bitmap callback calls from INSIDE
    // vdf_search_self_device_replay, which holds the context's lock
    if (!ctx || !ctx->subs.empty()) return VDF_E_INVAL;
    if (n_words == 0 || n_srcs == 0) return VDF_OK;
    if (!d_dst || !d_srcs) return VDF_E_INVAL;
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    VDF_HIP(ctx, vdf::launch_bitmap_or(d_dst, d_srcs, n_words, n_srcs, stream ? (hipStream_t)stream : ctx->stream));
    return VDF_OK;
}

int vdf_search_refs_device(vdf_ctx *ctx, const uint64_t *d_cand_hashes, const uint32_t *d_cand_durations,
                           size_t n_cand, const uint64_t *d_ref_hashes, const uint32_t *d_ref_durations, size_t n_ref,
                           uint32_t tol_int, uint32_t ref_index_base, vdf_hit *hits, uint64_t capacity,
                           uint64_t *n_hits, void *stream)
{
    if (!ctx || !n_hits || (capacity && !hits)) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    return search_refs_device_locked(ctx, d_cand_hashes, d_cand_durations, n_cand, d_ref_hashes, d_ref_durations,
                                     n_ref, tol_int, ref_index_base, hits, capacity, n_hits,
                                     stream ? (hipStream_t)stream : ctx->stream);
}

int vdf_sort_order_device(vdf_ctx *ctx, const uint32_t *d_durations, const uint32_t *d_path_rank, size_t n, uint32_t *d_perm_out,
                          void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    if (n == 0) return VDF_OK;
    if (!d_durations || !d_perm_out) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (n >= 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "more than 2^32-1 hashes");
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    VDF_HIP(ctx, ctx->sort_scratch_pub.reserve(vdf::sort_order_scratch_bytes((uint32_t)n, d_path_rank != nullptr)));
    VDF_HIP(ctx, vdf::launch_sort_order(d_durations, d_path_rank, (uint32_t)n, d_perm_out, ctx->sort_scratch_pub.p, ctx->sort_scratch_pub.cap,
                                        stream ? (hipStream_t)stream : ctx->stream));
    return VDF_OK;
}

int vdf_apply_order_device(vdf_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_durations, const uint32_t *d_perm, size_t n,
                           uint64_t *d_hashes_out, uint32_t *d_durations_out, void *stream)
{
    if (!ctx) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VDF_SINGLE_DEVICE_ONLY(ctx);
    if (n == 0) return VDF_OK;
    if (!d_hashes || !d_perm || !d_hashes_out || (d_durations_out && !d_durations)) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (n >= 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "more than 2^32-1 hashes");
    if (d_hashes == d_hashes_out || (d_durations && d_durations == d_durations_out)) return fail(ctx, VDF_E_INVAL, "the gather is not in place");
    VDF_HIP(ctx, hipSetDevice(ctx->device));
    VDF_HIP(ctx, vdf::launch_gather_hashes(d_hashes, d_durations, d_perm, (uint32_t)n, d_hashes_out, d_durations_out,
                                           stream ? (hipStream_t)stream : ctx->stream));
    return VDF_OK;
}

int vdf_search_self(vdf_ctx *ctx, const uint64_t *hashes, const uint32_t *durations, size_t n, uint32_t tol_int,
                    vdf_groups *out)
{
    if (!ctx || !out) return VDF_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    std::memset(out, 0, sizeof *out);
    ctx->stats = vdf_search_stats{};
    if (n == 0) return vdf_groups_finish_self(out);  // search_algorithm.rs:89-91
    if (!hashes || !durations) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (n >= 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "more than 2^32-1 hashes");
    // the windows are binary searches over the durations: the arrays must be in Search::sort order (search_algorithm.rs:55-61)
    if (!is_sorted_u32(durations, n)) return fail(ctx, VDF_E_INVAL, "durations are not ascending: pass the arrays in Search::sort order");
    // every device receives the whole database straight from the host arrays (no collective needed)
    int rc = for_each_device(ctx, [&](int, vdf_ctx *d) {
        VDF_HIP(d, hipSetDevice(d->device));
        int r = upload(d, d->up_hashes, hashes, n * VDF_HASH_WORDS * 8, d->stream);
        if (r == VDF_OK) r = upload(d, d->up_dur, durations, n * 4, d->stream);
        return r;
    });
    if (rc) return rc;
    return search_self_resident(ctx, n, tol_int, out);
}

int vdf_search_refs(vdf_ctx *ctx, const uint64_t *cand_hashes, const uint32_t *cand_durations, size_t n_cand,
                    const uint64_t *ref_hashes, const uint32_t *ref_durations, size_t n_ref, uint32_t tol_int,
                    vdf_groups *out)
{
    if (!ctx || !out) return VDF_E_INVAL;
    std::memset(out, 0, sizeof *out);
    if (n_cand == 0 || n_ref == 0) return vdf_groups_from_ref_hits(nullptr, 0, out);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!cand_hashes || !cand_durations || !ref_hashes || !ref_durations) return fail(ctx, VDF_E_INVAL, "null pointer");
    if (n_cand >= 0xFFFFFFFFull || n_ref >= 0xFFFFFFFFull) return fail(ctx, VDF_E_INVAL, "more than 2^32-1 hashes");
    if (!is_sorted_u32(cand_durations, n_cand))
        return fail(ctx, VDF_E_INVAL, "candidate durations are not ascending: pass the candidates in Search::sort order");
    const int G = device_count(ctx);
    std::vector<size_t> cnt((size_t)G), base((size_t)G);
    for (int k = 0; k < G; k++) {  // contiguous, order-preserving split of the references
        const size_t b = n_ref / (size_t)G, rem = n_ref % (size_t)G;
        base[(size_t)k] = (size_t)k * b + std::min<size_t>((size_t)k, rem);
        cnt[(size_t)k] = b + ((size_t)k < rem ? 1 : 0);
    }
    int rc = for_each_device(ctx, [&](int k, vdf_ctx *d) {
        VDF_HIP(d, hipSetDevice(d->device));
        int r = upload(d, d->up_hashes, cand_hashes, n_cand * VDF_HASH_WORDS * 8, d->stream);
        if (r == VDF_OK) r = upload(d, d->up_dur, cand_durations, n_cand * 4, d->stream);
        if (r == VDF_OK) r = upload(d, d->up_ref_hashes, ref_hashes + base[(size_t)k] * VDF_HASH_WORDS, cnt[(size_t)k] * VDF_HASH_WORDS * 8, d->stream);
        if (r == VDF_OK) r = upload(d, d->up_ref_dur, ref_durations + base[(size_t)k], cnt[(size_t)k] * 4, d->stream);
        return r;
    });
    if (rc) return rc;
    return search_refs_resident(ctx, n_cand, cnt, base, tol_int, out);
}

}  // extern "C"
