// Alignment of videos on their window hashes for gfx950 (MI355X), wave64: the longest shared stretch of every (video a, video b) pair
// (include/vdf.h: vdf_align_windows[_device]).  The answer is a reduction along the diagonals of each pair's distance
// matrix, so nothing here emits a hit list and the cost does not depend on how dense the matches are.
//
// align_bands_kernel<Unit, MASKED>: ONE band walk for every alignment call.  One wave per unit = band of 64 diagonals d0 ... d0 + 63 of one
// sub-matrix, four waves per workgroup.  The wave walks ka upward:
//   - the row of A is wave-uniform: scalar loads, the SGPR operand of v_xor_b32, v_bcnt_u32_b32 accumulates - the inner loop of the
//     VALU search backend (hamming.hip: hamming_tile_kernel), 64 VALU lane-ops per cell;
//   - lane kb mod 64 keeps row kb of B in 32 VGPRs; the 64 rows a step needs slide by one per step, so one lane reloads one row
//     (128 B, exec-masked) per step and every other lane keeps its row;
//   - the run state of a diagonal (length, dist_sum) moves one lane up per step: two wave rotates (ds_bpermute_b32), the only cross-lane traffic.
//     No LDS, no carry between waves: a diagonal never leaves its wave;
//   - a run ends at a non-matching cell or at the matrix edge; the lane that sees the end folds it into its own best.
// The lane-ownership rules are align_plan.h's (shared with the CPU replay in tests/cpp/align_plan_main.cpp).  What differs between the calls
// lies in front of the loop and is a Unit policy's:
//   - AlignPairUnits<false>: (pair, band) on the pair's own matrix - vdf_align_windows* and, MASKED (the cells of a pair's rectangles are
//     misses), the rounds r >= 1 of vdf_align_windows_stretches* (DESIGN.md 4.12);
//   - AlignPairUnits<true>: (pair, phase, band) on the strided rows of a phase's sub-matrix at the call's one rate - vdf_align_windows_retimed*
//     (align_retimed_plan.h);
//   - AlignTripleUnits: (triple, phase, band), the rate looked up per wave from the triple's slot - vdf_align_windows_rates* (DESIGN.md 4.23;
//     align_rates_plan.h) and, MASKED with rectangles in rows of the two videos so that they mask every phase, the rounds r >= 1 of
//     vdf_align_windows_rates_stretches* (align_rates_stretch_plan.h).
// Why the walk is a __global__ template with its text inside it, and not a device function that five kernels call: DESIGN.md 4.25.
// align_run_chunk: ONE chunk pipeline - the walk in launch cuts, the call's reduction (align_reduce_kernel: the bands of a pair -> one record;
// align_reduce_retimed_kernel / align_reduce_rates_kernel: bands -> phase-best -> record), align_scan_kernel and align_scatter_kernel<Record>: the
// items that have a record -> a dense list in the chunk's order (flag + scan).
// align_seed_kernel / align_seed_count_kernel / align_seed_scatter_kernel: which pairs of videos can have a record at all (vdf_align_seed_pairs*;
// DESIGN.md 4.13), so that the walk runs on those pairs only.
// align_class_layout_kernel / align_seed_variants_kernel / align_seed_variants_scatter_kernel: the same question against the mirrored, flipped and
// reversed variants of B, every requested variant from one pass over the seeds (vdf_align_seed_pairs_variants*; DESIGN.md 4.14;
// window_class_layout.h).
// align_seed_rates_kernel, at the very end: the seed pass of the retimed alignment, every phase of up to 8 rates on gathered rows of B
// (vdf_align_seed_pairs_rates*; align_seed_rates_plan.h).  It is align_seed_kernel's body, and a COPY of it on purpose: folded into
// one template the two instantiations with 14 check words did not keep the parent's seed loop.
#include "align_plan.h"
#include "align_rates_stretch_plan.h"
#include "align_retimed_plan.h"
#include "align_seed_rates_plan.h"
#include "vdf_internal.h"
#include "window_class_layout.h"

namespace vdf {

typedef const __attribute__((address_space(4))) uint32_t *align_u32_ptr;  // forces s_load for uniform addresses

// every lane takes the value of the lane below it, lane 0 that of lane 63 (align_plan.h: align_rotate_source).  The DPP form (one
// v_mov_b32_dpp wave_ror:1 instead of a ds_bpermute_b32) assembles for gfx950 but has not been run on the part: it stays off until
// tools/probe_wave_rotate.hip has confirmed it there.
constexpr bool kAlignRotateDpp = false;
__device__ __forceinline__ uint32_t align_rotate_up(uint32_t v, uint32_t lane)
{
    if (kAlignRotateDpp) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x13C, 0xF, 0xF, false);  // v_mov_b32_dpp wave_ror:1
    return (uint32_t)__shfl((int)v, (int)align_rotate_source(lane), 64);
}

__device__ __forceinline__ void align_load_row(uint32_t (&rw)[32], const uint32_t *__restrict__ rows, uint32_t kb)
{
    const uint4 *rp = reinterpret_cast<const uint4 *>(rows + (size_t)kb * 32);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const uint4 v = rp[q];
        rw[4 * q + 0] = v.x; rw[4 * q + 1] = v.y; rw[4 * q + 2] = v.z; rw[4 * q + 3] = v.w;
    }
}

// ---- the units of a walk: what a wave finds in front of the loop ---------------------------------------------------------------------------------
// What every walk's kernel reads.  n_items counts the chunk's pairs or triples (unit_offset has n_items + 1 entries); rects / n_rects are read by
// the masked instantiations only: item i has n_rects rectangles at rects[i * n_rects] (align_plan.h: AlignRect).
struct AlignBandsArgs {
    const uint32_t *a_hashes, *a_first;
    const uint8_t *a_skip;
    const uint32_t *b_hashes, *b_first;
    const uint8_t *b_skip;
    const uint32_t *unit_offset;
    uint32_t n_items, n_units, tol, min_run;
    AlignBandRecord *band_records;
    const AlignRect *rects;
    uint32_t n_rects;
};
// where a unit's walk runs: its item, the first rows of its videos, the sub-matrix (Na x Nb cells, cell (i, j) = row phase + num i of a, row den j
// of b) and its band.  Everything is wave-uniform and stays in SGPRs.
struct AlignUnitAt { uint32_t item, fa, fb, Na, Nb, phase, num, den, band; };

// Pair units.  RETIMED false: (pair, band) on the pair's whole matrix (vdf_align_windows*; masked: the rounds r >= 1 of
// vdf_align_windows_stretches*) - the identity mapping is a compile-time fact, so that no multiply is left in the walk.
// RETIMED true: (pair, phase, band) at the call's one rate num / den (vdf_align_windows_retimed*; align_retimed_plan.h).
template <bool RETIMED> struct AlignPairUnits {
    static constexpr bool kRetimed = RETIMED;
    struct Args : AlignBandsArgs {  // every instantiation carries num, den, rects and n_rects, read or not: the SGPR counts were matched on this layout
        const AlignPair *pairs;
        uint32_t num, den;  // read if RETIMED
    };
    static __device__ __forceinline__ AlignUnitAt locate(const Args &k, uint32_t unit)
    {
        const uint32_t p = align_unit_pair((align_u32_ptr)(uintptr_t)k.unit_offset, k.n_items, unit);
        const uint32_t u = unit - ((align_u32_ptr)(uintptr_t)k.unit_offset)[p];
        const uint32_t va = ((align_u32_ptr)(uintptr_t)k.pairs)[2 * p], vb = ((align_u32_ptr)(uintptr_t)k.pairs)[2 * p + 1];
        const uint32_t fa = ((align_u32_ptr)(uintptr_t)k.a_first)[va], Na_all = ((align_u32_ptr)(uintptr_t)k.a_first)[va + 1] - fa;
        const uint32_t fb = ((align_u32_ptr)(uintptr_t)k.b_first)[vb], Nb_all = ((align_u32_ptr)(uintptr_t)k.b_first)[vb + 1] - fb;
        if (!RETIMED) return AlignUnitAt{p, fa, fb, Na_all, Nb_all, 0u, 1u, 1u, u};
        uint32_t phase, band;
        align_retimed_unit(align_retimed_split(Na_all, Nb_all, k.num, k.den), u, &phase, &band);
        return AlignUnitAt{p, fa, fb, align_retimed_na(Na_all, k.num, phase), align_retimed_nb(Nb_all, k.den), phase, k.num, k.den, band};
    }
};

// Triple units: (triple, phase, band), the triple names its rate (vdf_align_windows_rates*; masked: the rounds r >= 1 of
// vdf_align_windows_rates_stretches*; align_rates_plan.h).  (a, b, rate) come by scalar loads from the chunk's triple array
// (vdf_video_pair_rate's layout), and num, den, the block's first row and its row of a_first come by one scalar load from the slot's 16 bytes of
// the table (AlignRatesSlot).  The table sits in the chunk's one upload, in front of the triples, not in the kernel arguments: indexed by a
// run-time slot, a by-value array can end up in scratch, and an s_load from memory cannot.  The slot is uniform per WAVE, not per workgroup - the
// four waves of a workgroup serve four units that may belong to four rates - so it and everything derived from it (num, den, phase, Na, Nb, d0,
// the row of A) stay in SGPRs: `unit` is built from readfirstlane(wave) and blockIdx, and every load on it is a scalar load.
struct AlignTripleUnits {
    static constexpr bool kRetimed = true;
    struct Args : AlignBandsArgs {
        const AlignRatesSlot *table;
        const AlignRatesTriple *triples;
    };
    static __device__ __forceinline__ AlignUnitAt locate(const Args &k, uint32_t unit)
    {
        const uint32_t t = align_unit_pair((align_u32_ptr)(uintptr_t)k.unit_offset, k.n_items, unit);
        align_u32_ptr tp = (align_u32_ptr)(uintptr_t)k.triples + (size_t)t * 3;
        const uint32_t va = tp[0], vb = tp[1];
        const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)tp[2]);  // < kAlignRatesMax: the host's planner wrote it
        align_u32_ptr sp = (align_u32_ptr)(uintptr_t)k.table + (size_t)slot * 4;
        const uint32_t num = sp[0], den = sp[1], row0 = sp[2];
        align_u32_ptr af = (align_u32_ptr)(uintptr_t)k.a_first + sp[3];      // the slot's row of a_first
        const uint32_t fa = row0 + af[va], Na_all = af[va + 1] - af[va];     // 32-bit sum: a row of the hashes the kernel sees (AlignRatesSlot)
        const uint32_t fb = ((align_u32_ptr)(uintptr_t)k.b_first)[vb], Nb_all = ((align_u32_ptr)(uintptr_t)k.b_first)[vb + 1] - fb;
        uint32_t phase, band;
        align_retimed_unit(align_retimed_split(Na_all, Nb_all, num, den), unit - ((align_u32_ptr)(uintptr_t)k.unit_offset)[t], &phase, &band);
        return AlignUnitAt{t, fa, fb, align_retimed_na(Na_all, num, phase), align_retimed_nb(Nb_all, den), phase, num, den, band};
    }
};

// the row of b behind row kb of the sub-matrix: den kb, or - the identity - kb itself in its own signed type, which the plain walk indexes with
__device__ __forceinline__ int32_t align_row_b(std::false_type, uint32_t, int32_t kb) { return kb; }
__device__ __forceinline__ uint32_t align_row_b(std::true_type, uint32_t den, int32_t kb) { return align_retimed_row_b(den, (uint32_t)kb); }

// ---- the band walk, once -----------------------------------------------------------------------------------------------------------------------
// The walk's text stays inside this __global__ template: moved into an inlined device function it compiles to a slower inner product (DESIGN.md
// 4.25).  ka, kb, d0, the lanes, the rotation and the reload are in sub-matrix coordinates; the rows behind a cell are ra = phase + num ka
// (wave-uniform: scalar loads) and rb = den kb, and the skip bytes are read at those same rows - A's with the aligned dword that holds it, which
// the stride lands on any of its four bytes.  The band record holds (offset = j - i, i0, n, sum) of the sub-matrix; the phases meet in the
// reduction.  MASKED: the cells of the item's rectangles are misses.  The rectangles are in ROWS OF THE TWO VIDEOS, so a stretch found in one
// phase masks its neighbourhood in every phase: a cell is masked iff one rectangle holds ra and rb.  They are wave-uniform: scalar loads into
// SGPRs in front of the walk (the slots behind n_rects are empty rectangles), the test on ra is scalar, and the test on rb - two compares per
// rectangle and lane - runs only in steps whose ra lies in a rectangle's rows of A.  A lane whose kb is outside the sub-matrix has row_ok false:
// what the test makes of its rb is not used.  The branch holds nothing else: the rotates and the reload run in every step.
template <class Unit, bool MASKED>
__global__ __launch_bounds__(256) void align_bands_kernel(typename Unit::Args k, uint32_t group_base)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t unit = (blockIdx.x + group_base) * kAlignWaves + wave;  // grids above 2^32 work-items are launched in cuts
    if (unit >= k.n_units) return;

    const AlignUnitAt at_unit = Unit::locate(k, unit);
    const uint32_t fa = at_unit.fa, fb = at_unit.fb, Na = at_unit.Na, Nb = at_unit.Nb, phase = at_unit.phase, num = at_unit.num, den = at_unit.den;
    const uint32_t tol = k.tol, min_run = k.min_run;
    const uint8_t *a_skip = k.a_skip;
    constexpr std::integral_constant<bool, Unit::kRetimed> retimed{};
    const int32_t d0 = align_band_d0(Na, at_unit.band);
    const uint32_t ka0 = align_ka_begin(d0), ka1 = align_ka_end(Na, Nb, d0);
    AlignRect rc[kAlignMaxStretches - 1];
    if (MASKED) {
        align_u32_ptr rp = (align_u32_ptr)(uintptr_t)k.rects + (size_t)at_unit.item * k.n_rects * 4;
#pragma unroll
        for (uint32_t i = 0; i < kAlignMaxStretches - 1; i++) {
            if (i < k.n_rects) rc[i] = AlignRect{rp[4 * i], rp[4 * i + 1], rp[4 * i + 2], rp[4 * i + 3]};
            else rc[i] = AlignRect{0u, 0u, 0u, 0u};
        }
    }

    const uint32_t *b_rows = k.b_hashes + (size_t)fb * 32;
    const uint8_t *b_sk = k.b_skip ? k.b_skip + fb : nullptr;
    align_u32_ptr a_rows = (align_u32_ptr)(uintptr_t)k.a_hashes + (size_t)fa * 32;

    // this lane's row of B; cells outside the sub-matrix are misses and no address is formed for them
    uint32_t rw[32];
    int32_t kb = align_lane_row(lane, ka0, d0);
    bool row_ok = kb >= 0 && kb < (int32_t)Nb;
    uint32_t row_skip = 0;  // the row's skip byte: compared where the row is used, so that the load is not waited for where it is issued
    if (row_ok) {
        const auto rb = align_row_b(retimed, den, kb);  // < Nb of the whole video
        if (b_sk) row_skip = b_sk[rb];
        align_load_row(rw, b_rows, (uint32_t)rb);
    } else {
#pragma unroll
        for (int q = 0; q < 32; q++) rw[q] = 0u;
    }

    uint32_t len = 0, sum = 0;                                              // the run of the diagonal this lane is on
    uint32_t best_score = 0, best_start = 0, best_n = 0, best_sum = 0;     // score 0 = none: every run scores at least 1
    int32_t best_off = 0;
    for (uint32_t ka = ka0; ka < ka1; ++ka) {
        const uint32_t ra = Unit::kRetimed ? align_retimed_row_a(phase, num, ka) : ka;  // < Na of the whole video, wave-uniform
        align_u32_ptr ap = a_rows + (size_t)ra * 32;
        uint32_t d = 0;
#pragma unroll
        for (int w = 0; w < 32; ++w) d += __builtin_popcount(rw[w] ^ ap[w]);  // ap[w]: SGPR
        bool a_ok = true;  // wave-uniform: the skip byte of A's row comes with the aligned dword that holds it, by a scalar load like the row
        if (a_skip) {
            const uintptr_t at = (uintptr_t)a_skip + fa + ra;
            a_ok = ((*(align_u32_ptr)(at & ~(uintptr_t)3) >> (8 * (uint32_t)(at & 3))) & 0xFFu) == 0u;
        }
        bool match = row_ok && row_skip == 0 && a_ok && d <= tol;
        if (MASKED) {
            bool in_a = false;  // wave-uniform: the rectangles and ra are
#pragma unroll
            for (uint32_t i = 0; i < kAlignMaxStretches - 1; i++) in_a = in_a || align_rect_has_a(rc[i], ra);
            if (in_a) match = match && !align_cell_masked(rc, kAlignMaxStretches - 1, ra, (uint32_t)align_row_b(retimed, den, kb));
        }
        if (match) { len += 1; sum += d; }
        const bool edge = ka + 1 == Na || kb + 1 == (int32_t)Nb;              // the diagonal's last cell
        const bool ends = len != 0 && (!match || edge);
        if (__builtin_amdgcn_ballot_w64(ends) != 0ull) {
            if (ends && len >= min_run) {
                const uint32_t score = len * (tol + 1) - sum;
                const uint32_t start = (match ? ka + 1 : ka) - len;
                const int32_t off = kb - (int32_t)ka;
                if (align_better(score, off, start, best_score, best_off, best_start)) {
                    best_score = score; best_off = off; best_start = start; best_n = len; best_sum = sum;
                }
            }
            if (ends) { len = 0; sum = 0; }
        }
        // the state follows its diagonal one lane up
        len = align_rotate_up(len, lane);
        sum = align_rotate_up(sum, lane);
        // the lane whose diagonal d0 is done takes the row of diagonal d0 + 63 of the next step
        if (ka + 1 < ka1 && lane == align_reload_lane(ka, d0)) {
            kb += (int32_t)kAlignBand;  // = align_reload_row(ka, d0) >= 1, from the lane's own register: the address stays a vector address
            row_ok = kb < (int32_t)Nb;
            row_skip = 0;
            if (row_ok) {
                const auto rb = align_row_b(retimed, den, kb);
                if (b_sk) row_skip = b_sk[rb];
                align_load_row(rw, b_rows, (uint32_t)rb);
            }
        }
    }

    // the wave's best of its 64 lane-bests; every run has its own (score, offset, start)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t o_score = (uint32_t)__shfl_xor((int)best_score, o, 64), o_start = (uint32_t)__shfl_xor((int)best_start, o, 64);
        const uint32_t o_n = (uint32_t)__shfl_xor((int)best_n, o, 64), o_sum = (uint32_t)__shfl_xor((int)best_sum, o, 64);
        const int32_t o_off = __shfl_xor(best_off, o, 64);
        if (align_better(o_score, o_off, o_start, best_score, best_off, best_start)) {
            best_score = o_score; best_off = o_off; best_start = o_start; best_n = o_n; best_sum = o_sum;
        }
    }
    if (lane == 0) k.band_records[unit] = AlignBandRecord{best_off, best_start, best_score ? best_n : 0u, best_sum};
}

__device__ __forceinline__ uint32_t align_block_rank(bool has, uint32_t *s_wave, uint32_t *block_total)
{  // rank of a thread among the threads of its 256-thread workgroup with `has`, in thread order
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(has);
    if (lane == 0) s_wave[wave] = (uint32_t)__builtin_popcountll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t k = 0; k < 4; k++) { if (k < wave) before += s_wave[k]; total += s_wave[k]; }
    *block_total = total;
    return before + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
}

// one thread per pair of the chunk: the best of its bands -> pair_records (n_windows = 0: none); block_count[g] = pairs with a record
__global__ __launch_bounds__(256) void align_reduce_kernel(const AlignPair *__restrict__ pairs, const uint32_t *__restrict__ unit_offset,
                                                           uint32_t n_pairs, uint32_t tol, const AlignBandRecord *__restrict__ band_records,
                                                           vdf_alignment *__restrict__ pair_records, uint32_t *__restrict__ block_count)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    bool has = false;
    if (p < n_pairs) {
        uint32_t best_score = 0, best_start = 0, best_n = 0, best_sum = 0;
        int32_t best_off = 0;
        const uint32_t u1 = unit_offset[p + 1];
        for (uint32_t u = unit_offset[p]; u < u1; ++u) {
            const AlignBandRecord r = band_records[u];
            if (r.n_windows == 0) continue;
            const uint32_t score = r.n_windows * (tol + 1) - r.dist_sum;
            if (align_better(score, r.offset, r.start_a, best_score, best_off, best_start)) {
                best_score = score; best_off = r.offset; best_start = r.start_a; best_n = r.n_windows; best_sum = r.dist_sum;
            }
        }
        has = best_score != 0;
        const AlignPair ab = pairs[p];
        pair_records[p] = vdf_alignment{ab.a, ab.b, best_off, best_start, has ? best_n : 0u, best_sum};
    }
    uint32_t total;
    (void)align_block_rank(has, s_wave, &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// exclusive scan of block_count[0 .. n) into block_offset, the sum to *total; one workgroup of 1024 threads
__global__ __launch_bounds__(1024) void align_scan_kernel(const uint32_t *__restrict__ block_count, uint32_t n, uint32_t *__restrict__ block_offset,
                                                          uint32_t *__restrict__ total)
{
    __shared__ uint32_t s_part[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n + 1023) / 1024;
    const uint32_t b = min(tid * per, n), e = min(b + per, n);
    uint32_t sum = 0;
    for (uint32_t i = b; i < e; i++) sum += block_count[i];
    s_part[tid] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan
        const uint32_t v = (tid >= o) ? s_part[tid - o] : 0u;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    uint32_t run = s_part[tid] - sum;
    for (uint32_t i = b; i < e; i++) { block_offset[i] = run; run += block_count[i]; }
    if (tid == 1023) *total = s_part[1023];
}

// the records with n_windows != 0, in their order; Record: vdf_alignment, vdf_alignment_retimed or vdf_alignment_rate
template <class Record>
__global__ __launch_bounds__(256) void align_scatter_kernel(const Record *__restrict__ pair_records, uint32_t n_pairs,
                                                            const uint32_t *__restrict__ block_offset, Record *__restrict__ out)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    Record r{};
    if (p < n_pairs) r = pair_records[p];
    const bool has = r.n_windows != 0;
    uint32_t total;
    const uint32_t rank = align_block_rank(has, s_wave, &total);
    if (has) out[(size_t)block_offset[blockIdx.x] + rank] = r;
}

size_t align_scratch_bytes(size_t n_pairs, size_t n_units)
{
    const size_t n_blocks = (n_pairs + 255) / 256;
    return n_units * sizeof(AlignBandRecord) + 2 * n_pairs * sizeof(vdf_alignment) + (2 * n_blocks + 4) * sizeof(uint32_t) + 64;
}

// One chunk of any alignment call: the band walk of k's units in launch cuts, the call's own reduction - reduce(band_records, item_records,
// block_count, n_blocks) launches it: one thread per item, block_count[g] = the items of workgroup g with a record - then the scan and the
// scatter.  k.band_records is set here.  Record is the call's record type; align_scratch_bytes / align_rates_scratch_bytes size the scratch.
template <class Unit, bool MASKED, class Record, class Reduce>
static hipError_t align_run_chunk(typename Unit::Args k, void *scratch, Record **dense_out, uint32_t **total_out, hipStream_t stream, Reduce reduce)
{
    // scratch: band records | item records | dense records | block counts | block offsets | total
    char *s = static_cast<char *>(scratch);
    k.band_records = reinterpret_cast<AlignBandRecord *>(s);
    s += (size_t)k.n_units * sizeof(AlignBandRecord);
    Record *item_records = reinterpret_cast<Record *>(s);
    s += (size_t)k.n_items * sizeof(Record);
    Record *dense = reinterpret_cast<Record *>(s);
    s += (size_t)k.n_items * sizeof(Record);
    const uint32_t n_blocks = (k.n_items + 255) / 256;
    uint32_t *block_count = reinterpret_cast<uint32_t *>(s), *block_offset = block_count + n_blocks, *total = block_offset + n_blocks;

    const size_t n_groups = ((size_t)k.n_units + kAlignWaves - 1) / kAlignWaves;
    for (const AlignLaunchCut &cut : align_launch_cuts(n_groups)) {
        hipLaunchKernelGGL((align_bands_kernel<Unit, MASKED>), dim3((uint32_t)cut.n), dim3(256), 0, stream, k, (uint32_t)cut.group_base);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    reduce(k.band_records, item_records, block_count, n_blocks);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(align_scan_kernel, dim3(1), dim3(1024), 0, stream, block_count, n_blocks, block_offset, total);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(align_scatter_kernel<Record>, dim3(n_blocks), dim3(256), 0, stream, item_records, k.n_items, block_offset, dense);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    *dense_out = dense;
    *total_out = total;
    return hipSuccess;
}

static AlignBandsArgs align_pair_args(const AlignLaunch &L)
{
    return AlignBandsArgs{L.a_hashes, L.a_first, L.a_skip, L.b_hashes, L.b_first, L.b_skip, L.unit_offset, L.n_pairs, L.n_units, L.tol, L.min_run,
                          nullptr, L.rects, L.n_rects};
}

hipError_t launch_align_chunk(const AlignLaunch &L, hipStream_t stream)
{
    if (L.n_pairs == 0 || L.n_units == 0 || L.n_rects >= kAlignMaxStretches || (L.n_rects && !L.rects)) return hipErrorInvalidValue;
    using Unit = AlignPairUnits<false>;
    const Unit::Args k{align_pair_args(L), L.pairs, 1u, 1u};
    const auto reduce = [&](const AlignBandRecord *band_records, vdf_alignment *pair_records, uint32_t *block_count, uint32_t n_blocks) {
        hipLaunchKernelGGL(align_reduce_kernel, dim3(n_blocks), dim3(256), 0, stream, L.pairs, L.unit_offset, L.n_pairs, L.tol, band_records, pair_records,
                           block_count);
    };
    if (L.n_rects) return align_run_chunk<Unit, true>(k, L.scratch, L.dense_out, L.total_out, stream, reduce);
    return align_run_chunk<Unit, false>(k, L.scratch, L.dense_out, L.total_out, stream, reduce);
}

// ---- retimed windows: every phase's sub-matrix of every pair in one launch (include/vdf.h: vdf_align_windows_retimed*) -----------
// one thread per pair of the chunk: its bands -> the best of every phase (align_better) -> the best of the phase-bests (align_retimed_plan.h:
// align_retimed_reduce, the text the plain C++ definition runs) -> pair_records (n_windows = 0: none); block_count[g] = pairs with a record
__global__ __launch_bounds__(256) void align_reduce_retimed_kernel(const AlignPair *__restrict__ pairs, const uint32_t *__restrict__ unit_offset,
                                                                   uint32_t n_pairs, const uint32_t *__restrict__ a_first,
                                                                   const uint32_t *__restrict__ b_first, uint32_t num, uint32_t den, uint32_t tol,
                                                                   const AlignBandRecord *__restrict__ band_records,
                                                                   vdf_alignment_retimed *__restrict__ pair_records, uint32_t *__restrict__ block_count)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    bool has = false;
    if (p < n_pairs) {
        const AlignPair ab = pairs[p];
        const AlignRetimedSplit sp = align_retimed_split(a_first[ab.a + 1] - a_first[ab.a], b_first[ab.b + 1] - b_first[ab.b], num, den);
        const AlignRetimedBest best = align_retimed_reduce(band_records + unit_offset[p], sp, den, tol);
        has = best.score != 0;
        pair_records[p] = vdf_alignment_retimed{ab.a, ab.b, best.first_a, best.first_b, has ? best.n_windows : 0u, best.dist_sum};
    }
    uint32_t total;
    (void)align_block_rank(has, s_wave, &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

hipError_t launch_align_retimed_chunk(const AlignLaunch &L, uint32_t num, uint32_t den, vdf_alignment_retimed **dense_out, hipStream_t stream)
{
    if (L.n_pairs == 0 || L.n_units == 0 || L.n_rects || num == 0 || den == 0 || num > kAlignRetimedMaxNum) return hipErrorInvalidValue;
    using Unit = AlignPairUnits<true>;
    const Unit::Args k{align_pair_args(L), L.pairs, num, den};
    return align_run_chunk<Unit, false>(
        k, L.scratch, dense_out, L.total_out, stream,
        [&](const AlignBandRecord *band_records, vdf_alignment_retimed *pair_records, uint32_t *block_count, uint32_t n_blocks) {
            hipLaunchKernelGGL(align_reduce_retimed_kernel, dim3(n_blocks), dim3(256), 0, stream, L.pairs, L.unit_offset, L.n_pairs, L.a_first, L.b_first, num,
                               den, L.tol, band_records, pair_records, block_count);
        });
}

// ---- retimed windows at up to 8 rates: the triples of every rate in one launch (include/vdf.h: vdf_align_windows_rates*), and
// the masked rounds of vdf_align_windows_rates_stretches* (align_rates_stretch_plan.h) ------------------------------------------
static_assert(sizeof(vdf_alignment_rate) == 32 && sizeof(AlignRatesTriple) == sizeof(vdf_video_pair_rate) &&
                  offsetof(AlignRatesTriple, a) == offsetof(vdf_video_pair_rate, a) && offsetof(AlignRatesTriple, b) == offsetof(vdf_video_pair_rate, b) &&
                  offsetof(AlignRatesTriple, rate) == offsetof(vdf_video_pair_rate, rate) && sizeof(AlignRatesSlot) == 16 && kAlignRatesMax == VDF_WINDOWS_MAX_RATES,
              "the chunk's triples are vdf_video_pair_rate, its records vdf_alignment_rate");

// one thread per triple of the chunk: its bands -> align_retimed_reduce with the triple's own split and den (the text the plain C++ definition and
// align_reduce_retimed_kernel run) -> triple_records with n_frames_b (n_windows = 0: none); block_count[g] = triples with a record
__global__ __launch_bounds__(256) void align_reduce_rates_kernel(const AlignRatesSlot *__restrict__ table, const AlignRatesTriple *__restrict__ triples,
                                                                 const uint32_t *__restrict__ unit_offset, uint32_t n_triples,
                                                                 const uint32_t *__restrict__ a_first, const uint32_t *__restrict__ b_first, uint32_t tol,
                                                                 const AlignBandRecord *__restrict__ band_records,
                                                                 vdf_alignment_rate *__restrict__ triple_records, uint32_t *__restrict__ block_count)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    bool has = false;
    if (p < n_triples) {
        const AlignRatesTriple t = triples[p];
        const AlignRatesSlot sl = table[t.rate];
        const uint32_t *af = a_first + sl.first_at;
        const AlignRetimedSplit sp = align_retimed_split(af[t.a + 1] - af[t.a], b_first[t.b + 1] - b_first[t.b], sl.num, sl.den);
        const AlignRetimedBest best = align_retimed_reduce(band_records + unit_offset[p], sp, sl.den, tol);
        has = best.score != 0;
        triple_records[p] = vdf_alignment_rate{t.a, t.b, t.rate, best.first_a, best.first_b, has ? best.n_windows : 0u, best.dist_sum,
                                               has ? (best.n_windows - 1) * sl.den + 16u : 0u};
    }
    uint32_t total;
    (void)align_block_rank(has, s_wave, &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// a chunk over triples: L.plan is the chunk's one upload (table | triples | unit_offset, and | rects behind them in a masked round)
template <bool MASKED> static hipError_t align_run_rates_chunk(const AlignRatesLaunch &L, uint32_t n_rects, hipStream_t stream)
{
    const char *plan = static_cast<const char *>(L.plan);
    const AlignRatesSlot *table = reinterpret_cast<const AlignRatesSlot *>(plan);
    const AlignRatesTriple *triples = reinterpret_cast<const AlignRatesTriple *>(plan + align_rates_plan_triples_at());
    const uint32_t *unit_offset = reinterpret_cast<const uint32_t *>(plan + align_rates_plan_offsets_at(L.n_triples));
    const AlignRect *rects = MASKED ? reinterpret_cast<const AlignRect *>(plan + align_rates_plan_rects_at(L.n_triples)) : nullptr;
    const AlignTripleUnits::Args k{AlignBandsArgs{L.a_hashes, L.a_first, L.a_skip, L.b_hashes, L.b_first, L.b_skip, unit_offset, L.n_triples, L.n_units, L.tol,
                                                  L.min_run, nullptr, rects, n_rects},
                                   table, triples};
    return align_run_chunk<AlignTripleUnits, MASKED>(
        k, L.scratch, L.dense_out, L.total_out, stream,
        [&](const AlignBandRecord *band_records, vdf_alignment_rate *triple_records, uint32_t *block_count, uint32_t n_blocks) {
            hipLaunchKernelGGL(align_reduce_rates_kernel, dim3(n_blocks), dim3(256), 0, stream, table, triples, unit_offset, L.n_triples, L.a_first, L.b_first,
                               L.tol, band_records, triple_records, block_count);
        });
}

hipError_t launch_align_rates_chunk(const AlignRatesLaunch &L, hipStream_t stream)
{
    if (L.n_triples == 0 || L.n_units == 0 || !L.plan) return hipErrorInvalidValue;
    return align_run_rates_chunk<false>(L, 0, stream);
}

// launch_align_rates_chunk with the masked walk: L.plan is the round's upload (align_rates_round_plan_bytes), n_rects in 1 ... kAlignMaxStretches
// - 1.  The reduction, the scan and the scatter are the plain chunk's: the rank of a round's records is the round's number, which the host adds.
hipError_t launch_align_rates_masked_chunk(const AlignRatesLaunch &L, uint32_t n_rects, hipStream_t stream)
{
    if (L.n_triples == 0 || L.n_units == 0 || !L.plan || n_rects == 0 || n_rects >= kAlignMaxStretches) return hipErrorInvalidValue;
    return align_run_rates_chunk<true>(L, n_rects, stream);
}

// ---- seeding: the pairs of videos that have a matching (seed, row) cell (include/vdf.h: vdf_align_seed_pairs*) -------------------
// align_seed_kernel: one workgroup per unit (chunk of seeds, tile of rows of B; align_plan.h: AlignSeedPlan), modelled on the VALU search
// backend (hamming.hip: hamming_tile_kernel).  The tile's rows sit in VGPRs, R per lane, each with its video index and its skip byte; the
// chunk's seeds stream through SGPRs (scalar loads: the seed's row of A, its video, its skip byte).  After CHKW dwords a seed that every row of
// the wave is already more than tol away from is left: partial distances only grow, so the exit is exact.  A hit - behind a wave-uniform ballot
// - sets bit seed_video * n_b + row_video of the bitmap: the word is read first and the atomic is issued only if the bit is still clear, so
// dense matches cost reads that hit in L2, no atomics and no list.  Rows at or behind n_rows are never addressed: their lanes hold zero rows
// with the skip byte set, which cannot hit.
typedef const __attribute__((address_space(4))) unsigned long long *align_u64_ptr;

template <int R, int CHKW>
__global__ __launch_bounds__(256) void align_seed_kernel(
    const uint32_t *__restrict__ a_hashes, const uint8_t *__restrict__ a_skip, const uint32_t *__restrict__ seed_window,
    const uint32_t *__restrict__ seed_video, uint32_t n_seeds, uint32_t chunk_seeds, const uint32_t *__restrict__ b_hashes,
    const uint8_t *__restrict__ b_skip, const uint32_t *__restrict__ row_video, uint32_t row_base, uint32_t n_rows,
    const unsigned long long *__restrict__ unit_offset, const uint32_t *__restrict__ tile_first, uint32_t n_chunks, uint32_t tol, int self_mode,
    uint32_t n_b, uint32_t *__restrict__ bitmap, unsigned long long unit_base)
{
    constexpr uint32_t TILE_ROWS = 256 * R;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long unit = unit_base + blockIdx.x;  // grids above 2^32 work-items are launched in cuts
    const uint32_t chunk = align_seed_unit_chunk((align_u64_ptr)(uintptr_t)unit_offset, n_chunks, unit);
    const uint32_t tile = ((align_u32_ptr)(uintptr_t)tile_first)[chunk] + (uint32_t)(unit - ((align_u64_ptr)(uintptr_t)unit_offset)[chunk]);
    const uint64_t wave_row0 = (uint64_t)tile * TILE_ROWS + wave * (64 * R);
    if (wave_row0 >= n_rows) return;  // wave-uniform: a wave of padding rows only (no barrier below)
    const uint32_t s0 = chunk * chunk_seeds, s1 = min(s0 + chunk_seeds, n_seeds);

    // rows -> VGPRs
    uint32_t rw[R][32];
    uint32_t rvid[R], rskip[R];
#pragma unroll
    for (int k = 0; k < R; k++) {
        const uint64_t r = wave_row0 + k * 64 + lane;
        if (r < n_rows) {
            const size_t w = (size_t)row_base + (size_t)r;
            align_load_row(rw[k], b_hashes, (uint32_t)w);  // row_base + r <= first_b[n_b]: 32 bits
            rvid[k] = row_video[r];
            rskip[k] = b_skip ? b_skip[w] : 0u;
        } else {
#pragma unroll
            for (int q = 0; q < 32; q++) rw[k][q] = 0u;
            rvid[k] = 0u;
            rskip[k] = 1u;
        }
    }

    align_u32_ptr a_rows = (align_u32_ptr)(uintptr_t)a_hashes;
    for (uint32_t s = s0; s < s1; ++s) {
        const uint32_t sw = ((align_u32_ptr)(uintptr_t)seed_window)[s];
        align_u32_ptr ap = a_rows + (size_t)sw * 32;
        uint32_t d[R];
#pragma unroll
        for (int k = 0; k < R; k++) d[k] = 0u;
#pragma unroll
        for (int w = 0; w < (CHKW < 32 ? CHKW : 32); ++w) {
            const uint32_t aw = ap[w];  // SGPR
#pragma unroll
            for (int k = 0; k < R; k++) d[k] += __builtin_popcount(rw[k][w] ^ aw);
        }
        uint32_t m = d[0];
#pragma unroll
        for (int k = 1; k < R; k++) m = min(m, d[k]);
        if (CHKW < 32) {
            if (__builtin_amdgcn_ballot_w64(m <= tol) == 0ull) continue;  // partial distances only grow
#pragma unroll
            for (int w = CHKW; w < 32; ++w) {
                const uint32_t aw = ap[w];
#pragma unroll
                for (int k = 0; k < R; k++) d[k] += __builtin_popcount(rw[k][w] ^ aw);
            }
            m = d[0];
#pragma unroll
            for (int k = 1; k < R; k++) m = min(m, d[k]);
        }
        if (__builtin_amdgcn_ballot_w64(m <= tol) != 0ull) {
            // rare path: the seed's skip byte (with the aligned dword that holds it, by a scalar load like the row), the triangle, the bitmap
            bool a_ok = true;
            if (a_skip) {
                const uintptr_t at = (uintptr_t)a_skip + sw;
                a_ok = ((*(align_u32_ptr)(at & ~(uintptr_t)3) >> (8 * (uint32_t)(at & 3))) & 0xFFu) == 0u;
            }
            if (a_ok) {
                const uint32_t sv = ((align_u32_ptr)(uintptr_t)seed_video)[s];
#pragma unroll
                for (int k = 0; k < R; k++) {
                    if (d[k] <= tol && rskip[k] == 0u && (!self_mode || sv < rvid[k])) {
                        const uint64_t bit = (uint64_t)sv * n_b + rvid[k];
                        uint32_t *word = bitmap + (size_t)(bit >> 5);
                        const uint32_t mask = 1u << (uint32_t)(bit & 31);
                        if ((__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & mask) == 0u) atomicOr(word, mask);
                    }
                }
            }
        }
    }
}

// the sum of v over the threads in front of this one in its 256-thread workgroup, and the workgroup's sum
__device__ __forceinline__ uint32_t align_block_prefix(uint32_t v, uint32_t *s_wave, uint32_t *block_total)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, o, 64);
        if (lane >= (uint32_t)o) inc += up;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t k = 0; k < 4; k++) { if (k < wave) before += s_wave[k]; total += s_wave[k]; }
    *block_total = total;
    return before + inc - v;
}

// align_seed_compact: bitmap -> the dense list of its set bits in bit order = (a, b) order.  Count (one thread per word, block_count[g] = bits
// of workgroup g's 256 words), the scan of the align reductions (align_scan_kernel, launched as it is), scatter.
__global__ __launch_bounds__(256) void align_seed_count_kernel(const uint32_t *__restrict__ bitmap, uint32_t n_words, uint32_t *__restrict__ block_count)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t n = i < n_words ? (uint32_t)__builtin_popcount(bitmap[i]) : 0u;
    uint32_t total;
    (void)align_block_prefix(n, s_wave, &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// the first `limit` pairs of the list are written (the caller's capacity: the list of a dense bitmap is 2^24 x 8 bytes)
__global__ __launch_bounds__(256) void align_seed_scatter_kernel(const uint32_t *__restrict__ bitmap, uint32_t n_words, uint32_t n_b,
                                                                 const uint32_t *__restrict__ block_offset, vdf_video_pair *__restrict__ out,
                                                                 uint32_t limit)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t bits = i < n_words ? bitmap[i] : 0u;
    uint32_t total;
    uint32_t at = block_offset[blockIdx.x] + align_block_prefix((uint32_t)__builtin_popcount(bits), s_wave, &total);
    while (bits != 0u && at < limit) {
        const uint64_t bit = (uint64_t)i * 32 + (uint32_t)__builtin_ctz(bits);
        bits &= bits - 1;
        out[at++] = vdf_video_pair{(uint32_t)(bit / n_b), (uint32_t)(bit % n_b)};
    }
}

size_t align_seed_scratch_bytes(size_t n_words) { return (2 * ((n_words + 255) / 256) + 4) * sizeof(uint32_t) + 64; }

hipError_t launch_align_seed(const AlignSeedLaunch &L, hipStream_t stream)
{
    if (L.n_units == 0 || L.n_words == 0 || L.n_words > (1u << 21)) return hipErrorInvalidValue;  // 2^24 pairs a < b: 5793^2 bits, just above 2^25
    for (const AlignLaunchCut &cut : align_launch_cuts((size_t)L.n_units)) {
#define VDF_SEED_LAUNCH(CW)                                                                                                                         \
    hipLaunchKernelGGL((align_seed_kernel<(int)kSeedRowsPerLane, CW>), dim3((uint32_t)cut.n), dim3(256), 0, stream, L.a_hashes, L.a_skip,            \
                       L.seed_window, L.seed_video, L.n_seeds, kSeedChunk, L.b_hashes, L.b_skip, L.row_video, L.row_base, L.n_rows, L.unit_offset, \
                       L.tile_first, L.n_chunks, L.tol, L.self_mode, L.n_b, L.bitmap, (unsigned long long)cut.group_base)
        switch (align_seed_check_words(L.tol)) {
        case 14: VDF_SEED_LAUNCH(14); break;
        case 22: VDF_SEED_LAUNCH(22); break;
        case 26: VDF_SEED_LAUNCH(26); break;
        default: VDF_SEED_LAUNCH(32); break;
        }
#undef VDF_SEED_LAUNCH
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    // scratch: block counts | block offsets | total
    const uint32_t n_blocks = (L.n_words + 255) / 256;
    uint32_t *block_count = static_cast<uint32_t *>(L.scratch), *block_offset = block_count + n_blocks, *total = block_offset + n_blocks;
    hipLaunchKernelGGL(align_seed_count_kernel, dim3(n_blocks), dim3(256), 0, stream, L.bitmap, L.n_words, block_count);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(align_scan_kernel, dim3(1), dim3(1024), 0, stream, block_count, n_blocks, block_offset, total);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    *L.total_out = total;
    return hipSuccess;
}

hipError_t launch_align_seed_scatter(const AlignSeedLaunch &L, vdf_video_pair *out, uint32_t limit, hipStream_t stream)
{
    const uint32_t n_blocks = (L.n_words + 255) / 256;
    const uint32_t *block_offset = static_cast<const uint32_t *>(L.scratch) + n_blocks;
    hipLaunchKernelGGL(align_seed_scatter_kernel, dim3(n_blocks), dim3(256), 0, stream, L.bitmap, L.n_words, L.n_b, block_offset, out, limit);
    return hipGetLastError();
}

// ---- seeding against the variants: every requested variant from one pass over the seeds (include/vdf.h: vdf_align_seed_pairs_variants*;
// DESIGN.md 4.14) --------------------------------------------------------------------------------------------------------------------------
// align_class_layout_kernel: the seeds of A, or the rows of B with their zero planes, into the class-major rows of window_class_layout.h.
// One thread per output dword, plain vector loads and stores; where a bit comes from is read from the header's table (4.2 KB, L1 / L2
// resident), and the live counts are popcounts of ~Z under the class masks.  zero == null: seeds (row r = window seed_window[r] of `hashes`, 36 dwords);
// otherwise rows of B (row r = window row_base + r, 72 dwords).
__device__ const ClassTables kClassTablesDevice = make_class_tables();  // window_class_layout.h: the permutation and the class masks as tables

__global__ __launch_bounds__(256) void align_class_layout_kernel(const uint32_t *__restrict__ hashes, const uint32_t *__restrict__ zero,
                                                                 const uint8_t *__restrict__ skip, const uint32_t *__restrict__ seed_window,
                                                                 const uint32_t *__restrict__ seed_video, uint32_t row_base, uint32_t n,
                                                                 uint32_t *__restrict__ out, unsigned long long block_base)
{
    const uint32_t stride = zero ? kClassRowStride : kClassSeedStride;
    const uint64_t i = (block_base + blockIdx.x) * 256 + threadIdx.x;
    if (i >= (uint64_t)n * stride) return;
    const uint32_t r = (uint32_t)(i / stride), q = (uint32_t)(i % stride);
    if (zero) {
        const size_t w = (size_t)row_base + r;
        out[i] = window_class_row_dword(hashes + w * 32, zero + w * 32, skip ? skip[w] : 0u, q, &kClassTablesDevice);
    } else {
        const size_t w = seed_window[r];
        out[i] = window_class_seed_dword(hashes + w * 32, skip ? skip[w] : 0u, seed_video[r], q, &kClassTablesDevice);
    }
}

// align_seed_variants_kernel: align_seed_kernel's units and streams (one workgroup per (chunk of seeds, tile of 256 rows of B); the rows in
// VGPRs, one per lane: Hz, nZ, the seven live counts, video, skip byte; the seeds through SGPRs by scalar loads) on the class-major rows.  Per
// dword t = a & nZ, u = t ^ Hz, popcount(t) into one subtrahend and popcount(u) into the accumulator of the dword's class; from the eight
// sums the distance to EVERY variant of the row follows (window_class_layout.h).  Behind the 33 dwords a lower bound of min_v d_v over the
// REQUESTED variants - popcount(A) - sub + acc_0 + per class acc_c, live_c - acc_c or the smaller of the two, as the requested variants keep
// it, flip it or differ on it - is compared with tol under a wave-uniform ballot (exact: no requested d_v lies below it; with one variant
// requested it is that d_v); only behind it are the distances to the requested variants formed, and a hit under variant v sets bit
// (slot(v) n_a + seed_video) n_b + row_video, read first, atomicOr only if clear.  Rows at or behind n_rows are never addressed: their
// lanes hold zero rows with the skip byte set.
__global__ __launch_bounds__(256) void align_seed_variants_kernel(
    const uint32_t *__restrict__ seeds, uint32_t n_seeds, uint32_t chunk_seeds, const uint32_t *__restrict__ rows,
    const uint32_t *__restrict__ row_video, uint32_t n_rows, const unsigned long long *__restrict__ unit_offset,
    const uint32_t *__restrict__ tile_first, uint32_t n_chunks, uint32_t tol, int self_mode, uint32_t variant_mask, uint32_t n_a, uint32_t n_b,
    uint32_t *__restrict__ bitmap, unsigned long long unit_base)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long unit = unit_base + blockIdx.x;
    const uint32_t chunk = align_seed_unit_chunk((align_u64_ptr)(uintptr_t)unit_offset, n_chunks, unit);
    const uint32_t tile = ((align_u32_ptr)(uintptr_t)tile_first)[chunk] + (uint32_t)(unit - ((align_u64_ptr)(uintptr_t)unit_offset)[chunk]);
    const uint64_t wave_row0 = (uint64_t)tile * kSeedVariantsTileRows + wave * 64;
    if (wave_row0 >= n_rows) return;  // wave-uniform: a wave of padding rows only (no barrier below)
    const uint32_t s0 = chunk * chunk_seeds, s1 = min(s0 + chunk_seeds, n_seeds);

    // this lane's row -> VGPRs
    uint32_t hz[kClassDwords], nz[kClassDwords], live[8], rvid = 0u, rskip = 1u;
    const uint64_t r = wave_row0 + lane;
    if (r < n_rows) {
        const uint4 *rp = reinterpret_cast<const uint4 *>(rows + (size_t)r * kClassRowStride);
        uint32_t lo[36], hi[36];
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const uint4 x = rp[k], y = rp[9 + k];
            lo[4 * k] = x.x; lo[4 * k + 1] = x.y; lo[4 * k + 2] = x.z; lo[4 * k + 3] = x.w;
            hi[4 * k] = y.x; hi[4 * k + 1] = y.y; hi[4 * k + 2] = y.z; hi[4 * k + 3] = y.w;
        }
#pragma unroll
        for (int q = 0; q < (int)kClassDwords; q++) { hz[q] = lo[q]; nz[q] = hi[q]; }
#pragma unroll
        for (int c = 1; c < 8; c++) live[c] = lo[33 + ((c - 1) >> 2)] >> (8 * ((c - 1) & 3)) & 0xFFu;
        rskip = lo[35];
        rvid = row_video[r];
    } else {
#pragma unroll
        for (int q = 0; q < (int)kClassDwords; q++) { hz[q] = 0u; nz[q] = 0u; }
#pragma unroll
        for (int c = 1; c < 8; c++) live[c] = 0u;
    }
    live[0] = 0u;

    // which classes some requested variant flips, and which some requested variant keeps (bit c; wave-uniform)
    uint32_t flip_any = 0u, keep_any = 0u;
#pragma unroll
    for (uint32_t v = 1; v < 8; v++) {
        if (!(variant_mask >> v & 1u)) continue;
#pragma unroll
        for (uint32_t c = 1; c < 8; c++) {
            if (window_class_flipped(v, c)) flip_any |= 1u << c;
            else keep_any |= 1u << c;
        }
    }

    align_u32_ptr seed_rows = (align_u32_ptr)(uintptr_t)seeds;
    for (uint32_t s = s0; s < s1; ++s) {
        align_u32_ptr ap = seed_rows + (size_t)s * kClassSeedStride;
        uint32_t sub = 0u, acc[8];
#pragma unroll
        for (int c = 0; c < 8; c++) acc[c] = 0u;
#pragma unroll
        for (int q = 0; q < (int)kClassDwords; q++) {
            const uint32_t t = ap[q] & nz[q];  // ap[q]: SGPR
            sub += __builtin_popcount(t);
            acc[window_class_of_dword(q)] += __builtin_popcount(t ^ hz[q]);
        }
        const uint32_t base = ap[33] - sub + acc[0];  // the never-flipped part: popcount(A & Z) + the distance inside group 0
        // a lower bound of min over the REQUESTED variants of d_v: a class that every requested variant flips counts flipped, one that none flips
        // counts as it is, one on which they differ counts the smaller of the two (flip_any / keep_any: wave-uniform).  With one variant requested
        // the bound is that variant's distance itself; with several, a row close to a mix of them that no single variant reaches still passes
        // the ballot and is turned away by the exact distances below.
        uint32_t bound = base;
#pragma unroll
        for (int c = 1; c < 8; c++) {
            const uint32_t kept = acc[c], flipped = live[c] - acc[c];
            bound += (flip_any >> c & 1u) ? ((keep_any >> c & 1u) ? min(kept, flipped) : flipped) : kept;
        }
        if (__builtin_amdgcn_ballot_w64(bound <= tol) == 0ull) continue;
        // rare path: the seed's skip byte and video, the triangle, the distances to the requested variants, the bitmap
        if (ap[34] != 0u) continue;  // (uniform)
        const uint32_t sv = ap[35];
        if (rskip == 0u && (!self_mode || sv < rvid)) {
#pragma unroll
            for (uint32_t v = 1; v < 8; v++) {
                if (!(variant_mask >> v & 1u)) continue;  // (uniform)
                uint32_t d = base;
#pragma unroll
                for (uint32_t c = 1; c < 8; c++) d += window_class_flipped(v, c) ? live[c] - acc[c] : acc[c];
                if (d <= tol) {
                    const uint32_t slot = (uint32_t)__builtin_popcount(variant_mask & ((1u << v) - 1u));
                    const uint64_t bit = ((uint64_t)slot * n_a + sv) * n_b + rvid;
                    uint32_t *word = bitmap + (size_t)(bit >> 5);
                    const uint32_t mask = 1u << (uint32_t)(bit & 31);
                    if ((__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & mask) == 0u) atomicOr(word, mask);
                }
            }
        }
    }
}

// bit order of the concatenated bitmap = (slot, a, b) order = (variant, a, b) order; slots: 4 bits per slot, the slot's variant
__global__ __launch_bounds__(256) void align_seed_variants_scatter_kernel(const uint32_t *__restrict__ bitmap, uint32_t n_words, uint32_t n_a,
                                                                          uint32_t n_b, uint32_t slots,
                                                                          const uint32_t *__restrict__ block_offset,
                                                                          vdf_video_pair_variant *__restrict__ out, uint32_t limit)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t bits = i < n_words ? bitmap[i] : 0u;
    uint32_t total;
    uint32_t at = block_offset[blockIdx.x] + align_block_prefix((uint32_t)__builtin_popcount(bits), s_wave, &total);
    while (bits != 0u && at < limit) {
        const uint64_t bit = (uint64_t)i * 32 + (uint32_t)__builtin_ctz(bits);
        bits &= bits - 1;
        const uint64_t sa = bit / n_b;
        out[at++] = vdf_video_pair_variant{(uint32_t)(sa % n_a), (uint32_t)(bit % n_b), slots >> (4 * (uint32_t)(sa / n_a)) & 15u};
    }
}

hipError_t launch_align_class_layout(const uint32_t *hashes, const uint32_t *zero, const uint8_t *skip, const uint32_t *seed_window,
                                     const uint32_t *seed_video, uint32_t row_base, uint32_t n, uint32_t *out, hipStream_t stream)
{
    const size_t n_blocks = ((size_t)n * (zero ? kClassRowStride : kClassSeedStride) + 255) / 256;
    for (const AlignLaunchCut &cut : align_launch_cuts(n_blocks)) {
        hipLaunchKernelGGL(align_class_layout_kernel, dim3((uint32_t)cut.n), dim3(256), 0, stream, hashes, zero, skip, seed_window, seed_video, row_base, n,
                           out, (unsigned long long)cut.group_base);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_align_seed_variants(const AlignSeedVariantsLaunch &L, hipStream_t stream)
{
    const uint32_t n_slots = (uint32_t)__builtin_popcount(L.variant_mask);
    if (L.n_units == 0 || n_slots == 0 || (L.variant_mask & ~0xFEu) || L.n_words == 0 || L.n_words > 7 * (1u << 21)) return hipErrorInvalidValue;
    for (const AlignLaunchCut &cut : align_launch_cuts((size_t)L.n_units)) {
        hipLaunchKernelGGL(align_seed_variants_kernel, dim3((uint32_t)cut.n), dim3(256), 0, stream, L.seeds, L.n_seeds, kSeedChunk, L.rows, L.row_video,
                           L.n_rows, L.unit_offset, L.tile_first, L.n_chunks, L.tol, L.self_mode, L.variant_mask, L.n_a, L.n_b, L.bitmap,
                           (unsigned long long)cut.group_base);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    const uint32_t n_blocks = (L.n_words + 255) / 256;
    uint32_t *block_count = static_cast<uint32_t *>(L.scratch), *block_offset = block_count + n_blocks, *total = block_offset + n_blocks;
    hipLaunchKernelGGL(align_seed_count_kernel, dim3(n_blocks), dim3(256), 0, stream, L.bitmap, L.n_words, block_count);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(align_scan_kernel, dim3(1), dim3(1024), 0, stream, block_count, n_blocks, block_offset, total);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    *L.total_out = total;
    return hipSuccess;
}

hipError_t launch_align_seed_variants_scatter(const AlignSeedVariantsLaunch &L, vdf_video_pair_variant *out, uint32_t limit, hipStream_t stream)
{
    const uint32_t n_blocks = (L.n_words + 255) / 256;
    const uint32_t *block_offset = static_cast<const uint32_t *>(L.scratch) + n_blocks;
    uint32_t slots = 0, slot = 0;
    for (uint32_t v = 1; v < 8; v++)
        if (L.variant_mask >> v & 1u) slots |= v << (4 * slot++);
    hipLaunchKernelGGL(align_seed_variants_scatter_kernel, dim3(n_blocks), dim3(256), 0, stream, L.bitmap, L.n_words, L.n_a, L.n_b, slots, block_offset, out,
                       limit);
    return hipGetLastError();
}

// ---- seeding the retimed alignment: every phase of up to 8 rates from one pass (include/vdf.h: vdf_align_seed_pairs_rates*; DESIGN.md 4.22;
// align_seed_rates_plan.h) ------------------------------------------------------------------------------------------------------------------
// align_seed_rates_kernel: align_seed_kernel's body on the plan of align_seed_rates_plan.h.  One workgroup per unit (chunk of seeds, tile of its
// class's rows).  The tile's rows are GATHERED: lane row r of the plan is window row_window[r] of b_hashes (the rows den j of B's videos), its
// skip byte is read at that same window, and a sentinel - the padding of a class's last tile - becomes a zero row with the skip byte set, as
// the lanes behind n_rows are in the plain kernel; a wave whose first row is a sentinel holds padding only (the sentinels are a suffix of
// the tile) and leaves.  The seeds stream through SGPRs as there; a seed's slot (its rate's index in the job's list) arrives with it by a scalar
// load and goes into the bit index (slot n_a + seed_video) n_b + row_video.  exclude_same is tested on the rare path.  The early exit, the
// seed's skip byte through its aligned dword and the read-before-atomic are the plain kernel's.  No LDS, vector stores only (the atomics).
template <int R, int CHKW>
__global__ __launch_bounds__(256) void align_seed_rates_kernel(
    const uint32_t *__restrict__ a_hashes, const uint8_t *__restrict__ a_skip, const uint32_t *__restrict__ seed_window,
    const uint32_t *__restrict__ seed_video, const uint32_t *__restrict__ seed_slot, const uint32_t *__restrict__ chunk_first,
    const uint32_t *__restrict__ b_hashes, const uint8_t *__restrict__ b_skip, const uint32_t *__restrict__ row_window,
    const uint32_t *__restrict__ row_video, const unsigned long long *__restrict__ unit_offset, const uint32_t *__restrict__ tile_first,
    uint32_t n_chunks, uint32_t tol, int exclude_same, uint32_t n_a, uint32_t n_b, uint32_t *__restrict__ bitmap, unsigned long long unit_base)
{
    constexpr uint32_t TILE_ROWS = 256 * R;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long unit = unit_base + blockIdx.x;  // grids above 2^32 work-items are launched in cuts
    const uint32_t chunk = align_seed_unit_chunk((align_u64_ptr)(uintptr_t)unit_offset, n_chunks, unit);
    const uint32_t tile = ((align_u32_ptr)(uintptr_t)tile_first)[chunk] + (uint32_t)(unit - ((align_u64_ptr)(uintptr_t)unit_offset)[chunk]);
    const uint64_t wave_row0 = (uint64_t)tile * TILE_ROWS + wave * (64 * R);  // inside the plan's rows: every class is padded to whole tiles
    if (((align_u32_ptr)(uintptr_t)row_window)[wave_row0] == kSeedRowSentinel) return;  // wave-uniform: a wave of padding rows only (no barrier below)
    const uint32_t s0 = ((align_u32_ptr)(uintptr_t)chunk_first)[chunk], s1 = ((align_u32_ptr)(uintptr_t)chunk_first)[chunk + 1];

    // rows -> VGPRs
    uint32_t rw[R][32];
    uint32_t rvid[R], rskip[R];
#pragma unroll
    for (int k = 0; k < R; k++) {
        const uint64_t r = wave_row0 + k * 64 + lane;
        const uint32_t w = row_window[r];
        if (w != kSeedRowSentinel) {
            align_load_row(rw[k], b_hashes, w);
            rvid[k] = row_video[r];
            rskip[k] = b_skip ? b_skip[w] : 0u;
        } else {
#pragma unroll
            for (int q = 0; q < 32; q++) rw[k][q] = 0u;
            rvid[k] = 0u;
            rskip[k] = 1u;
        }
    }

    align_u32_ptr a_rows = (align_u32_ptr)(uintptr_t)a_hashes;
    for (uint32_t s = s0; s < s1; ++s) {
        const uint32_t sw = ((align_u32_ptr)(uintptr_t)seed_window)[s];
        align_u32_ptr ap = a_rows + (size_t)sw * 32;
        uint32_t d[R];
#pragma unroll
        for (int k = 0; k < R; k++) d[k] = 0u;
#pragma unroll
        for (int w = 0; w < (CHKW < 32 ? CHKW : 32); ++w) {
            const uint32_t aw = ap[w];  // SGPR
#pragma unroll
            for (int k = 0; k < R; k++) d[k] += __builtin_popcount(rw[k][w] ^ aw);
        }
        uint32_t m = d[0];
#pragma unroll
        for (int k = 1; k < R; k++) m = min(m, d[k]);
        if (CHKW < 32) {
            if (__builtin_amdgcn_ballot_w64(m <= tol) == 0ull) continue;  // partial distances only grow
#pragma unroll
            for (int w = CHKW; w < 32; ++w) {
                const uint32_t aw = ap[w];
#pragma unroll
                for (int k = 0; k < R; k++) d[k] += __builtin_popcount(rw[k][w] ^ aw);
            }
            m = d[0];
#pragma unroll
            for (int k = 1; k < R; k++) m = min(m, d[k]);
        }
        if (__builtin_amdgcn_ballot_w64(m <= tol) != 0ull) {
            // rare path: the seed's skip byte (with the aligned dword that holds it, by a scalar load), its video and slot, exclude_same, the bitmap
            bool a_ok = true;
            if (a_skip) {
                const uintptr_t at = (uintptr_t)a_skip + sw;
                a_ok = ((*(align_u32_ptr)(at & ~(uintptr_t)3) >> (8 * (uint32_t)(at & 3))) & 0xFFu) == 0u;
            }
            if (a_ok) {
                const uint32_t sv = ((align_u32_ptr)(uintptr_t)seed_video)[s];
                const uint32_t slot = ((align_u32_ptr)(uintptr_t)seed_slot)[s];
#pragma unroll
                for (int k = 0; k < R; k++) {
                    if (d[k] <= tol && rskip[k] == 0u && (!exclude_same || sv != rvid[k])) {
                        const uint64_t bit = align_seed_rates_bit(slot, sv, rvid[k], n_a, n_b);
                        uint32_t *word = bitmap + (size_t)(bit >> 5);
                        const uint32_t mask = 1u << (uint32_t)(bit & 31);
                        if ((__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & mask) == 0u) atomicOr(word, mask);
                    }
                }
            }
        }
    }
}

// vdf_video_pair_rate has vdf_video_pair_variant's layout, so the triples are scattered by align_seed_variants_scatter_kernel with the identity
// slot table (4 bits per slot: slot s names rate s)
static_assert(sizeof(vdf_video_pair_rate) == sizeof(vdf_video_pair_variant) && offsetof(vdf_video_pair_rate, a) == offsetof(vdf_video_pair_variant, a) &&
                  offsetof(vdf_video_pair_rate, b) == offsetof(vdf_video_pair_variant, b) &&
                  offsetof(vdf_video_pair_rate, rate) == offsetof(vdf_video_pair_variant, variant) && kSeedRatesMax <= 8,
              "vdf_video_pair_rate is scattered as vdf_video_pair_variant");

// count, scan and scatter are launched as they are: 8 slots x 2^24 bits are 2^22 words, 2^14 workgroups of 256 threads, 16 block counts per
// thread of the scan, and a total below 2^27 - all inside 32 bits
hipError_t launch_align_seed_rates(const AlignSeedRatesLaunch &L, hipStream_t stream)
{
    if (L.n_units == 0 || L.n_slots == 0 || L.n_slots > kSeedRatesMax || L.n_words == 0 || L.n_words > kSeedRatesMax * (1u << 19)) return hipErrorInvalidValue;
    for (const AlignLaunchCut &cut : align_launch_cuts((size_t)L.n_units)) {
#define VDF_SEED_RATES_LAUNCH(CW)                                                                                                                       \
    hipLaunchKernelGGL((align_seed_rates_kernel<(int)kSeedRowsPerLane, CW>), dim3((uint32_t)cut.n), dim3(256), 0, stream, L.a_hashes, L.a_skip,          \
                       L.seed_window, L.seed_video, L.seed_slot, L.chunk_first, L.b_hashes, L.b_skip, L.row_window, L.row_video, L.unit_offset,        \
                       L.tile_first, L.n_chunks, L.tol, L.exclude_same, L.n_a, L.n_b, L.bitmap, (unsigned long long)cut.group_base)
        switch (align_seed_check_words(L.tol)) {
        case 14: VDF_SEED_RATES_LAUNCH(14); break;
        case 22: VDF_SEED_RATES_LAUNCH(22); break;
        case 26: VDF_SEED_RATES_LAUNCH(26); break;
        default: VDF_SEED_RATES_LAUNCH(32); break;
        }
#undef VDF_SEED_RATES_LAUNCH
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    const uint32_t n_blocks = (L.n_words + 255) / 256;
    uint32_t *block_count = static_cast<uint32_t *>(L.scratch), *block_offset = block_count + n_blocks, *total = block_offset + n_blocks;
    hipLaunchKernelGGL(align_seed_count_kernel, dim3(n_blocks), dim3(256), 0, stream, L.bitmap, L.n_words, block_count);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(align_scan_kernel, dim3(1), dim3(1024), 0, stream, block_count, n_blocks, block_offset, total);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    *L.total_out = total;
    return hipSuccess;
}

hipError_t launch_align_seed_rates_scatter(const AlignSeedRatesLaunch &L, vdf_video_pair_rate *out, uint32_t limit, hipStream_t stream)
{
    const uint32_t n_blocks = (L.n_words + 255) / 256;
    const uint32_t *block_offset = static_cast<const uint32_t *>(L.scratch) + n_blocks;
    hipLaunchKernelGGL(align_seed_variants_scatter_kernel, dim3(n_blocks), dim3(256), 0, stream, L.bitmap, L.n_words, L.n_a, L.n_b, 0x76543210u, block_offset,
                       reinterpret_cast<vdf_video_pair_variant *>(out), limit);
    return hipGetLastError();
}

}  // namespace vdf
