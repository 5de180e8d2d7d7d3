// Alignment of videos on their window hashes (vdf_align_windows[_device]): which (video a, video b) pairs a call evaluates,
// how a pair's distance matrix is cut into bands of 64 diagonals, which ka range a band walks, how the workgroups of a launch map to
// (pair, band) units - and the lane-ownership rules of the band kernel (align.hip), as __host__ __device__ inline functions so that the
// kernel and the CPU replay (tests/cpp/align_plan_main.cpp) share one text.  No HIP calls: api.cpp and the test program include it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define VDF_ALIGN_HD __host__ __device__ inline
#else
#define VDF_ALIGN_HD inline
#endif

namespace vdf {

constexpr uint32_t kAlignBand = 64;                      // diagonals per band = lanes of a wave
constexpr uint32_t kAlignWaves = 4;                      // (pair, band) units per workgroup: one per wave
constexpr uint32_t kAlignMaxWindows = 1u << 20;          // per video: score = n (tol + 1) - dist_sum <= 2^20 * 1025 < 2^31
constexpr uint64_t kAlignMaxPairs = 1ull << 24;          // per call
constexpr size_t kAlignMaxGroupsPerLaunch = size_t(1) << 23;  // x 256 threads stays under HIP's 2^32 work-item grid limit
// A call is evaluated in chunks of consecutive pairs: a chunk closes once it holds this many pairs or units (it always takes one pair,
// and one pair has at most 2^15 bands), which bounds the scratch of a call: 16 B per unit, 24 B + 24 B per pair.
constexpr size_t kAlignChunkPairs = size_t(1) << 20;
constexpr size_t kAlignChunkUnits = size_t(1) << 22;

// ---- one pair: Na x Nb cells (ka, kb), diagonal d = kb - ka in [-(Na - 1), Nb - 1] -----------------------------------------------------------
VDF_ALIGN_HD uint32_t align_bands(uint32_t Na, uint32_t Nb) { return (Na == 0 || Nb == 0) ? 0u : (Na + Nb - 1 + kAlignBand - 1) / kAlignBand; }
// band j owns the diagonals d0 ... d0 + 63
VDF_ALIGN_HD int32_t align_band_d0(uint32_t Na, uint32_t band) { return -(int32_t)(Na - 1) + (int32_t)(band * kAlignBand); }
// the steps ka a band needs: every cell of its diagonals lies in [ka_begin, ka_end), and at both ends some diagonal has a cell
VDF_ALIGN_HD uint32_t align_ka_begin(int32_t d0) { const int32_t d_hi = d0 + (int32_t)kAlignBand - 1; return d_hi < 0 ? (uint32_t)(-d_hi) : 0u; }
VDF_ALIGN_HD uint32_t align_ka_end(uint32_t Na, uint32_t Nb, int32_t d0) { const int64_t e = (int64_t)Nb - d0; return e < (int64_t)Na ? (uint32_t)e : Na; }

// ---- lane ownership inside a band (one wave) --------------------------------------------------------------------------------------------------
// Row kb of B lives in lane kb mod 64 for as long as the band needs it (kb may be negative or >= Nb: a cell outside the matrix, never loaded).
VDF_ALIGN_HD uint32_t align_row_lane(int32_t kb) { return (uint32_t)kb & (kAlignBand - 1); }
// the row a lane holds at step ka: the one of ka + d0 ... ka + d0 + 63 that is congruent to the lane
VDF_ALIGN_HD int32_t align_lane_row(uint32_t lane, uint32_t ka, int32_t d0)
{
    const int32_t base = (int32_t)ka + d0;
    return base + (int32_t)((lane - (uint32_t)base) & (kAlignBand - 1));
}
// after step ka the row ka + d0 (diagonal d0) is done; its lane takes row ka + d0 + 64 (diagonal d0 + 63 of step ka + 1) - if there is a step ka + 1
VDF_ALIGN_HD uint32_t align_reload_lane(uint32_t ka, int32_t d0) { return align_row_lane((int32_t)ka + d0); }
VDF_ALIGN_HD int32_t align_reload_row(uint32_t ka, int32_t d0) { return (int32_t)ka + d0 + (int32_t)kAlignBand; }
// the run state (length, dist_sum) of diagonal d is read and written at step ka by the lane of its cell's row; between two steps every
// lane takes the state of the lane below it (lane 0 that of lane 63): the state follows its diagonal
VDF_ALIGN_HD uint32_t align_state_lane(int32_t d, uint32_t ka) { return align_row_lane((int32_t)ka + d); }
VDF_ALIGN_HD uint32_t align_rotate_source(uint32_t lane) { return (lane - 1) & (kAlignBand - 1); }

// ---- ranking: the better of two runs (score = n (tol + 1) - dist_sum; 0 = no run) -----------------------------------------------------------
VDF_ALIGN_HD bool align_better(uint32_t score, int32_t offset, uint32_t start_a, uint32_t best_score, int32_t best_offset, uint32_t best_start_a)
{
    if (score != best_score) return score > best_score;
    if (offset != best_offset) return offset < best_offset;
    return start_a < best_start_a;
}

// ---- the pairs of a call and their units ------------------------------------------------------------------------------------------------------
struct AlignPair { uint32_t a, b; };
// what a band leaves in scratch: its best run (n_windows = 0: none)
struct AlignBandRecord { int32_t offset; uint32_t start_a, n_windows, dist_sum; };

inline uint64_t align_pair_count(uint64_t n_a, uint64_t n_b, bool self) { return self ? n_a * (n_a - (n_a ? 1 : 0)) / 2 : n_a * n_b; }

// Walks the pairs of a call in (a, b) order - all a x b, or a < b in self mode - and cuts them into chunks.
struct AlignChunk {
    std::vector<AlignPair> pairs;      // pairs with at least one band (a video of 0 windows pairs with nothing)
    std::vector<uint32_t> unit_offset; // [pairs + 1]: pair i owns the units unit_offset[i] ... unit_offset[i + 1], one per band
    size_t n_units() const { return unit_offset.empty() ? 0 : unit_offset.back(); }
    size_t n_groups() const { return (n_units() + kAlignWaves - 1) / kAlignWaves; }
};
struct AlignCursor { uint64_t a = 0, b = 0; bool started = false; };

// Fills `c` with the next chunk; false once the pairs are used up (c is then empty).  first_b = first_a, n_b = n_a in self mode.
inline bool align_next_chunk(const uint32_t *first_a, size_t n_a, const uint32_t *first_b, size_t n_b, bool self, AlignCursor &cur, AlignChunk &c,
                             size_t max_pairs = kAlignChunkPairs, size_t max_units = kAlignChunkUnits)
{
    c.pairs.clear();
    c.unit_offset.assign(1, 0u);
    if (!cur.started) { cur.started = true; cur.a = 0; cur.b = self ? 1 : 0; }
    size_t units = 0;
    while (cur.a < n_a) {
        if (cur.b >= n_b) { cur.a++; cur.b = self ? cur.a + 1 : 0; continue; }
        const uint32_t Na = first_a[cur.a + 1] - first_a[cur.a], Nb = first_b[cur.b + 1] - first_b[cur.b];
        const uint32_t bands = align_bands(Na, Nb);
        if (bands) {
            if (!c.pairs.empty() && (c.pairs.size() >= max_pairs || units + bands > max_units)) return true;
            c.pairs.push_back({(uint32_t)cur.a, (uint32_t)cur.b});
            units += bands;
            c.unit_offset.push_back((uint32_t)units);
        }
        cur.b++;
    }
    return !c.pairs.empty();
}

// unit -> pair of the chunk: the largest i with unit_offset[i] <= unit (the kernel makes the same search)
template <class Ptr> VDF_ALIGN_HD uint32_t align_unit_pair(Ptr unit_offset, uint32_t n_pairs, uint32_t unit)
{
    uint32_t lo = 0, hi = n_pairs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (unit_offset[mid] <= unit) lo = mid; else hi = mid;
    }
    return lo;
}

// launches of a chunk: [group_base, group_base + n) for every cut of at most kAlignMaxGroupsPerLaunch workgroups
struct AlignLaunchCut { size_t group_base, n; };
inline std::vector<AlignLaunchCut> align_launch_cuts(size_t n_groups, size_t max_groups = kAlignMaxGroupsPerLaunch)
{
    std::vector<AlignLaunchCut> cuts;
    for (size_t g = 0; g < n_groups; g += max_groups) cuts.push_back({g, std::min(max_groups, n_groups - g)});
    return cuts;
}

// ---- more than one stretch per pair (vdf_align_windows_stretches*) --------------------------------------------------------------
// Rank r of a pair is the best run of its matrix with the rectangles of ranks 0 ... r - 1 masked: a masked cell is a miss.  A chunk is walked
// in rounds: round 0 is the plain launch on the chunk's pairs, round r >= 1 the masked kernel on the SURVIVORS - the pairs that had a record in
// round r - 1 - each with exactly r rectangles.
constexpr uint32_t kAlignMaxStretches = 8;       // ranks per pair: at most 7 rectangles in a masked round
constexpr uint32_t kAlignMaxGuard = 1u << 20;    // = kAlignMaxWindows: a wider guard masks no more

struct AlignRect { uint32_t a_lo, a_hi, b_lo, b_hi; };  // [a_lo, a_hi) x [b_lo, b_hi); a_lo == a_hi: empty

// the rectangle a reported stretch masks: its rows of A and of B (start_b = start_a + offset), each widened by guard and clipped to the matrix.
// 64-bit arithmetic: nothing wraps for any start, n and guard of 32 bits.
VDF_ALIGN_HD AlignRect align_rect_of(int32_t offset, uint32_t start_a, uint32_t n, uint32_t guard, uint32_t Na, uint32_t Nb)
{
    const int64_t sa = (int64_t)start_a, sb = sa + offset, g = (int64_t)guard, len = (int64_t)n, na = (int64_t)Na, nb = (int64_t)Nb;
    const auto clip = [](int64_t v, int64_t hi) { return (uint32_t)(v < 0 ? 0 : v > hi ? hi : v); };  // a stretch outside the matrix: an empty range
    return AlignRect{clip(sa - g, na), clip(sa + len + g, na), clip(sb - g, nb), clip(sb + len + g, nb)};
}
VDF_ALIGN_HD bool align_rect_has_a(const AlignRect &r, uint32_t ka) { return ka >= r.a_lo && ka < r.a_hi; }
VDF_ALIGN_HD bool align_rect_has_b(const AlignRect &r, uint32_t kb) { return kb >= r.b_lo && kb < r.b_hi; }
// a cell is masked iff ONE rectangle holds both its row of A and its row of B (kb of a cell outside the matrix, cast from a negative
// int32_t, is above every b_hi)
template <class Ptr> VDF_ALIGN_HD bool align_cell_masked(Ptr rects, uint32_t n_rects, uint32_t ka, uint32_t kb)
{
    bool masked = false;
    for (uint32_t i = 0; i < n_rects; i++) masked = masked || (align_rect_has_a(rects[i], ka) && align_rect_has_b(rects[i], kb));
    return masked;
}

// One round of a chunk: its pairs in (a, b) order, their units, and rects[pair * n_rects + i], the rectangles of ranks 0 ... n_rects - 1.
struct AlignRound {
    std::vector<AlignPair> pairs;
    std::vector<uint32_t> unit_offset;  // [pairs + 1]
    std::vector<AlignRect> rects;       // [pairs][n_rects]
    uint32_t n_rects = 0;               // = the round's number
    size_t n_units() const { return unit_offset.empty() ? 0 : unit_offset.back(); }
};
// round 0 of a chunk: all of its pairs, no rectangle.  The chunk's arrays are TAKEN, not copied (a chunk holds up to 2^20 pairs, and a call
// whose pairs have no record must cost what the plain call costs); align_next_chunk refills the chunk from scratch.
inline void align_round_zero(AlignChunk &c, AlignRound &r0)
{
    r0.pairs.swap(c.pairs);
    r0.unit_offset.swap(c.unit_offset);
    c.pairs.clear();
    c.unit_offset.assign(1, 0u);
    r0.rects.clear();
    r0.n_rects = 0;
}
// Round prev.n_rects + 1 from round prev and its records (one per pair of prev that had a competing run, in (a, b) order; Rec has a, b, offset,
// start_a, n_windows): the pairs with a record survive, in (a, b) order, each with its rectangles so far and the one of its new record, and
// the same align_bands units as before.  So a round is a subset of its predecessor and of its chunk: it stays inside the chunk's pair and unit
// limits, and the scratch of the chunk's round 0 holds every later round (align_scratch_bytes grows with both counts).  False: a record
// names a pair that prev does not hold in that order - not a result of prev.
template <class Rec>
inline bool align_next_round(const AlignRound &prev, const Rec *recs, size_t n_recs, const uint32_t *first_a, const uint32_t *first_b, uint32_t guard,
                             AlignRound &next)
{
    next.pairs.clear();
    next.unit_offset.assign(1, 0u);
    next.rects.clear();
    next.n_rects = prev.n_rects + 1;
    size_t p = 0;
    for (size_t i = 0; i < n_recs; i++) {
        while (p < prev.pairs.size() && (prev.pairs[p].a != recs[i].a || prev.pairs[p].b != recs[i].b)) p++;
        if (p == prev.pairs.size()) return false;
        const uint32_t Na = first_a[recs[i].a + 1] - first_a[recs[i].a], Nb = first_b[recs[i].b + 1] - first_b[recs[i].b];
        next.pairs.push_back(prev.pairs[p]);
        next.unit_offset.push_back(next.unit_offset.back() + (prev.unit_offset[p + 1] - prev.unit_offset[p]));
        for (uint32_t k = 0; k < prev.n_rects; k++) next.rects.push_back(prev.rects[p * prev.n_rects + k]);
        next.rects.push_back(align_rect_of(recs[i].offset, recs[i].start_a, recs[i].n_windows, guard, Na, Nb));
        p++;
    }
    return next.pairs.size() <= prev.pairs.size() && next.n_units() <= prev.n_units();
}

// ---- a caller-given list of pairs instead of all of them (vdf_align_windows_pairs*, vdf_align_windows_stretches_pairs*) --------
// What a pair list must be: strictly increasing in (a, b), a < n_a, b < n_b, and a < b in self mode.  0: fine; 1: not strictly increasing at
// *at (unsorted or a duplicate); 2: pair *at names a video that does not exist; 3: pair *at has a >= b in self mode.
template <class P> inline int align_pair_list_check(const P *list, size_t n_list, size_t n_a, size_t n_b, bool self, size_t *at)
{
    for (size_t i = 0; i < n_list; i++) {
        *at = i;
        if (i && (list[i].a < list[i - 1].a || (list[i].a == list[i - 1].a && list[i].b <= list[i - 1].b))) return 1;
        if (list[i].a >= n_a || list[i].b >= (self ? n_a : n_b)) return 2;
        if (self && list[i].a >= list[i].b) return 3;
    }
    return 0;
}

// The list of vdf_align_windows_variants_pairs* (DESIGN.md 4.14): strictly increasing in (variant, a, b), every variant in 1 ... 7, the pair
// rules above.  0: fine; 1: not strictly increasing at *at; 2: video; 3: a >= b in self mode; 4: entry *at has a variant outside 1 ... 7.
template <class T> inline int align_triple_list_check(const T *list, size_t n_list, size_t n_a, size_t n_b, bool self, size_t *at)
{
    for (size_t i = 0; i < n_list; i++) {
        *at = i;
        if (i) {
            const T &p = list[i - 1], &q = list[i];
            if (q.variant < p.variant || (q.variant == p.variant && (q.a < p.a || (q.a == p.a && q.b <= p.b)))) return 1;
        }
        if (list[i].variant < 1 || list[i].variant > 7) return 4;
        if (list[i].a >= n_a || list[i].b >= (self ? n_a : n_b)) return 2;
        if (self && list[i].a >= list[i].b) return 3;
    }
    return 0;
}

// align_next_chunk fed from a checked pair list: the same limits per chunk, pairs with a video of 0 windows skipped.  cur: the next list entry.
template <class P>
inline bool align_next_chunk_pairs(const uint32_t *first_a, const uint32_t *first_b, const P *list, size_t n_list, size_t &cur, AlignChunk &c,
                                   size_t max_pairs = kAlignChunkPairs, size_t max_units = kAlignChunkUnits)
{
    c.pairs.clear();
    c.unit_offset.assign(1, 0u);
    size_t units = 0;
    for (; cur < n_list; cur++) {
        const uint32_t a = list[cur].a, b = list[cur].b;
        const uint32_t bands = align_bands(first_a[a + 1] - first_a[a], first_b[b + 1] - first_b[b]);
        if (!bands) continue;
        if (!c.pairs.empty() && (c.pairs.size() >= max_pairs || units + bands > max_units)) return true;
        c.pairs.push_back({a, b});
        units += bands;
        c.unit_offset.push_back((uint32_t)units);
    }
    return !c.pairs.empty();
}

// ---- seeding: which pairs of videos can have a record at all (vdf_align_seed_pairs*) ---------------------------------------------
// A competing run has min_run consecutive matching cells on one diagonal, and any min_run consecutive ka hold a multiple of min_run: a pair
// with a record has a matching cell whose ka - counted inside video a - is a multiple of min_run.  Those windows of A are the SEEDS; the seed
// kernel (align.hip) compares every seed with every row of B and marks the pairs of videos that have a matching cell.
// Rows of B are cut into tiles (a workgroup keeps a tile in VGPRs), seeds into chunks (a workgroup streams one through SGPRs); a UNIT is
// (chunk, tile).  In self mode only the cells with seed video < row video count: both video arrays ascend, so the tiles that hold such a
// cell for chunk c are a suffix of the tiles, tile_first[c] ... n_tiles - 1 - the triangle.
constexpr uint32_t kSeedRowsPerLane = 2;                       // the VALU search backend's default instantiation (hamming.hip)
constexpr uint32_t kSeedTileRows = 256 * kSeedRowsPerLane;
constexpr uint32_t kSeedChunk = 256;                           // seeds per unit
constexpr uint32_t kSeedVariantsTileRows = 256;                // the seed pass against the variants keeps ONE class-major row per lane
// The exact early exit: after this many of a hash's 32 dwords, unrelated hashes (partial distance 16 w +- sqrt(8 w)) are, 4 sigma down, still
// more than tol apart, and nearly every (seed, wave) stops there.  32: no test.  The kernel is instantiated for 14, 22, 26 and 32.
inline uint32_t align_seed_check_words(uint32_t tol)
{
    for (uint32_t w : {14u, 22u, 26u}) {
        uint32_t r = 0;  // floor(sqrt(32 w))
        while ((r + 1) * (r + 1) <= 32 * w) r++;
        if (16 * w >= tol + 1 + 2 * (r + 1)) return w;
    }
    return 32;
}

struct AlignSeedPlan {
    std::vector<uint32_t> seed_window;  // [seeds]: the seed's row of A (an index into a_hashes, as first_a counts)
    std::vector<uint32_t> seed_video;   // [seeds]: ascending
    std::vector<uint32_t> row_video;    // [rows]: the video of row r of B; row r is window row_base + r of b_hashes.  Ascending
    std::vector<uint32_t> tile_first;   // [chunks]: the first tile chunk c is compared with
    std::vector<uint64_t> unit_offset;  // [chunks + 1]: chunk c owns the units unit_offset[c] ..., unit u is tile tile_first[c] + u - unit_offset[c]
    uint32_t row_base = 0, n_rows = 0, n_tiles = 0;
    size_t n_seeds() const { return seed_window.size(); }
    size_t n_chunks() const { return tile_first.size(); }
    uint64_t n_units() const { return unit_offset.empty() ? 0 : unit_offset.back(); }
};

// first_b = first_a, n_b = n_a in self mode
inline void align_seed_plan(const uint32_t *first_a, size_t n_a, const uint32_t *first_b, size_t n_b, bool self, uint32_t min_run, AlignSeedPlan &p,
                            uint32_t tile_rows = kSeedTileRows, uint32_t chunk = kSeedChunk)
{
    p.seed_window.clear(); p.seed_video.clear(); p.row_video.clear(); p.tile_first.clear(); p.unit_offset.assign(1, 0ull);
    p.row_base = n_b ? first_b[0] : 0;
    p.n_rows = n_b ? first_b[n_b] - first_b[0] : 0;
    p.n_tiles = (uint32_t)(((uint64_t)p.n_rows + tile_rows - 1) / tile_rows);
    for (size_t a = 0; a < n_a; a++)
        for (uint64_t w = first_a[a]; w < first_a[a + 1]; w += min_run) {  // ka = w - first_a[a] = 0, min_run, 2 min_run, ...
            p.seed_window.push_back((uint32_t)w);
            p.seed_video.push_back((uint32_t)a);
        }
    p.row_video.resize(p.n_rows);
    for (size_t b = 0; b < n_b; b++)
        for (uint32_t w = first_b[b]; w < first_b[b + 1]; w++) p.row_video[w - p.row_base] = (uint32_t)b;
    if (p.n_rows == 0) return;
    const size_t n_chunks = (p.n_seeds() + chunk - 1) / chunk;
    uint32_t t = 0;
    for (size_t c = 0; c < n_chunks; c++) {
        if (self) {  // the first tile whose largest row video is above the chunk's smallest seed video; it ascends with c
            const uint32_t v_min = p.seed_video[c * chunk];
            while (t < p.n_tiles && p.row_video[std::min<uint64_t>((uint64_t)(t + 1) * tile_rows, p.n_rows) - 1] <= v_min) t++;
        }
        p.tile_first.push_back(t);
        p.unit_offset.push_back(p.unit_offset.back() + (p.n_tiles - t));
    }
}

// unit -> chunk: the largest c with unit_offset[c] <= unit, among the chunks that own a unit (the kernel makes the same search)
template <class Ptr> VDF_ALIGN_HD uint32_t align_seed_unit_chunk(Ptr unit_offset, uint32_t n_chunks, uint64_t unit)
{
    uint32_t lo = 0, hi = n_chunks;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (unit_offset[mid] <= unit) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace vdf
