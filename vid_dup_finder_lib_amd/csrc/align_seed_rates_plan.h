// Seeding of the retimed alignment: every phase of up to 8 rates in one pass (vdf_align_seed_pairs_rates*).  A holds one block
// of retimed windows per listed rate - rate-major, as vdf_hash_windows_clips_u8_rates* writes them - B plain windows.  Under rate r = num / den
// (lowest terms) window ka of video a is a SEED iff (ka / num) % min_run == 0 and window kb of video b is a ROW iff kb % den == 0; pair (a, b) is
// a candidate under r iff some seed and some row match.  This header lists, on the host, what the seed kernel of that call (align.hip:
// align_seed_rates_kernel) walks: rates that share a den form a CLASS and share their rows; the rows of a class are gathered into row_window[] /
// row_video[] and padded to whole tiles with a sentinel; the seeds of a class are listed by (slot, video, ka) and cut into chunks that stay inside
// the class; a unit is (chunk, tile of the chunk's class), decoded with align_plan.h's align_seed_unit_chunk.  No HIP calls: api.cpp and the CPU
// replay (tests/cpp/align_seed_rates_plan_main.cpp) include it.
#pragma once
#include "align_retimed_plan.h"

namespace vdf {

constexpr uint32_t kSeedRatesMax = 8;                    // = VDF_WINDOWS_MAX_RATES: slots of the bitmap
constexpr uint32_t kSeedRowSentinel = 0xFFFFFFFFu;       // row_window[] of a padding row: never a row (fewer than 2^32 rows in all)

struct AlignSeedRate { uint32_t num, den; };             // lowest terms: align_retimed_rate

// is window ka (counted inside its video) a seed under num at min_run?  Sub-sampled index i = ka / num of phase ka % num, i a multiple of min_run
VDF_ALIGN_HD bool align_seed_rates_is_seed(uint32_t ka, uint32_t num, uint32_t min_run) { return (ka / num) % min_run == 0; }
// the bit of (slot, a, b) in the bitmap of a call
VDF_ALIGN_HD uint64_t align_seed_rates_bit(uint32_t slot, uint32_t a, uint32_t b, uint32_t n_a, uint32_t n_b) { return ((uint64_t)slot * n_a + a) * n_b + b; }

struct AlignSeedRatesPlan {
    std::vector<uint32_t> seed_window;   // [seeds]: the seed's row of a_hashes / a_skip: rate_first[slot] + first_a[slot][video] + ka - a_shift
    std::vector<uint32_t> seed_video;    // [seeds]
    std::vector<uint32_t> seed_slot;     // [seeds]: the index of the seed's rate in the job's list
    std::vector<uint32_t> row_window;    // [tiles x tile_rows]: the row of b_hashes / b_skip (- b_shift), or kSeedRowSentinel
    std::vector<uint32_t> row_video;     // [tiles x tile_rows]: 0 at a sentinel
    std::vector<uint32_t> chunk_first;   // [chunks + 1]: chunk c owns the seeds chunk_first[c] ... chunk_first[c + 1], all of one class
    std::vector<uint32_t> tile_first;    // [chunks]: the first tile of the chunk's class
    std::vector<uint64_t> unit_offset;   // [chunks + 1]: chunk c owns one unit per tile of its class; unit u is tile tile_first[c] + u - unit_offset[c]
    std::vector<uint32_t> class_den, class_tile_first, class_tiles, class_rows, chunk_class;  // per class / per chunk: for the replay and the docs
    size_t n_seeds() const { return seed_window.size(); }
    size_t n_chunks() const { return tile_first.size(); }
    size_t n_tiles() const { return row_window.size() / (tile_rows ? tile_rows : 1); }
    uint64_t n_units() const { return unit_offset.empty() ? 0 : unit_offset.back(); }
    uint32_t tile_rows = 0;
};

// first_a: n_rates x (n_a + 1), row r at first_a + r (n_a + 1); rate_first: n_rates + 1 entries or null (zeros).  The rows listed are absolute
// rows of the arrays minus a_shift / b_shift (what a host-array call has cut off in front of its upload).  The caller has checked the first
// arrays (they ascend) and that every row index fits 32 bits.
inline void align_seed_rates_plan(const uint32_t *first_a, const size_t *rate_first, size_t n_a, const uint32_t *first_b, size_t n_b,
                                  const AlignSeedRate *rates, uint32_t n_rates, uint32_t min_run, uint64_t a_shift, uint64_t b_shift, AlignSeedRatesPlan &p,
                                  uint32_t tile_rows = kSeedTileRows, uint32_t chunk = kSeedChunk)
{
    p = AlignSeedRatesPlan{};
    p.tile_rows = tile_rows;
    p.chunk_first.assign(1, 0u);
    p.unit_offset.assign(1, 0ull);
    if (n_a == 0 || n_b == 0) return;
    for (uint32_t r0 = 0; r0 < n_rates; r0++) {
        const uint32_t den = rates[r0].den;
        bool seen = false;
        for (uint32_t r = 0; r < r0; r++) seen = seen || rates[r].den == den;
        if (seen) continue;  // the class of this den is listed already
        // the rows den j of every video of B, then the padding of the class's last tile
        const size_t row0 = p.row_window.size();
        for (size_t b = 0; b < n_b; b++)
            for (uint64_t w = first_b[b]; w < first_b[b + 1]; w += den) {
                p.row_window.push_back((uint32_t)(w - b_shift));
                p.row_video.push_back((uint32_t)b);
            }
        const uint32_t rows = (uint32_t)(p.row_window.size() - row0);
        const uint32_t tiles = (uint32_t)(((uint64_t)rows + tile_rows - 1) / tile_rows);
        p.row_window.resize(row0 + (size_t)tiles * tile_rows, kSeedRowSentinel);
        p.row_video.resize(row0 + (size_t)tiles * tile_rows, 0u);
        const uint32_t cls = (uint32_t)p.class_den.size(), tile0 = (uint32_t)(row0 / tile_rows);
        p.class_den.push_back(den); p.class_tile_first.push_back(tile0); p.class_tiles.push_back(tiles); p.class_rows.push_back(rows);
        // the seeds of the class's rates, by (slot, video, ka)
        const size_t seed0 = p.seed_window.size();
        for (uint32_t r = r0; r < n_rates; r++) {
            if (rates[r].den != den) continue;
            const uint32_t *fa = first_a + (size_t)r * (n_a + 1);
            const uint64_t base = (rate_first ? (uint64_t)rate_first[r] : 0ull) - a_shift;
            for (size_t a = 0; a < n_a; a++) {
                const uint32_t Na = fa[a + 1] - fa[a];
                for (uint32_t ka = 0; ka < Na; ka++)
                    if (align_seed_rates_is_seed(ka, rates[r].num, min_run)) {
                        p.seed_window.push_back((uint32_t)(base + fa[a] + ka));
                        p.seed_video.push_back((uint32_t)a);
                        p.seed_slot.push_back(r);
                    }
            }
        }
        if (tiles == 0) {  // a class without a row has no cell: its seeds are not listed
            p.seed_window.resize(seed0); p.seed_video.resize(seed0); p.seed_slot.resize(seed0);
            continue;
        }
        for (size_t s = seed0; s < p.seed_window.size(); s += chunk) {
            p.chunk_first.push_back((uint32_t)std::min(s + chunk, p.seed_window.size()));
            p.tile_first.push_back(tile0);
            p.chunk_class.push_back(cls);
            p.unit_offset.push_back(p.unit_offset.back() + tiles);
        }
    }
}

}  // namespace vdf
