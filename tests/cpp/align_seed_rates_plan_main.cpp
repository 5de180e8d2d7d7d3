// The planner behind vdf_align_seed_pairs_rates* (csrc/align_seed_rates_plan.h) replayed on the CPU, built with
// -fsanitize=address,undefined by tests/test_align_seed_rates_plan.py.  For window counts 0 .. 140 per video - three videos per side, one of
// them empty - and the seven rates of the retimed planner's test in ONE list (classes of den 1 (two rates), 2, 4, 5, 16 and 17), at min_run
// 1 .. 3, with tiles and chunks of a few rows and of the kernel's own size and first arrays that begin at 0, 3 and 5, the units of the plan are
// walked as the seed kernel (csrc/align.hip: align_seed_rates_kernel) walks them - unit -> chunk -> tile, four waves, 64 lanes, R rows per lane -
// with the header's own functions, and
//   - the seeds are exactly the windows of the definition, by (class, slot, video, ka), each with its video, slot and absolute row;
//   - the gathered rows are exactly the windows den j of every video of B, none at or behind its video's end;
//   - every (seed, row) cell of the definition is visited by exactly one (unit, lane, k), and nothing else is;
//   - no chunk straddles a class; sentinels appear only as the suffix of a class's last tile, and a wave that leaves holds sentinels only;
//   - the launch cuts cover the units once.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "align_seed_rates_plan.h"

using namespace vdf;

#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond)) {                                           \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                            \
            std::printf("\n");                                   \
            std::exit(1);                                        \
        }                                                        \
    } while (0)

static unsigned long long g_cells = 0, g_units = 0, g_plans = 0;

static void replay(const std::vector<uint32_t> &ca, const std::vector<uint32_t> &cb, const std::vector<AlignSeedRate> &rates, uint32_t min_run, uint32_t tile_rows,
                   uint32_t chunk, uint32_t a_base, uint32_t b_base, bool with_rate_first, size_t max_groups)
{
    const size_t n_a = ca.size(), n_b = cb.size();
    const uint32_t n_rates = (uint32_t)rates.size();
    // the layout of a hash call: every block is a library of its own; without rate_first the blocks lie on top of each other (legal: zeros)
    std::vector<uint32_t> fa(n_rates * (n_a + 1)), fb(n_b + 1, b_base);
    std::vector<size_t> rate_first(n_rates + 1, 0);
    for (uint32_t r = 0; r < n_rates; r++) {
        uint32_t *f = fa.data() + (size_t)r * (n_a + 1);
        f[0] = a_base + r;
        for (size_t a = 0; a < n_a; a++) f[a + 1] = f[a] + ca[a];
        rate_first[r + 1] = rate_first[r] + f[n_a];
    }
    for (size_t b = 0; b < n_b; b++) fb[b + 1] = fb[b] + cb[b];
    const uint64_t a_shift = a_base, b_shift = b_base;  // what a host-array call cuts off in front of its uploads
    AlignSeedRatesPlan p;
    align_seed_rates_plan(fa.data(), with_rate_first ? rate_first.data() : nullptr, n_a, fb.data(), n_b, rates.data(), n_rates, min_run, a_shift, b_shift, p,
                          tile_rows, chunk);
    g_plans++;
    CHECK(p.row_window.size() == p.row_video.size() && p.row_window.size() % tile_rows == 0, "rows are whole tiles");
    CHECK(p.seed_window.size() == p.seed_video.size() && p.seed_window.size() == p.seed_slot.size(), "seed arrays");
    CHECK(p.chunk_first.size() == p.n_chunks() + 1 && p.unit_offset.size() == p.n_chunks() + 1 && p.chunk_class.size() == p.n_chunks(), "chunk arrays");

    // the classes, their rows and their seeds by the definition
    struct Seed { uint32_t slot, a, ka; };
    std::vector<uint32_t> dens;
    for (const AlignSeedRate &r : rates) {
        bool seen = false;
        for (uint32_t d : dens) seen = seen || d == r.den;
        if (!seen) dens.push_back(r.den);
    }
    if (n_a == 0 || n_b == 0) dens.clear();
    CHECK(p.class_den == dens, "%zu classes of %zu", p.class_den.size(), dens.size());
    std::vector<Seed> seeds;
    std::vector<uint32_t> seed_class;
    size_t row_at = 0;
    for (size_t c = 0; c < dens.size(); c++) {
        const uint32_t den = dens[c];
        CHECK(row_at % tile_rows == 0 && p.class_tile_first[c] == row_at / tile_rows, "class %zu begins at a tile", c);
        uint32_t rows = 0;
        for (size_t b = 0; b < n_b; b++)
            for (uint32_t kb = 0; kb < cb[b]; kb += den, rows++, row_at++) {
                CHECK(row_at < p.row_window.size() && p.row_window[row_at] == fb[b] + kb - b_shift && p.row_video[row_at] == b, "class %zu row %u", c, rows);
                CHECK((uint64_t)p.row_window[row_at] + b_shift >= fb[b] && (uint64_t)p.row_window[row_at] + b_shift < fb[b + 1], "a row behind its video's end");
            }
        CHECK(p.class_rows[c] == rows && p.class_tiles[c] == (rows + tile_rows - 1) / tile_rows, "class %zu has %u rows", c, rows);
        for (; row_at < ((size_t)p.class_tile_first[c] + p.class_tiles[c]) * tile_rows; row_at++)  // sentinels: the suffix of the class's last tile only
            CHECK(p.row_window[row_at] == kSeedRowSentinel && row_at / tile_rows == (size_t)p.class_tile_first[c] + p.class_tiles[c] - 1, "padding at row %zu", row_at);
        if (rows == 0) continue;
        for (uint32_t r = 0; r < n_rates; r++) {
            if (rates[r].den != den) continue;
            for (size_t a = 0; a < n_a; a++)
                for (uint32_t ka = 0; ka < ca[a]; ka++)
                    if ((ka / rates[r].num) % min_run == 0) { seeds.push_back({r, (uint32_t)a, ka}); seed_class.push_back((uint32_t)c); }
        }
    }
    CHECK(row_at == p.row_window.size(), "rows behind the last class");
    CHECK(seeds.size() == p.n_seeds(), "%zu seeds of %zu", p.n_seeds(), seeds.size());
    for (size_t s = 0; s < seeds.size(); s++) {
        const uint64_t row = (with_rate_first ? rate_first[seeds[s].slot] : 0) + fa[(size_t)seeds[s].slot * (n_a + 1) + seeds[s].a] + seeds[s].ka - a_shift;
        CHECK(p.seed_slot[s] == seeds[s].slot && p.seed_video[s] == seeds[s].a && p.seed_window[s] == row, "seed %zu", s);
    }
    // chunks: inside one class, in order, none empty, at most `chunk` seeds
    for (size_t c = 0; c < p.n_chunks(); c++) {
        CHECK(p.chunk_first[c] < p.chunk_first[c + 1] && p.chunk_first[c + 1] - p.chunk_first[c] <= chunk && p.chunk_first[c + 1] <= seeds.size(), "chunk %zu", c);
        for (uint32_t s = p.chunk_first[c]; s < p.chunk_first[c + 1]; s++)
            CHECK(seed_class[s] == p.chunk_class[c] && rates[p.seed_slot[s]].den == p.class_den[p.chunk_class[c]], "chunk %zu straddles a class at seed %u", c, s);
        CHECK(p.tile_first[c] == p.class_tile_first[p.chunk_class[c]] && p.unit_offset[c + 1] - p.unit_offset[c] == p.class_tiles[p.chunk_class[c]], "units of chunk %zu", c);
    }
    CHECK(p.chunk_first[0] == 0 && p.chunk_first[p.n_chunks()] == seeds.size() && p.unit_offset[0] == 0, "the chunks cover the seeds");
    if (p.n_units() == 0) {
        CHECK(seeds.empty(), "seeds without a unit");
        return;
    }
    // the kernel's walk
    const size_t n_rows = p.row_window.size();
    const uint32_t waves = 4, R = tile_rows >= 8 ? 2 : 1, wave_rows = tile_rows / waves, lanes = wave_rows / R;
    CHECK(lanes * R * waves == tile_rows, "tile shape");
    std::vector<uint8_t> visited(seeds.size() * n_rows, 0);
    size_t groups = 0;
    for (const AlignLaunchCut &cut : align_launch_cuts((size_t)p.n_units(), max_groups)) {
        CHECK(cut.n >= 1 && cut.n <= max_groups && cut.group_base == groups, "cut");
        for (size_t g = 0; g < cut.n; g++) {
            const uint64_t unit = cut.group_base + g;
            const uint32_t c = align_seed_unit_chunk(p.unit_offset.data(), (uint32_t)p.n_chunks(), unit);
            CHECK(c < p.n_chunks() && p.unit_offset[c] <= unit && unit < p.unit_offset[c + 1], "unit %llu -> chunk %u", (unsigned long long)unit, c);
            const uint32_t tile = p.tile_first[c] + (uint32_t)(unit - p.unit_offset[c]);
            CHECK(tile < p.n_tiles(), "unit %llu -> tile %u", (unsigned long long)unit, tile);
            for (uint32_t wave = 0; wave < waves; wave++) {
                const uint64_t wave_row0 = (uint64_t)tile * tile_rows + wave * wave_rows;
                CHECK(wave_row0 < n_rows, "a wave outside the rows");
                if (p.row_window[wave_row0] == kSeedRowSentinel) {
                    for (uint32_t i = 0; i < wave_rows; i++) CHECK(p.row_window[wave_row0 + i] == kSeedRowSentinel, "a wave that leaves holds a row");
                    continue;
                }
                for (uint32_t lane = 0; lane < lanes; lane++)
                    for (uint32_t k = 0; k < R; k++) {
                        const uint64_t r = wave_row0 + k * lanes + lane;
                        CHECK(r < n_rows, "a lane outside the rows");
                        if (p.row_window[r] == kSeedRowSentinel) continue;
                        for (uint32_t s = p.chunk_first[c]; s < p.chunk_first[c + 1]; s++) {
                            CHECK(visited[s * n_rows + r] == 0, "cell (%u, %llu) twice", s, (unsigned long long)r);
                            visited[s * n_rows + r] = 1;
                        }
                    }
            }
            g_units++;
        }
        groups += cut.n;
    }
    CHECK(groups == p.n_units(), "cuts cover %zu of %llu units", groups, (unsigned long long)p.n_units());
    for (size_t s = 0; s < seeds.size(); s++)
        for (size_t r = 0; r < n_rows; r++) {
            const uint32_t c = seed_class[s];
            const bool cell = p.row_window[r] != kSeedRowSentinel && r / tile_rows >= p.class_tile_first[c] && r / tile_rows < p.class_tile_first[c] + p.class_tiles[c];
            CHECK(visited[s * n_rows + r] == (cell ? 1 : 0), "cell (seed %zu, row %zu): %d visits, wanted %d", s, r, visited[s * n_rows + r], (int)cell);
            g_cells += cell;
        }
}

int main()
{
    const uint32_t raw[7][2] = {{1, 1}, {2, 1}, {3, 2}, {5, 4}, {6, 5}, {31, 16}, {32, 17}};
    std::vector<AlignSeedRate> rates;
    for (const auto &r : raw) {
        AlignSeedRate x{};
        CHECK(align_retimed_rate(r[0], r[1], &x.num, &x.den) == 0, "rate");
        rates.push_back(x);
    }
    const uint32_t fixed_b[] = {0, 1, 16, 17, 35, 140}, fixed_a[] = {0, 1, 31, 33, 140};
    for (uint32_t n = 0; n <= 140; n++) {
        const uint32_t min_run = 1 + n % 3, base = n % 3 == 0 ? 0 : (n % 3 == 1 ? 3 : 5);
        const bool big = n % 4 == 0;  // the kernel's own tile and chunk on every fourth count, a few rows and seeds otherwise
        for (uint32_t nb : fixed_b)
            replay({n, 3, 0}, {0, nb, 2}, rates, min_run, big ? kSeedTileRows : 8, big ? kSeedChunk : 5, base, 5 - base, n % 2 == 0, n % 5 ? (size_t)1 << 23 : 3);
        for (uint32_t na : fixed_a)
            replay({0, na, 2}, {n, 0, 5}, rates, min_run, big ? kSeedTileRows : 8, big ? kSeedChunk : 5, base, 5 - base, n % 2 == 1, n % 5 ? (size_t)1 << 23 : 3);
    }
    // the shapes of the GPU tests: classes of 2610, 1306, 654 and 523 rows, more than one chunk per class at min_run 1 .. 3
    std::vector<AlignSeedRate> usual(rates.begin(), rates.begin() + 5);
    for (uint32_t min_run = 1; min_run <= 3; min_run++) replay({0, 1, 2, 3, 31, 33, 600}, {0, 1, 4, 700, 5, 1900}, usual, min_run, kSeedTileRows, kSeedChunk, 5, 3, true, (size_t)1 << 23);
    // duplicate rates: each gets its slot, both in the class of their den
    replay({40, 7}, {9, 50}, {{32, 17}, {32, 17}, {3, 2}, {3, 2}, {1, 1}}, 2, 8, 5, 0, 0, true, 7);
    // empty sides and a one-rate list
    replay({}, {4}, usual, 1, 8, 5, 0, 0, true, 4);
    replay({4}, {}, usual, 1, 8, 5, 0, 0, true, 4);
    replay({4}, {0, 0}, usual, 1, 8, 5, 0, 0, false, 4);
    replay({0}, {7}, usual, 1, 8, 5, 0, 0, false, 4);
    replay({70, 1}, {33}, {{3, 2}}, 2, 8, 5, 2, 1, true, 4);
    CHECK(align_seed_rates_bit(0, 0, 0, 7, 6) == 0 && align_seed_rates_bit(1, 0, 0, 7, 6) == 42 && align_seed_rates_bit(4, 6, 5, 7, 6) == 209, "bit index");
    CHECK(align_seed_rates_is_seed(0, 3, 2) && align_seed_rates_is_seed(2, 3, 2) && !align_seed_rates_is_seed(3, 3, 2) && align_seed_rates_is_seed(6, 3, 2), "seeds");
    std::printf("align seed rates plan ok: %llu plans, %llu cells in %llu units\n", g_plans, g_cells, g_units);
    return 0;
}
