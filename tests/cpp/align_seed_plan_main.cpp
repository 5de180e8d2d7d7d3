// The planner behind vdf_align_seed_pairs* and the *_pairs calls (csrc/align_plan.h: AlignSeedPlan, align_seed_plan, align_seed_unit_chunk,
// align_next_chunk_pairs, align_pair_list_check) replayed on the CPU, built with -fsanitize=address,undefined by
// tests/test_align_seed_plan.py.  For every combination of window counts 0 .. 3 of three videos per side (five in self mode) - empty videos in
// every position - at min_run 1 .. 4, with tiles and chunks of a few rows and of the kernel's own size, and with first arrays that begin at 0
// and at 5: the units of the plan are walked as the seed kernel (csrc/align.hip) walks them, with the header's own functions, and
//   - the seeds are exactly the windows of A whose index inside their video is a multiple of min_run, in order, each with its video;
//   - every row of B carries its video;
//   - every (seed, row) cell with seed video < row video - any cell between two sets - lies in exactly one unit, no cell in two;
//   - no unit reaches outside the seeds, the rows, the tiles or the chunks, and the launch cuts cover the units once.
// Pair lists: the chunks of align_next_chunk_pairs hold the listed pairs that have a band, once, in order, within their limits; the list
// check names the first offence of every kind.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "align_plan.h"

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

static std::vector<uint32_t> first_of(const std::vector<uint32_t> &counts, uint32_t base)
{
    std::vector<uint32_t> f(1, base);
    for (uint32_t n : counts) f.push_back(f.back() + n);
    return f;
}

static void replay_seed(const std::vector<uint32_t> &ca, const std::vector<uint32_t> &cb, bool self, uint32_t min_run, uint32_t tile_rows, uint32_t chunk,
                        uint32_t base, size_t max_groups, unsigned long long *cells_seen, unsigned long long *units_seen)
{
    const std::vector<uint32_t> fa = first_of(ca, base), fb = self ? fa : first_of(cb, base + 2);
    const size_t n_a = ca.size(), n_b = self ? ca.size() : cb.size();
    AlignSeedPlan p;
    align_seed_plan(fa.data(), n_a, fb.data(), n_b, self, min_run, p, tile_rows, chunk);
    // the seeds and the rows
    size_t s = 0;
    for (size_t a = 0; a < n_a; a++)
        for (uint32_t w = fa[a]; w < fa[a + 1]; w++)
            if ((w - fa[a]) % min_run == 0) {
                CHECK(s < p.n_seeds() && p.seed_window[s] == w && p.seed_video[s] == a, "seed %zu", s);
                s++;
            }
    CHECK(s == p.n_seeds() && p.seed_video.size() == p.seed_window.size(), "%zu seeds of %zu", s, p.n_seeds());
    CHECK(p.row_base == (n_b ? fb[0] : 0u) && p.n_rows == (n_b ? fb[n_b] - fb[0] : 0u) && p.row_video.size() == p.n_rows, "rows");
    for (size_t b = 0; b < n_b; b++)
        for (uint32_t w = fb[b]; w < fb[b + 1]; w++) CHECK(p.row_video[w - p.row_base] == b, "row %u", w);
    CHECK(p.n_tiles == (p.n_rows + tile_rows - 1) / tile_rows, "tiles");
    if (p.n_rows == 0 || p.n_seeds() == 0) {
        CHECK(p.n_units() == 0, "units without a cell");
        return;
    }
    CHECK(p.n_chunks() == (p.n_seeds() + chunk - 1) / chunk && p.unit_offset.size() == p.n_chunks() + 1 && p.unit_offset[0] == 0, "chunks");
    // the kernel's walk
    std::vector<uint8_t> visited(p.n_seeds() * (size_t)p.n_rows, 0);
    size_t groups = 0;
    for (const AlignLaunchCut &cut : align_launch_cuts((size_t)p.n_units(), max_groups)) {
        CHECK(cut.n >= 1 && cut.n <= max_groups && cut.group_base == groups, "cut");
        for (size_t g = 0; g < cut.n; g++) {
            const uint64_t unit = cut.group_base + g;
            const uint32_t c = align_seed_unit_chunk(p.unit_offset.data(), (uint32_t)p.n_chunks(), unit);
            CHECK(c < p.n_chunks() && p.unit_offset[c] <= unit && unit < p.unit_offset[c + 1], "unit %llu -> chunk %u", (unsigned long long)unit, c);
            const uint32_t tile = p.tile_first[c] + (uint32_t)(unit - p.unit_offset[c]);
            CHECK(tile < p.n_tiles, "unit %llu -> tile %u of %u", (unsigned long long)unit, tile, p.n_tiles);
            const size_t s0 = (size_t)c * chunk, s1 = std::min(s0 + chunk, p.n_seeds());
            CHECK(s0 < s1, "an empty chunk");
            const uint64_t r0 = (uint64_t)tile * tile_rows, r1 = std::min<uint64_t>(r0 + tile_rows, p.n_rows);  // the lanes behind n_rows form no address
            CHECK(r0 < r1, "an empty tile");
            for (size_t q = s0; q < s1; q++) {
                CHECK(p.seed_window[q] >= fa[0] && p.seed_window[q] < fa[n_a], "seed %zu reads window %u", q, p.seed_window[q]);
                for (uint64_t r = r0; r < r1; r++) {
                    CHECK(p.row_base + r >= fb[0] && p.row_base + r < fb[n_b], "row %llu", (unsigned long long)r);
                    CHECK(visited[q * p.n_rows + r] == 0, "cell (%zu, %llu) in two units", q, (unsigned long long)r);
                    visited[q * p.n_rows + r] = 1;
                }
            }
            (*units_seen)++;
        }
        groups += cut.n;
    }
    CHECK(groups == p.n_units(), "cuts cover %zu of %llu units", groups, (unsigned long long)p.n_units());
    for (size_t q = 0; q < p.n_seeds(); q++)
        for (uint32_t r = 0; r < p.n_rows; r++)
            if (!self || p.seed_video[q] < p.row_video[r]) {
                CHECK(visited[q * p.n_rows + r] == 1, "cell (seed %zu of video %u, row %u of video %u) in no unit", q, p.seed_video[q], r, p.row_video[r]);
                (*cells_seen)++;
            }
    // the triangle: no unit is kept whose largest row video is not above its smallest seed video
    if (self)
        for (size_t c = 0; c < p.n_chunks(); c++)
            for (uint32_t t = p.tile_first[c]; t < p.n_tiles; t++) {
                const uint32_t v_max = p.row_video[std::min<uint64_t>((uint64_t)(t + 1) * tile_rows, p.n_rows) - 1];
                CHECK(v_max > p.seed_video[c * chunk], "chunk %zu keeps tile %u without a cell", c, t);
            }
}

struct Pair { uint32_t a, b; };

static void replay_pair_lists(unsigned long long *pairs_seen)
{
    const std::vector<uint32_t> ca = {1, 2, 63, 64, 65, 0, 127, 128, 129, 200, 0, 5}, cb = {200, 0, 65, 1, 128, 64, 2};
    for (bool self : {false, true}) {
        const std::vector<uint32_t> fa = first_of(ca, 0), fb = self ? fa : first_of(cb, 0);
        const size_t n_a = ca.size(), n_b = self ? n_a : cb.size();
        for (uint32_t keep : {1u, 2u, 3u, 7u}) {  // every keep-th pair of the call
            std::vector<Pair> list;
            uint32_t k = 0;
            for (uint32_t a = 0; a < n_a; a++)
                for (uint32_t b = self ? a + 1 : 0; b < n_b; b++)
                    if (k++ % keep == 0) list.push_back({a, b});
            size_t bad = 0;
            CHECK(align_pair_list_check(list.data(), list.size(), n_a, n_b, self, &bad) == 0, "a good list refused at %zu", bad);
            for (size_t max_pairs : {(size_t)1, (size_t)5, kAlignChunkPairs})
                for (size_t max_units : {(size_t)1, (size_t)7, kAlignChunkUnits}) {
                    AlignChunk ch;
                    size_t cur = 0, at = 0;
                    while (align_next_chunk_pairs(fa.data(), fb.data(), list.data(), list.size(), cur, ch, max_pairs, max_units)) {
                        CHECK(!ch.pairs.empty() && ch.unit_offset.size() == ch.pairs.size() + 1 && ch.unit_offset[0] == 0, "chunk shape");
                        CHECK(ch.pairs.size() <= max_pairs && (ch.pairs.size() == 1 || ch.n_units() <= max_units), "chunk limits");
                        for (size_t i = 0; i < ch.pairs.size(); i++, at++) {
                            while (at < list.size() && !align_bands(fa[list[at].a + 1] - fa[list[at].a], fb[list[at].b + 1] - fb[list[at].b])) at++;
                            CHECK(at < list.size() && ch.pairs[i].a == list[at].a && ch.pairs[i].b == list[at].b, "pair %zu of the list", at);
                            const uint32_t bands = align_bands(fa[list[at].a + 1] - fa[list[at].a], fb[list[at].b + 1] - fb[list[at].b]);
                            CHECK(ch.unit_offset[i + 1] - ch.unit_offset[i] == bands, "units of pair %zu", at);
                            (*pairs_seen)++;
                        }
                    }
                    while (at < list.size() && !align_bands(fa[list[at].a + 1] - fa[list[at].a], fb[list[at].b + 1] - fb[list[at].b])) at++;
                    CHECK(at == list.size() && cur == list.size() && ch.pairs.empty(), "the chunks hold %zu of %zu pairs", at, list.size());
                }
        }
    }
    // the list check: the first offence, of every kind
    size_t at = 99;
    const Pair unsorted[] = {{0, 1}, {2, 3}, {2, 2}}, dup[] = {{0, 1}, {0, 1}}, back[] = {{1, 2}, {0, 3}}, range_a[] = {{0, 1}, {4, 0}}, range_b[] = {{0, 5}},
               diag[] = {{0, 1}, {2, 2}}, swapped[] = {{3, 1}}, fine[] = {{0, 0}, {0, 4}, {3, 0}, {3, 4}};
    CHECK(align_pair_list_check(unsorted, 3, 4, 5, false, &at) == 1 && at == 2, "unsorted");
    CHECK(align_pair_list_check(dup, 2, 4, 5, false, &at) == 1 && at == 1, "duplicate");
    CHECK(align_pair_list_check(back, 2, 4, 5, false, &at) == 1 && at == 1, "a goes back");
    CHECK(align_pair_list_check(range_a, 2, 4, 5, false, &at) == 2 && at == 1, "a out of range");
    CHECK(align_pair_list_check(range_b, 1, 4, 5, false, &at) == 2 && at == 0, "b out of range");
    CHECK(align_pair_list_check(range_b, 1, 6, 5, true, &at) == 0, "self mode: b counts against n_a");
    CHECK(align_pair_list_check(range_b, 1, 5, 9, true, &at) == 2, "self mode: b counts against n_a, not n_b");
    CHECK(align_pair_list_check(diag, 2, 4, 4, true, &at) == 3 && at == 1, "a == b in self mode");
    CHECK(align_pair_list_check(swapped, 1, 4, 4, true, &at) == 3 && at == 0, "a > b in self mode");
    CHECK(align_pair_list_check(swapped, 1, 4, 4, false, &at) == 0, "a > b between two sets");
    CHECK(align_pair_list_check(fine, 4, 4, 5, false, &at) == 0 && align_pair_list_check(fine, 0, 0, 0, true, &at) == 0, "good lists");
}

int main()
{
    unsigned long long cells = 0, units = 0, pairs = 0, plans = 0;
    const uint32_t sizes[][2] = {{2, 2}, {4, 3}, {3, 1}, {kSeedTileRows, kSeedChunk}};  // (rows per tile, seeds per chunk)
    for (uint32_t code = 0; code < 4096; code++) {  // three videos of 0 .. 3 windows per side
        const std::vector<uint32_t> ca = {code & 3, (code >> 2) & 3, (code >> 4) & 3}, cb = {(code >> 6) & 3, (code >> 8) & 3, (code >> 10) & 3};
        for (uint32_t min_run = 1; min_run <= 4; min_run++)
            for (const auto &sz : sizes) {
                replay_seed(ca, cb, false, min_run, sz[0], sz[1], code % 3 ? 0 : 5, code % 5 ? (size_t)1 << 23 : 2, &cells, &units);
                plans++;
            }
    }
    for (uint32_t code = 0; code < 1024; code++) {  // self mode: five videos of 0 .. 3 windows
        const std::vector<uint32_t> ca = {code & 3, (code >> 2) & 3, (code >> 4) & 3, (code >> 6) & 3, (code >> 8) & 3};
        for (uint32_t min_run = 1; min_run <= 4; min_run++)
            for (const auto &sz : sizes) {
                replay_seed(ca, {}, true, min_run, sz[0], sz[1], code % 3 ? 0 : 5, code % 5 ? (size_t)1 << 23 : 2, &cells, &units);
                plans++;
            }
    }
    // more than one tile and chunk of the kernel's own size, videos across their edges
    const std::vector<uint32_t> big_a = {0, 300, 1, 0, 700, 255, 513, 0}, big_b = {0, 511, 2, 0, 1025, 3, 0};
    for (uint32_t min_run : {1u, 2u, 7u, 2000u}) {
        replay_seed(big_a, big_b, false, min_run, kSeedTileRows, kSeedChunk, 3, (size_t)1 << 23, &cells, &units);
        replay_seed(big_a, {}, true, min_run, kSeedTileRows, kSeedChunk, 3, 3, &cells, &units);
        plans += 2;
    }
    replay_seed({}, {4}, false, 1, 4, 3, 0, 4, &cells, &units);
    replay_seed({4}, {}, false, 1, 4, 3, 0, 4, &cells, &units);
    replay_seed({4}, {}, true, 1, 4, 3, 0, 4, &cells, &units);
    replay_pair_lists(&pairs);
    // the early exit's dwords: exact whatever is picked, but the kernel is instantiated for these only
    for (uint32_t tol = 0; tol <= 1024; tol++) {
        const uint32_t w = align_seed_check_words(tol);
        CHECK(w == 14 || w == 22 || w == 26 || w == 32, "tol %u -> %u dwords", tol, w);
        if (tol) CHECK(w >= align_seed_check_words(tol - 1), "the exit moves forward as the tolerance grows");
    }
    CHECK(align_seed_check_words(0) == 14 && align_seed_check_words(350) == 26 && align_seed_check_words(1024) == 32, "early-exit dwords");
    std::printf("align seed plan ok: %llu plans, %llu cells in %llu units, %llu listed pairs\n", plans, cells, units, pairs);
    return 0;
}
