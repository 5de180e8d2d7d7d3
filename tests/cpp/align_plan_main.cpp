// The planner and the lane-ownership rules of the align kernel (csrc/align_plan.h) replayed on the CPU, built with
// -fsanitize=address,undefined by tests/test_align_plan.py.  For every (Na, Nb) in 0 .. 140 x 0 .. 140: the bands of the pair are walked step
// by step with the header's own functions - the kernel (csrc/align.hip) calls the same ones - and
//   - every cell of the matrix is visited by exactly one (band, lane, step), no band walks a ka outside its range, no band is empty;
//   - at every step every lane holds the row the header says it holds, and after the rotation every diagonal's state sits in the lane
//     that works on the diagonal's next cell;
//   - a band loads each row it needs exactly once and no row outside [0, Nb).
// For pair lists of mixed lengths in both modes: the chunks hold every pair with a band once, in (a, b) order, within their limits; every
// (workgroup, wave) of every launch cut maps to exactly one (pair, band) and back.
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

static void replay_pair(uint32_t Na, uint32_t Nb, unsigned long long *cells, unsigned long long *steps)
{
    const uint32_t bands = align_bands(Na, Nb);
    CHECK((bands == 0) == (Na == 0 || Nb == 0), "Na %u Nb %u", Na, Nb);
    if (bands) CHECK(bands == (Na + Nb - 1 + 63) / 64, "Na %u Nb %u", Na, Nb);
    std::vector<uint32_t> visited((size_t)Na * Nb, 0);
    for (uint32_t band = 0; band < bands; band++) {
        const int32_t d0 = align_band_d0(Na, band);
        const uint32_t ka0 = align_ka_begin(d0), ka1 = align_ka_end(Na, Nb, d0);
        CHECK(ka0 < ka1 && ka1 <= Na, "Na %u Nb %u band %u: steps %u .. %u", Na, Nb, band, ka0, ka1);
        CHECK(d0 >= -(int32_t)(Na - 1) && d0 <= (int32_t)Nb - 1, "band %u begins outside the diagonals", band);
        // the range is tight: the first and the last step hold a cell of the matrix
        bool first_has = false, last_has = false;
        std::vector<uint32_t> loaded(Nb, 0);
        int32_t row[kAlignBand];    // the row a lane holds
        int32_t state[kAlignBand];  // the diagonal whose run state sits in the lane
        for (uint32_t lane = 0; lane < kAlignBand; lane++) {
            row[lane] = align_lane_row(lane, ka0, d0);
            CHECK(align_row_lane(row[lane]) == lane, "lane %u holds row %d", lane, row[lane]);
            state[lane] = row[lane] - (int32_t)ka0;
            if (row[lane] >= 0 && row[lane] < (int32_t)Nb) loaded[row[lane]]++;
        }
        for (uint32_t ka = ka0; ka < ka1; ka++) {
            bool seen[kAlignBand] = {};
            for (uint32_t lane = 0; lane < kAlignBand; lane++) {
                const int32_t kb = row[lane], d = kb - (int32_t)ka;
                CHECK(kb == align_lane_row(lane, ka, d0), "Na %u Nb %u band %u step %u lane %u: row %d", Na, Nb, band, ka, lane, kb);
                CHECK(d >= d0 && d < d0 + (int32_t)kAlignBand && !seen[d - d0], "step %u lane %u: diagonal %d", ka, lane, d);
                seen[d - d0] = true;
                CHECK(state[lane] == d && align_state_lane(d, ka) == lane, "Na %u Nb %u band %u step %u lane %u: state of diagonal %d, works on %d", Na, Nb,
                      band, ka, lane, state[lane], d);
                if (kb >= 0 && kb < (int32_t)Nb) {
                    CHECK(loaded[kb] == 1, "row %d used with %u loads", kb, loaded[kb]);
                    visited[(size_t)ka * Nb + kb]++;
                    (*cells)++;
                    if (ka == ka0) first_has = true;
                    if (ka + 1 == ka1) last_has = true;
                }
            }
            (*steps)++;
            int32_t next[kAlignBand];
            for (uint32_t lane = 0; lane < kAlignBand; lane++) next[lane] = state[align_rotate_source(lane)];
            for (uint32_t lane = 0; lane < kAlignBand; lane++) state[lane] = next[lane];
            if (ka + 1 < ka1) {
                const uint32_t lane = align_reload_lane(ka, d0);
                CHECK(row[lane] == (int32_t)ka + d0, "step %u: lane %u reloads but holds row %d", ka, lane, row[lane]);
                row[lane] = align_reload_row(ka, d0);
                CHECK(row[lane] >= 1 && align_row_lane(row[lane]) == lane, "step %u: reloaded row %d", ka, row[lane]);
                if (row[lane] < (int32_t)Nb) loaded[row[lane]]++;
            }
        }
        CHECK(first_has && last_has, "Na %u Nb %u band %u walks an empty step", Na, Nb, band);
        // each row with a cell in the band was loaded once, no other row at all
        for (uint32_t kb = 0; kb < Nb; kb++) {
            bool needed = false;
            for (uint32_t ka = ka0; ka < ka1 && !needed; ka++) needed = (int32_t)kb - (int32_t)ka >= d0 && (int32_t)kb - (int32_t)ka < d0 + (int32_t)kAlignBand;
            CHECK(loaded[kb] == (needed ? 1u : 0u), "Na %u Nb %u band %u: row %u loaded %u times, needed %d", Na, Nb, band, kb, loaded[kb], (int)needed);
        }
    }
    for (size_t i = 0; i < visited.size(); i++) CHECK(visited[i] == 1, "Na %u Nb %u: cell (%zu, %zu) visited %u times", Na, Nb, i / Nb, i % Nb, visited[i]);
}

static void replay_lists(const std::vector<uint32_t> &ca, const std::vector<uint32_t> &cb, bool self, size_t max_pairs, size_t max_units, size_t max_groups,
                         unsigned long long *units_seen)
{
    std::vector<uint32_t> fa(1, 0), fb(1, 0);
    for (uint32_t n : ca) fa.push_back(fa.back() + n);
    for (uint32_t n : (self ? ca : cb)) fb.push_back(fb.back() + n);
    const size_t n_a = ca.size(), n_b = self ? ca.size() : cb.size();
    // what the chunks must hold, in order
    std::vector<AlignPair> want;
    for (size_t a = 0; a < n_a; a++)
        for (size_t b = self ? a + 1 : 0; b < n_b; b++)
            if (align_bands(fa[a + 1] - fa[a], fb[b + 1] - fb[b])) want.push_back({(uint32_t)a, (uint32_t)b});
    CHECK(want.size() <= align_pair_count(n_a, n_b, self), "pair count");
    AlignCursor cur;
    AlignChunk ch;
    size_t at = 0;
    while (align_next_chunk(fa.data(), n_a, fb.data(), n_b, self, cur, ch, max_pairs, max_units)) {
        CHECK(!ch.pairs.empty() && ch.unit_offset.size() == ch.pairs.size() + 1 && ch.unit_offset[0] == 0, "chunk shape");
        CHECK(ch.pairs.size() <= max_pairs, "chunk of %zu pairs", ch.pairs.size());
        CHECK(ch.pairs.size() == 1 || ch.n_units() <= max_units, "chunk of %zu units", ch.n_units());
        for (size_t i = 0; i < ch.pairs.size(); i++, at++) {
            CHECK(at < want.size() && ch.pairs[i].a == want[at].a && ch.pairs[i].b == want[at].b, "pair %zu of the call", at);
            const uint32_t bands = align_bands(fa[ch.pairs[i].a + 1] - fa[ch.pairs[i].a], fb[ch.pairs[i].b + 1] - fb[ch.pairs[i].b]);
            CHECK(ch.unit_offset[i + 1] - ch.unit_offset[i] == bands && bands > 0, "units of pair %zu", at);
        }
        // every (workgroup, wave) of every cut is one unit, every unit is reached once
        std::vector<uint32_t> hit(ch.n_units(), 0);
        size_t groups = 0;
        for (const AlignLaunchCut &cut : align_launch_cuts(ch.n_groups(), max_groups)) {
            CHECK(cut.n >= 1 && cut.n <= max_groups && cut.group_base == groups, "cut");
            for (size_t g = 0; g < cut.n; g++)
                for (uint32_t w = 0; w < kAlignWaves; w++) {
                    const size_t unit = (g + cut.group_base) * kAlignWaves + w;
                    if (unit >= ch.n_units()) continue;  // the kernel's exit
                    const uint32_t p = align_unit_pair(ch.unit_offset.data(), (uint32_t)ch.pairs.size(), (uint32_t)unit);
                    CHECK(p < ch.pairs.size() && ch.unit_offset[p] <= unit && unit < ch.unit_offset[p + 1], "unit %zu -> pair %u", unit, p);
                    hit[unit]++;
                    (*units_seen)++;
                }
            groups += cut.n;
        }
        CHECK(groups == ch.n_groups(), "cuts cover %zu of %zu groups", groups, ch.n_groups());
        for (uint32_t h : hit) CHECK(h == 1, "a unit reached %u times", h);
    }
    CHECK(at == want.size() && ch.pairs.empty(), "the chunks hold %zu of %zu pairs", at, want.size());
}

int main()
{
    unsigned long long cells = 0, steps = 0, want_cells = 0, units = 0;
    for (uint32_t Na = 0; Na <= 140; Na++)
        for (uint32_t Nb = 0; Nb <= 140; Nb++) {
            replay_pair(Na, Nb, &cells, &steps);
            want_cells += (unsigned long long)Na * Nb;
        }
    for (uint32_t n : {199u, 200u, 257u}) { replay_pair(n, 3, &cells, &steps); replay_pair(3, n, &cells, &steps); want_cells += 6ull * n; }
    CHECK(cells == want_cells, "%llu cells of %llu", cells, want_cells);
    const std::vector<uint32_t> ca = {1, 2, 63, 64, 65, 0, 127, 128, 129, 200, 0, 5}, cb = {200, 0, 65, 1, 128, 64, 2};
    for (bool self : {false, true})
        for (size_t max_pairs : {(size_t)1, (size_t)5, kAlignChunkPairs})
            for (size_t max_units : {(size_t)1, (size_t)7, kAlignChunkUnits})
                for (size_t max_groups : {(size_t)1, (size_t)3, kAlignMaxGroupsPerLaunch}) replay_lists(ca, cb, self, max_pairs, max_units, max_groups, &units);
    replay_lists({}, cb, false, 4, 4, 4, &units);
    replay_lists(ca, {}, false, 4, 4, 4, &units);
    replay_lists({7}, {}, true, 4, 4, 4, &units);
    replay_lists({0, 0}, {0}, false, 4, 4, 4, &units);
    CHECK(align_pair_count(5, 7, false) == 35 && align_pair_count(5, 5, true) == 10 && align_pair_count(0, 0, true) == 0 && align_pair_count(1, 1, true) == 0, "pair counts");
    std::printf("align plan ok: %llu cells in %llu steps, %llu units\n", cells, steps, units);
    return 0;
}
