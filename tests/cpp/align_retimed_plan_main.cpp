// The planner of the retimed align calls (csrc/align_retimed_plan.h) replayed on the CPU, built with
// -fsanitize=address,undefined by tests/test_align_retimed_plan.py.  For every (Na, Nb) in 0 .. 140 x 0 .. 140 and seven rates every unit
// (phase, band) of the pair is walked step by step and lane by lane with the header's own functions - the kernel (csrc/align.hip:
// align_bands_kernel<AlignPairUnits<true>, false>) calls the same ones - on a synthetic distance function, and
//   - every cell of every phase's sub-matrix is visited exactly once, and nothing else;
//   - no row index behind a visited cell reaches Na or Nb;
//   - the band records, reduced by the header's two-level reduction, give the record of a brute-force twin that walks every diagonal of every
//     phase and ranks with tuples: inside a phase (score, offset, i0), across the phases (score, first_a, first_b);
//   - unit -> (phase, band) is a bijection onto the bands of the phases, phase-major.
// For lists of videos of mixed lengths: the chunks hold every pair with a unit once, in (a, b) order, within the pair and unit bounds, in the
// all-pairs form and fed from a pair list.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <tuple>
#include <vector>

#include "align_retimed_plan.h"

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

// distances 0 .. 7 with tolerance 3: about every second cell matches, and equal scores are everywhere
constexpr uint32_t kTol = 3;
static uint32_t dist_of(uint32_t ra, uint32_t rb, uint32_t salt)
{
    uint32_t x = ra * 2654435761u ^ (rb + 0x9E3779B9u) * 40503u ^ salt * 0x85EBCA6Bu;
    x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 12; x *= 0x297A2D39u; x ^= x >> 15;
    return x & 7u;
}

struct Record { uint32_t first_a, first_b, n, sum; bool any; };

// the twin: every diagonal of every phase, tuples
static Record twin(uint32_t Na, uint32_t Nb, uint32_t num, uint32_t den, uint32_t min_run, uint32_t salt)
{
    typedef std::tuple<int64_t, int64_t, int64_t> Key;
    bool any = false;
    Key best_key;
    Record best{0, 0, 0, 0, false};
    for (uint32_t p = 0; p < num && p < Na; p++) {
        const int64_t na = (Na - p + num - 1) / num, nb = (Nb + den - 1) / den;
        bool ph_any = false;
        Key ph_key;
        uint32_t ph_n = 0, ph_sum = 0;
        for (int64_t d = -(na - 1); d <= nb - 1; d++) {
            uint32_t len = 0, sum = 0;
            for (int64_t i = std::max<int64_t>(0, -d); i <= std::min<int64_t>(na, nb - d); i++) {
                const bool inside = i < std::min<int64_t>(na, nb - d);
                const uint32_t dd = inside ? dist_of((uint32_t)(p + num * i), (uint32_t)(den * (i + d)), salt) : 99u;
                if (dd <= kTol) { len++; sum += dd; continue; }
                if (len >= min_run) {
                    const Key k(-(int64_t)(len * (kTol + 1) - sum), d, i - len);
                    if (!ph_any || k < ph_key) { ph_any = true; ph_key = k; ph_n = len; ph_sum = sum; }
                }
                len = 0; sum = 0;
            }
        }
        if (!ph_any) continue;
        const int64_t i0 = std::get<2>(ph_key), off = std::get<1>(ph_key);
        const Key k(std::get<0>(ph_key), p + num * i0, den * (i0 + off));
        if (!any || k < best_key) { any = true; best_key = k; best = Record{(uint32_t)(p + num * i0), (uint32_t)(den * (i0 + off)), ph_n, ph_sum, true}; }
    }
    return best;
}

static void replay_pair(uint32_t Na, uint32_t Nb, uint32_t num, uint32_t den, unsigned long long *cells, unsigned long long *lane_steps, unsigned long long *records)
{
    const uint32_t min_run = 1 + (Na + Nb) % 3, salt = Na * 141 + Nb;
    const AlignRetimedSplit sp = align_retimed_split(Na, Nb, num, den);
    const uint32_t n_units = align_retimed_units(sp), nb0 = align_retimed_nb(Nb, den);
    CHECK(n_units == align_retimed_pair_units(Na, Nb, num, den), "units");
    // the units are the bands of the phases, phase-major
    uint32_t want_units = 0;
    std::vector<std::vector<uint32_t>> visited(num);
    for (uint32_t p = 0; p < num; p++) {
        const uint32_t na = align_retimed_na(Na, num, p);
        CHECK(na == (p < Na ? (Na - p + num - 1) / num : 0u), "Na_p");
        CHECK(align_retimed_phase_first(sp, p) == want_units && align_retimed_phase_units(sp, p) == align_bands(na, nb0), "Na %u Nb %u %u/%u phase %u", Na, Nb, num, den, p);
        want_units += align_bands(na, nb0);
        visited[p].assign((size_t)na * nb0, 0);
        if (na) CHECK(align_retimed_row_a(p, num, na - 1) < Na && align_retimed_row_a(p, num, na) >= Na, "the rows of phase %u", p);
    }
    CHECK(nb0 == (Nb + den - 1) / den && (nb0 == 0 || (align_retimed_row_b(den, nb0 - 1) < Nb && align_retimed_row_b(den, nb0) >= Nb)), "Nb_0");
    CHECK(n_units == want_units, "Na %u Nb %u %u/%u: %u units of %u", Na, Nb, num, den, n_units, want_units);

    std::vector<AlignBandRecord> band_records(n_units);
    for (uint32_t u = 0; u < n_units; u++) {
        uint32_t phase = ~0u, band = ~0u;
        align_retimed_unit(sp, u, &phase, &band);
        CHECK(phase < num, "unit %u: phase %u", u, phase);
        const uint32_t na = align_retimed_na(Na, num, phase);
        CHECK(band < align_bands(na, nb0) && align_retimed_phase_first(sp, phase) + band == u, "Na %u Nb %u %u/%u unit %u -> phase %u band %u", Na, Nb, num, den, u, phase, band);
        const int32_t d0 = align_band_d0(na, band);
        const uint32_t ka0 = align_ka_begin(d0), ka1 = align_ka_end(na, nb0, d0);
        CHECK(ka0 < ka1 && ka1 <= na, "steps %u .. %u", ka0, ka1);
        // the kernel's walk: lane state, lane bests
        int32_t row[kAlignBand];
        uint32_t len[kAlignBand] = {}, sum[kAlignBand] = {};
        uint32_t b_score[kAlignBand] = {}, b_start[kAlignBand] = {}, b_n[kAlignBand] = {}, b_sum[kAlignBand] = {};
        int32_t b_off[kAlignBand] = {};
        for (uint32_t lane = 0; lane < kAlignBand; lane++) row[lane] = align_lane_row(lane, ka0, d0);
        for (uint32_t ka = ka0; ka < ka1; ka++) {
            const uint32_t ra = align_retimed_row_a(phase, num, ka);
            CHECK(ra < Na, "Na %u %u/%u phase %u step %u: row %u of A", Na, num, den, phase, ka, ra);
            for (uint32_t lane = 0; lane < kAlignBand; lane++) {
                const int32_t kb = row[lane];
                const bool row_ok = kb >= 0 && kb < (int32_t)nb0;
                uint32_t d = 99;
                if (row_ok) {
                    const uint32_t rb = align_retimed_row_b(den, (uint32_t)kb);
                    CHECK(rb < Nb, "Nb %u %u/%u column %d: row %u of B", Nb, num, den, kb, rb);
                    d = dist_of(ra, rb, salt);
                    visited[phase][(size_t)ka * nb0 + (uint32_t)kb]++;
                    (*cells)++;
                }
                (*lane_steps)++;
                const bool match = row_ok && d <= kTol;
                if (match) { len[lane] += 1; sum[lane] += d; }
                const bool edge = ka + 1 == na || kb + 1 == (int32_t)nb0;
                const bool ends = len[lane] != 0 && (!match || edge);
                if (ends && len[lane] >= min_run) {
                    const uint32_t score = len[lane] * (kTol + 1) - sum[lane], start = (match ? ka + 1 : ka) - len[lane];
                    const int32_t off = kb - (int32_t)ka;
                    if (align_better(score, off, start, b_score[lane], b_off[lane], b_start[lane])) {
                        b_score[lane] = score; b_off[lane] = off; b_start[lane] = start; b_n[lane] = len[lane]; b_sum[lane] = sum[lane];
                    }
                }
                if (ends) { len[lane] = 0; sum[lane] = 0; }
            }
            uint32_t nlen[kAlignBand], nsum[kAlignBand];
            for (uint32_t lane = 0; lane < kAlignBand; lane++) { nlen[lane] = len[align_rotate_source(lane)]; nsum[lane] = sum[align_rotate_source(lane)]; }
            for (uint32_t lane = 0; lane < kAlignBand; lane++) { len[lane] = nlen[lane]; sum[lane] = nsum[lane]; }
            if (ka + 1 < ka1) {
                const uint32_t lane = align_reload_lane(ka, d0);
                row[lane] += (int32_t)kAlignBand;
                CHECK(row[lane] == align_reload_row(ka, d0), "reload");
            }
        }
        uint32_t w_score = 0, w_start = 0, w_n = 0, w_sum = 0;
        int32_t w_off = 0;
        for (uint32_t lane = 0; lane < kAlignBand; lane++)
            if (align_better(b_score[lane], b_off[lane], b_start[lane], w_score, w_off, w_start)) {
                w_score = b_score[lane]; w_off = b_off[lane]; w_start = b_start[lane]; w_n = b_n[lane]; w_sum = b_sum[lane];
            }
        band_records[u] = AlignBandRecord{w_off, w_start, w_score ? w_n : 0u, w_sum};
    }
    for (uint32_t p = 0; p < num; p++)
        for (size_t i = 0; i < visited[p].size(); i++) CHECK(visited[p][i] == 1, "Na %u Nb %u %u/%u phase %u: cell %zu visited %u times", Na, Nb, num, den, p, i, visited[p][i]);

    const AlignRetimedBest got = align_retimed_reduce(band_records.data(), sp, den, kTol);
    const Record want = twin(Na, Nb, num, den, min_run, salt);
    CHECK((got.score != 0) == want.any, "Na %u Nb %u %u/%u: a record on one side only", Na, Nb, num, den);
    if (want.any) {
        CHECK(got.first_a == want.first_a && got.first_b == want.first_b && got.n_windows == want.n && got.dist_sum == want.sum,
              "Na %u Nb %u %u/%u min_run %u: (%u, %u, %u, %u), the twin has (%u, %u, %u, %u)", Na, Nb, num, den, min_run, got.first_a, got.first_b, got.n_windows,
              got.dist_sum, want.first_a, want.first_b, want.n, want.sum);
        CHECK(got.score == want.n * (kTol + 1) - want.sum, "score");
        (*records)++;
    }
}

static void replay_lists(const std::vector<uint32_t> &ca, const std::vector<uint32_t> &cb, uint32_t num, uint32_t den, size_t max_pairs, size_t max_units,
                         bool listed, unsigned long long *units_seen)
{
    std::vector<uint32_t> fa(1, 0), fb(1, 0);
    for (uint32_t n : ca) fa.push_back(fa.back() + n);
    for (uint32_t n : cb) fb.push_back(fb.back() + n);
    std::vector<AlignPair> list, want;
    for (size_t a = 0; a < ca.size(); a++)
        for (size_t b = 0; b < cb.size(); b++) {
            if (listed && (a * 7 + b * 3) % 4 == 0) continue;  // a list leaves some pairs out
            list.push_back({(uint32_t)a, (uint32_t)b});
            if (align_retimed_pair_units(ca[a], cb[b], num, den)) want.push_back({(uint32_t)a, (uint32_t)b});
        }
    size_t at_list = 0;
    CHECK(align_pair_list_check(list.data(), list.size(), ca.size(), cb.size(), false, &at_list) == 0, "the list");
    AlignCursor cur;
    AlignChunk ch;
    size_t at = 0, list_at = 0;
    while (listed ? align_retimed_next_chunk_pairs(fa.data(), fb.data(), list.data(), list.size(), num, den, list_at, ch, max_pairs, max_units)
                  : align_retimed_next_chunk(fa.data(), ca.size(), fb.data(), cb.size(), num, den, cur, ch, max_pairs, max_units)) {
        CHECK(!ch.pairs.empty() && ch.unit_offset.size() == ch.pairs.size() + 1 && ch.unit_offset[0] == 0, "chunk shape");
        CHECK(ch.pairs.size() <= max_pairs, "chunk of %zu pairs", ch.pairs.size());
        CHECK(ch.pairs.size() == 1 || ch.n_units() <= max_units, "chunk of %zu units, bound %zu", ch.n_units(), max_units);
        for (size_t i = 0; i < ch.pairs.size(); i++, at++) {
            CHECK(at < want.size() && ch.pairs[i].a == want[at].a && ch.pairs[i].b == want[at].b, "pair %zu of the call", at);
            const uint32_t n = align_retimed_pair_units(ca[ch.pairs[i].a], cb[ch.pairs[i].b], num, den);
            CHECK(ch.unit_offset[i + 1] - ch.unit_offset[i] == n && n > 0, "units of pair %zu", at);
        }
        std::vector<uint32_t> hit(ch.n_units(), 0);
        for (const AlignLaunchCut &cut : align_launch_cuts(ch.n_groups(), 3))
            for (size_t g = 0; g < cut.n; g++)
                for (uint32_t w = 0; w < kAlignWaves; w++) {
                    const size_t unit = (g + cut.group_base) * kAlignWaves + w;
                    if (unit >= ch.n_units()) continue;  // the kernel's exit
                    const uint32_t p = align_unit_pair(ch.unit_offset.data(), (uint32_t)ch.pairs.size(), (uint32_t)unit);
                    CHECK(p < ch.pairs.size() && ch.unit_offset[p] <= unit && unit < ch.unit_offset[p + 1], "unit %zu -> pair %u", unit, p);
                    uint32_t phase, band;
                    const AlignRetimedSplit sp = align_retimed_split(ca[ch.pairs[p].a], cb[ch.pairs[p].b], num, den);
                    align_retimed_unit(sp, (uint32_t)unit - ch.unit_offset[p], &phase, &band);
                    CHECK(phase < num && band < align_retimed_phase_units(sp, phase), "unit %zu -> phase %u band %u", unit, phase, band);
                    hit[unit]++;
                    (*units_seen)++;
                }
        for (uint32_t h : hit) CHECK(h == 1, "a unit reached %u times", h);
    }
    CHECK(at == want.size() && ch.pairs.empty(), "the chunks hold %zu of %zu pairs", at, want.size());
}

int main()
{
    const uint32_t rates[7][2] = {{1, 1}, {2, 1}, {3, 2}, {5, 4}, {6, 5}, {31, 16}, {32, 17}};
    unsigned long long cells = 0, lane_steps = 0, want_cells = 0, records = 0, units = 0;
    // 7 rates x 4 residues of Na: 28 tasks on up to 8 threads (the walk is 300 M cells under two sanitizers)
    std::atomic<uint32_t> next_task{0};
    std::mutex sum_mu;
    const auto worker = [&]() {
        for (uint32_t task = next_task++; task < 28; task = next_task++) {
            const uint32_t *r = rates[task / 4];
            uint32_t num = 0, den = 0;
            CHECK(align_retimed_rate(r[0], r[1], &num, &den) == 0 && num == r[0] && den == r[1], "rate %u/%u", r[0], r[1]);
            unsigned long long c = 0, l = 0, w = 0, n = 0;
            for (uint32_t Na = task % 4; Na <= 140; Na += 4)
                for (uint32_t Nb = 0; Nb <= 140; Nb++) {
                    replay_pair(Na, Nb, num, den, &c, &l, &n);
                    w += (unsigned long long)Na * ((Nb + den - 1) / den);  // the phases partition the rows of A
                }
            std::lock_guard<std::mutex> lk(sum_mu);
            cells += c; lane_steps += l; want_cells += w; records += n;
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < std::min(8u, std::max(1u, std::thread::hardware_concurrency())); t++) pool.emplace_back(worker);
    worker();
    for (std::thread &t : pool) t.join();
    CHECK(cells == want_cells, "%llu cells of %llu", cells, want_cells);
    uint32_t num = 0, den = 0;
    CHECK(align_retimed_rate(64, 34, &num, &den) == 0 && num == 32 && den == 17, "64/34");
    CHECK(align_retimed_rate(12, 10, &num, &den) == 0 && num == 6 && den == 5, "12/10");
    CHECK(align_retimed_rate(6, 0, &num, &den) == 1 && align_retimed_rate(0, 0, &num, &den) == 1 && align_retimed_rate(4, 5, &num, &den) == 1 &&
              align_retimed_rate(11, 5, &num, &den) == 1 && align_retimed_rate(0xFFFFFFFFu, 0x80000000u, &num, &den) == 2 && align_retimed_rate(0xFFFFFFFFu, 0x7FFFFFFFu, &num, &den) == 1,
          "rates outside the range");
    CHECK(align_retimed_rate(33, 32, &num, &den) == 2 && align_retimed_rate(33, 17, &num, &den) == 2 && align_retimed_rate(66, 64, &num, &den) == 2, "num above 32");
    // the largest pair a call takes: its units fit the unit offsets by far
    CHECK(align_retimed_pair_units(kAlignMaxWindows, kAlignMaxWindows, 32, 17) < (1u << 20) && align_retimed_pair_units(kAlignMaxWindows, kAlignMaxWindows, 1, 1) == (1u << 15),
          "units of the largest pair");
    const std::vector<uint32_t> ca = {1, 2, 63, 64, 65, 0, 127, 128, 129, 200, 0, 5, 400}, cb = {200, 0, 65, 1, 128, 64, 2, 390};
    for (const auto &r : rates)
        for (bool listed : {false, true})
            for (size_t max_pairs : {(size_t)1, (size_t)5, kAlignChunkPairs})
                for (size_t max_units : {(size_t)1, (size_t)7, (size_t)40, kAlignChunkUnits}) replay_lists(ca, cb, r[0], r[1], max_pairs, max_units, listed, &units);
    replay_lists({}, cb, 3, 2, 4, 4, false, &units);
    replay_lists(ca, {}, 3, 2, 4, 4, false, &units);
    replay_lists({0, 0}, {0}, 6, 5, 4, 4, true, &units);
    std::printf("align retimed plan ok: %llu cells in %llu lane steps, %llu records, %llu units\n", cells, lane_steps, records, units);
    return 0;
}
