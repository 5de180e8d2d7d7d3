// The planner of the align call over (rate, a, b) triples (csrc/align_rates_plan.h) replayed on the CPU, built with
// -fsanitize=address,undefined by tests/test_align_rates_plan.py.  One call: 71 videos of A against 71 of B, 0 .. 70 windows each, with all of
// 1/1, 2/1, 3/2, 5/4, 6/5, 31/16 and 32/17 in ONE rate list, the window counts of A another permutation of 0 .. 70 in every rate's block, every
// block of A some rows into its rows, and the hashes cut off in front as a host-array call cuts them (so that a slot's row0 wraps).  Every unit
// of every chunk is walked step by step and lane by lane as the kernel walks it (csrc/align.hip: align_bands_kernel<AlignTripleUnits, false>) - the triple from
// unit_offset, the slot from the triple, num / den / row0 / the row of a_first from the table - on a synthetic distance of the ABSOLUTE rows, and
//   - every cell of every phase of every triple is visited exactly once;
//   - no row is at or behind Na or Nb of the triple's own block;
//   - the absolute row of A is a_rate_first[r] + a_first[r][a] + k - a_shift, worked out here without the table;
//   - the band records, reduced by align_retimed_reduce with the triple's split and den, equal a brute-force twin's record;
//   - the chunks hold every triple with a unit once, in (rate, a, b) order, inside both bounds - with small max_pairs and max_units given so
//     that chunks close inside a rate and across a rate boundary - in the all-triples form, under exclude_same, and fed from a list.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <tuple>
#include <vector>

#include "align_rates_plan.h"

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
constexpr uint32_t kTol = 3, kMinRun = 2;
static uint32_t dist_of(uint32_t row_a, uint32_t row_b)
{
    uint32_t x = row_a * 2654435761u ^ (row_b + 0x9E3779B9u) * 40503u;
    x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 12; x *= 0x297A2D39u; x ^= x >> 15;
    return x & 7u;
}

constexpr uint32_t kRates = 7, kVideos = 71;
static const AlignSeedRate kRateList[kRates] = {{1, 1}, {2, 1}, {3, 2}, {5, 4}, {6, 5}, {31, 16}, {32, 17}};

struct Call {
    std::vector<uint32_t> first_a;   // [kRates][kVideos + 1]
    std::vector<size_t> rate_first;  // [kRates + 1]
    std::vector<uint32_t> first_b;   // [kVideos + 1]
    uint64_t a_shift;
    AlignRatesTable table;
    uint32_t na(uint32_t r, uint32_t a) const { return first_a[r * (kVideos + 1) + a + 1] - first_a[r * (kVideos + 1) + a]; }
    uint32_t nb(uint32_t b) const { return first_b[b + 1] - first_b[b]; }
    // absolute rows, without the table: what the kernel's addresses must come to
    uint32_t row_a(uint32_t r, uint32_t a, uint32_t k) const { return (uint32_t)(rate_first[r] + first_a[r * (kVideos + 1) + a] + k - a_shift); }
    uint32_t row_b(uint32_t b, uint32_t k) const { return first_b[b] + k; }
};

static Call make_call()
{
    Call c;
    c.first_a.assign(kRates * (kVideos + 1), 0);
    c.rate_first.assign(kRates + 1, 0);
    for (uint32_t r = 0; r < kRates; r++) {
        uint32_t *f = c.first_a.data() + r * (kVideos + 1);
        f[0] = 3 + r;  // the block begins some rows into its rows
        for (uint32_t v = 0; v < kVideos; v++) f[v + 1] = f[v] + (v * (2 * r + 1) + 5 * r) % kVideos;  // a permutation of 0 .. 70, another per rate
        c.rate_first[r + 1] = c.rate_first[r] + f[kVideos] + 2;
    }
    for (uint32_t r = 0; r < kRates; r++) c.rate_first[r] += 11;  // and the first block some rows into the array
    c.first_b.assign(kVideos + 1, 4);
    for (uint32_t v = 0; v < kVideos; v++) c.first_b[v + 1] = c.first_b[v] + v;
    c.a_shift = c.rate_first[0] + c.first_a[0];  // the smallest row any block uses: row0 of slot 0 wraps below zero
    c.table = align_rates_table(kRateList, kRates, c.rate_first.data(), kVideos, c.a_shift);
    return c;
}

struct Record { uint32_t first_a, first_b, n, sum; bool any; };

// the twin: every diagonal of every phase of the triple, tuples, on the absolute rows
static Record twin(const Call &c, uint32_t r, uint32_t a, uint32_t b)
{
    typedef std::tuple<int64_t, int64_t, int64_t> Key;
    const uint32_t num = kRateList[r].num, den = kRateList[r].den, Na = c.na(r, a), Nb = c.nb(b);
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
                const uint32_t dd = inside ? dist_of(c.row_a(r, a, (uint32_t)(p + num * i)), c.row_b(b, (uint32_t)(den * (i + d)))) : 99u;
                if (dd <= kTol) { len++; sum += dd; continue; }
                if (len >= kMinRun) {
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

// one unit of a chunk as the kernel walks it; cells[] counts the visits of the triple's cells, phase-major
static AlignBandRecord walk_unit(const Call &c, const AlignRatesChunk &ch, uint32_t unit, std::vector<std::vector<uint32_t>> &visits, unsigned long long *cells)
{
    const uint32_t t = align_unit_pair(ch.unit_offset.data(), (uint32_t)ch.n_triples(), unit);
    CHECK(t < ch.n_triples() && ch.unit_offset[t] <= unit && unit < ch.unit_offset[t + 1], "unit %u -> triple %u", unit, t);
    const uint32_t va = ch.triple(t).a, vb = ch.triple(t).b, slot = ch.triple(t).rate;
    CHECK(slot < kAlignRatesMax, "slot %u", slot);
    const AlignRatesSlot sl = c.table.slot[slot];
    const uint32_t *af = c.first_a.data() + sl.first_at;
    const uint32_t fa = sl.row0 + af[va], Na_all = af[va + 1] - af[va];  // 32-bit sum, as the kernel forms it
    const uint32_t fb = c.first_b[vb], Nb_all = c.first_b[vb + 1] - fb;
    CHECK(sl.num == kRateList[slot].num && sl.den == kRateList[slot].den && Na_all == c.na(slot, va) && Nb_all == c.nb(vb), "the slot of triple %u", t);
    CHECK(fa == c.row_a(slot, va, 0), "triple (%u, %u, %u): first row %u of A, not %u", slot, va, vb, fa, c.row_a(slot, va, 0));
    uint32_t phase = ~0u, band = ~0u;
    const AlignRetimedSplit sp = align_retimed_split(Na_all, Nb_all, sl.num, sl.den);
    align_retimed_unit(sp, unit - ch.unit_offset[t], &phase, &band);
    CHECK(phase < sl.num && band < align_retimed_phase_units(sp, phase), "unit %u -> phase %u band %u", unit, phase, band);
    const uint32_t Na = align_retimed_na(Na_all, sl.num, phase), Nb = align_retimed_nb(Nb_all, sl.den);
    const int32_t d0 = align_band_d0(Na, band);
    const uint32_t ka0 = align_ka_begin(d0), ka1 = align_ka_end(Na, Nb, d0);
    CHECK(ka0 < ka1 && ka1 <= Na, "steps %u .. %u", ka0, ka1);
    std::vector<uint32_t> &seen = visits[t];
    const size_t cell0 = [&]() { size_t n = 0; for (uint32_t p = 0; p < phase; p++) n += (size_t)align_retimed_na(Na_all, sl.num, p) * Nb; return n; }();
    int32_t row[kAlignBand];
    uint32_t len[kAlignBand] = {}, sum[kAlignBand] = {};
    uint32_t b_score[kAlignBand] = {}, b_start[kAlignBand] = {}, b_n[kAlignBand] = {}, b_sum[kAlignBand] = {};
    int32_t b_off[kAlignBand] = {};
    for (uint32_t lane = 0; lane < kAlignBand; lane++) row[lane] = align_lane_row(lane, ka0, d0);
    for (uint32_t ka = ka0; ka < ka1; ka++) {
        const uint32_t ra = align_retimed_row_a(phase, sl.num, ka);
        CHECK(ra < Na_all, "triple (%u, %u, %u) phase %u step %u: row %u of A at or behind %u", slot, va, vb, phase, ka, ra, Na_all);
        for (uint32_t lane = 0; lane < kAlignBand; lane++) {
            const int32_t kb = row[lane];
            const bool row_ok = kb >= 0 && kb < (int32_t)Nb;
            uint32_t d = 99;
            if (row_ok) {
                const uint32_t rb = align_retimed_row_b(sl.den, (uint32_t)kb);
                CHECK(rb < Nb_all, "triple (%u, %u, %u) column %d: row %u of B at or behind %u", slot, va, vb, kb, rb, Nb_all);
                d = dist_of(fa + ra, fb + rb);
                seen[cell0 + (size_t)ka * Nb + (uint32_t)kb]++;
                (*cells)++;
            }
            const bool match = row_ok && d <= kTol;
            if (match) { len[lane] += 1; sum[lane] += d; }
            const bool edge = ka + 1 == Na || kb + 1 == (int32_t)Nb;
            const bool ends = len[lane] != 0 && (!match || edge);
            if (ends && len[lane] >= kMinRun) {
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
    return AlignBandRecord{w_off, w_start, w_score ? w_n : 0u, w_sum};
}

// every unit of one chunk through the launch cuts, then the reduction of every triple against the twin
static void walk_chunk(const Call &c, const AlignRatesChunk &ch, unsigned long long *cells, unsigned long long *records)
{
    std::vector<std::vector<uint32_t>> visits(ch.n_triples());
    for (size_t t = 0; t < ch.n_triples(); t++) visits[t].assign((size_t)c.na(ch.triple(t).rate, ch.triple(t).a) * align_retimed_nb(c.nb(ch.triple(t).b), kRateList[ch.triple(t).rate].den), 0);
    std::vector<AlignBandRecord> band_records(ch.n_units());
    std::vector<uint32_t> hit(ch.n_units(), 0);
    for (const AlignLaunchCut &cut : align_launch_cuts(ch.n_groups(), 97))
        for (size_t g = 0; g < cut.n; g++)
            for (uint32_t w = 0; w < kAlignWaves; w++) {
                const size_t unit = (g + cut.group_base) * kAlignWaves + w;
                if (unit >= ch.n_units()) continue;  // the kernel's exit
                band_records[unit] = walk_unit(c, ch, (uint32_t)unit, visits, cells);
                hit[unit]++;
            }
    for (uint32_t h : hit) CHECK(h == 1, "a unit reached %u times", h);
    for (size_t t = 0; t < ch.n_triples(); t++) {
        const AlignRatesTriple tr = ch.triple(t);
        for (size_t i = 0; i < visits[t].size(); i++) CHECK(visits[t][i] == 1, "triple (%u, %u, %u): cell %zu visited %u times", tr.rate, tr.a, tr.b, i, visits[t][i]);
        const AlignRetimedSplit sp = align_retimed_split(c.na(tr.rate, tr.a), c.nb(tr.b), kRateList[tr.rate].num, kRateList[tr.rate].den);
        CHECK(ch.unit_offset[t + 1] - ch.unit_offset[t] == align_retimed_units(sp), "units of triple %zu", t);
        const AlignRetimedBest got = align_retimed_reduce(band_records.data() + ch.unit_offset[t], sp, kRateList[tr.rate].den, kTol);
        const Record want = twin(c, tr.rate, tr.a, tr.b);
        CHECK((got.score != 0) == want.any, "triple (%u, %u, %u): a record on one side only", tr.rate, tr.a, tr.b);
        if (want.any) {
            CHECK(got.first_a == want.first_a && got.first_b == want.first_b && got.n_windows == want.n && got.dist_sum == want.sum,
                  "triple (%u, %u, %u): (%u, %u, %u, %u), the twin has (%u, %u, %u, %u)", tr.rate, tr.a, tr.b, got.first_a, got.first_b, got.n_windows, got.dist_sum,
                  want.first_a, want.first_b, want.n, want.sum);
            (*records)++;
        }
    }
}

// the chunks of one form of the call: order, bounds, and where they close; walk: also every unit lane by lane (on up to 8 threads)
struct Closes { bool inside_rate = false, across_rates = false; size_t chunks = 0, triples = 0; };
static Closes replay_chunks(const Call &c, size_t max_pairs, size_t max_units, bool exclude_same, bool listed, bool walk, unsigned long long *cells, unsigned long long *records)
{
    std::vector<AlignRatesTriple> list, want;
    for (uint32_t r = 0; r < kRates; r++)
        for (uint32_t a = 0; a < kVideos; a++)
            for (uint32_t b = 0; b < kVideos; b++) {
                if (exclude_same && a == b) continue;
                if (listed && (a * 7 + b * 3 + r) % 4 == 0) continue;  // a list leaves some triples out
                list.push_back({a, b, r});
                if (align_rates_triple_units(c.first_a.data(), kVideos, c.first_b.data(), kRateList, r, a, b)) want.push_back({a, b, r});
            }
    size_t bad = 0;
    CHECK(align_rates_list_check(list.data(), list.size(), kVideos, kVideos, kRates, &bad) == 0, "the list");
    std::vector<AlignRatesChunk> chunks;
    AlignRatesCursor cur;
    AlignRatesChunk ch;
    size_t at = 0, list_at = 0;
    Closes cl;
    uint32_t last_rate = ~0u;
    while (listed ? align_rates_next_chunk_triples(c.first_a.data(), kVideos, c.first_b.data(), list.data(), list.size(), kRateList, list_at, ch, max_pairs, max_units)
                  : align_rates_next_chunk(c.first_a.data(), kVideos, c.first_b.data(), kVideos, kRateList, kRates, exclude_same, cur, ch, max_pairs, max_units)) {
        CHECK(!ch.empty() && ch.unit_offset.size() == ch.n_triples() + 1 && ch.unit_offset[0] == 0, "chunk shape");
        {   // sealed, the chunk is its upload - table | triples | unit_offset - and still reads as before
            AlignRatesChunk sealed = ch;
            const uint32_t *up = static_cast<const uint32_t *>(sealed.seal(c.table));
            const size_t n = ch.n_triples();
            CHECK(sealed.n_triples() == n && sealed.plan.size() * 4 == align_rates_plan_bytes(n) && up[0] == c.table.slot[0].num && up[3] == c.table.slot[0].first_at, "sealed shape");
            CHECK(up[align_rates_plan_triples_at() / 4 + 2] == ch.triple(0).rate && up[align_rates_plan_offsets_at(n) / 4 + n] == ch.n_units() &&
                      sealed.triple(n - 1).b == ch.triple(n - 1).b && sealed.seal(c.table) == up, "sealed contents");
        }
        CHECK(ch.n_triples() <= max_pairs, "chunk of %zu triples", ch.n_triples());
        CHECK(ch.n_triples() == 1 || ch.n_units() <= max_units, "chunk of %zu units, bound %zu", ch.n_units(), max_units);
        if (ch.triple(0).rate == last_rate) cl.inside_rate = true;                 // the chunk before closed inside this rate
        if (ch.triple(0).rate != ch.triple(ch.n_triples() - 1).rate) cl.across_rates = true;   // this chunk spans a rate boundary
        last_rate = ch.triple(ch.n_triples() - 1).rate;
        for (size_t i = 0; i < ch.n_triples(); i++, at++) {
            CHECK(at < want.size() && ch.triple(i).a == want[at].a && ch.triple(i).b == want[at].b && ch.triple(i).rate == want[at].rate, "triple %zu of the call", at);
            const uint32_t n = align_rates_triple_units(c.first_a.data(), kVideos, c.first_b.data(), kRateList, ch.triple(i).rate, ch.triple(i).a, ch.triple(i).b);
            CHECK(ch.unit_offset[i + 1] - ch.unit_offset[i] == n && n > 0, "units of triple %zu", at);
        }
        CHECK(align_rates_scratch_bytes(ch.n_triples(), ch.n_units()) >= ch.n_units() * 16 + ch.n_triples() * 64 + ((ch.n_triples() + 255) / 256 * 2 + 1) * 4,
              "scratch");
        CHECK(align_rates_plan_bytes(ch.n_triples()) == 128 + ch.n_triples() * 12 + (ch.n_triples() + 1) * 4, "plan bytes");
        cl.chunks++;
        if (walk) chunks.push_back(ch);
    }
    CHECK(at == want.size() && ch.empty(), "the chunks hold %zu of %zu triples", at, want.size());
    cl.triples = at;
    if (walk) {
        std::atomic<size_t> next{0};
        std::mutex mu;
        const auto worker = [&]() {
            unsigned long long cc = 0, rr = 0;
            for (size_t i = next++; i < chunks.size(); i = next++) walk_chunk(c, chunks[i], &cc, &rr);
            std::lock_guard<std::mutex> lk(mu);
            *cells += cc; *records += rr;
        };
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < std::min(8u, std::max(1u, std::thread::hardware_concurrency())); t++) pool.emplace_back(worker);
        worker();
        for (std::thread &t : pool) t.join();
    }
    return cl;
}

int main()
{
    const Call c = make_call();
    CHECK(c.table.slot[0].row0 > 0xFFFFFF00u && c.table.slot[1].row0 < 0x10000u, "row0 of slot 0 wraps, the others do not");
    for (uint32_t r = 0; r < kRates; r++) {
        std::vector<uint32_t> seen(kVideos, 0);
        for (uint32_t a = 0; a < kVideos; a++) seen[c.na(r, a)]++;
        for (uint32_t n : seen) CHECK(n == 1, "block %u holds every count 0 .. 70 once", r);
        if (r) CHECK(c.na(r, 1) != c.na(0, 1), "the window counts differ per rate");
    }
    unsigned long long cells = 0, records = 0, none = 0, want_cells = 0;
    for (uint32_t r = 0; r < kRates; r++)
        for (uint32_t a = 0; a < kVideos; a++)
            for (uint32_t b = 0; b < kVideos; b++) want_cells += (unsigned long long)c.na(r, a) * align_retimed_nb(c.nb(b), kRateList[r].den);
    // the walk: chunks of at most 600 triples and 2500 units close inside rates and, at the end of every rate, across the boundary
    const Closes w = replay_chunks(c, 600, 2500, false, false, true, &cells, &records);
    CHECK(cells == want_cells, "%llu cells of %llu", cells, want_cells);
    CHECK(w.inside_rate && w.across_rates && w.chunks > kRates, "the chunks of the walk close inside a rate and span a rate boundary");
    CHECK(records > w.triples / 4 && records < w.triples, "%llu records of %zu triples", records, w.triples);
    // the chunks alone: the library's bounds (one chunk: it spans all seven rates), tiny ones, each form
    const Closes one = replay_chunks(c, kAlignChunkPairs, kAlignChunkUnits, false, false, false, &none, &none);
    CHECK(one.chunks == 1 && one.across_rates && one.triples == w.triples, "one chunk for seven rates");
    size_t forms = 0;
    for (bool exclude_same : {false, true})
        for (bool listed : {false, true}) {
            if (exclude_same && listed) continue;
            for (size_t max_pairs : {(size_t)1, (size_t)5, (size_t)4000, kAlignChunkPairs})
                for (size_t max_units : {(size_t)1, (size_t)7, (size_t)40, kAlignChunkUnits}) {
                    const Closes cl = replay_chunks(c, max_pairs, max_units, exclude_same, listed, false, &none, &none);
                    CHECK(cl.triples <= w.triples && (exclude_same || listed) == (cl.triples < w.triples), "the triples of a form");
                    if (max_pairs == 4000 && max_units == kAlignChunkUnits) CHECK(cl.inside_rate && cl.across_rates, "4000 triples per chunk: inside and across");
                    forms++;
                }
        }
    // a list is checked with the rate in the variant's place
    size_t at = 0;
    const AlignRatesTriple unsorted[2] = {{0, 1, 1}, {0, 0, 1}}, rate_down[2] = {{0, 0, 1}, {5, 5, 0}}, twice[2] = {{2, 2, 3}, {2, 2, 3}}, far[1] = {{0, 0, kRates}};
    const AlignRatesTriple video[2] = {{0, 0, 0}, {kVideos, 0, 0}}, fine[3] = {{5, 5, 0}, {0, 0, 1}, {0, 1, 1}};
    CHECK(align_rates_list_check(unsorted, 2, kVideos, kVideos, kRates, &at) == 1 && at == 1 && align_rates_list_check(rate_down, 2, kVideos, kVideos, kRates, &at) == 1 &&
              align_rates_list_check(twice, 2, kVideos, kVideos, kRates, &at) == 1 && align_rates_list_check(far, 1, kVideos, kVideos, kRates, &at) == 4 && at == 0 &&
              align_rates_list_check(video, 2, kVideos, kVideos, kRates, &at) == 2 && at == 1 && align_rates_list_check(fine, 3, kVideos, kVideos, kRates, &at) == 0 &&
              align_rates_list_check(fine, 0, 0, 0, 1, &at) == 0,
          "the list check");
    // nothing to walk: no videos on a side, no rates
    AlignRatesCursor cur;
    AlignRatesChunk ch;
    CHECK(!align_rates_next_chunk(c.first_a.data(), 0, c.first_b.data(), kVideos, kRateList, kRates, false, cur, ch) && ch.empty(), "no videos of A");
    cur = AlignRatesCursor{};
    CHECK(!align_rates_next_chunk(c.first_a.data(), kVideos, c.first_b.data(), 0, kRateList, kRates, false, cur, ch) && ch.empty(), "no videos of B");
    std::printf("align rates plan ok: %llu cells, %llu records of %zu triples in %zu chunks, %zu chunkings\n", cells, records, w.triples, w.chunks, forms);
    return 0;
}
