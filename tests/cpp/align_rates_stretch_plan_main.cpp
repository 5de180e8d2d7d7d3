// The planner of the stretches call over (rate, a, b) triples (csrc/align_rates_stretch_plan.h) replayed on the CPU, built with
// -fsanitize=address,undefined by tests/test_align_rates_stretch_plan.py.  One call: 40 videos of A against 40 of B, 0 .. 70 windows each, with
// 1/1, 2/1, 3/2, 6/5 and 32/17 in ONE rate list and another window count of A in every rate's block.  Every chunk runs rounds 0 .. 3: round 0 on
// the chunk as align_rates_next_chunk made it, round k on what align_rates_next_round makes of round k - 1 and its records.  Every unit of every
// round is walked step by step and lane by lane as the kernels walk it (csrc/align.hip: align_bands_kernel<AlignTripleUnits, false>, align_bands_kernel<AlignTripleUnits, true>)
// - the triple from unit_offset, the slot from the triple, the rectangles from the round's sealed UPLOAD, at the offset the launch reads them - and
//   - every cell of every phase of every triple of the round is visited exactly once per round, masked or not;
//   - a cell is a miss by masking in exactly the rounds behind its rectangle: the mask the walk reads from the upload equals, cell by cell, the
//     mask of a brute-force twin that keeps its own rectangles in its own arithmetic;
//   - the band records of round k, reduced, equal the twin's rank-k record;
//   - the triples of round k are exactly the triples with a record in round k - 1, in order, with the units they had;
//   - a round without a record has no successor (align_rates_more_rounds), and none follows round max_stretches - 1;
//   - chunks close inside a rate and across a rate boundary.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <tuple>
#include <vector>

#include "align_rates_stretch_plan.h"

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

// distances 0 .. 7 with tolerance 2: three cells of eight match, runs of two and more are common and rare enough that some triples run dry
constexpr uint32_t kTol = 2, kMinRun = 2, kRounds = 4, kGuard = 3;
static uint32_t dist_of(uint32_t row_a, uint32_t row_b)
{
    uint32_t x = row_a * 2654435761u ^ (row_b + 0x9E3779B9u) * 40503u;
    x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 12; x *= 0x297A2D39u; x ^= x >> 15;
    return x & 7u;
}

constexpr uint32_t kRates = 5, kVideos = 40;
static const AlignSeedRate kRateList[kRates] = {{1, 1}, {2, 1}, {3, 2}, {6, 5}, {32, 17}};

struct Call {
    std::vector<uint32_t> first_a;   // [kRates][kVideos + 1]
    std::vector<size_t> rate_first;  // [kRates + 1]
    std::vector<uint32_t> first_b;   // [kVideos + 1]
    AlignRatesTable table;
    uint32_t na(uint32_t r, uint32_t a) const { return first_a[r * (kVideos + 1) + a + 1] - first_a[r * (kVideos + 1) + a]; }
    uint32_t nb(uint32_t b) const { return first_b[b + 1] - first_b[b]; }
    uint32_t row_a(uint32_t r, uint32_t a, uint32_t k) const { return (uint32_t)(rate_first[r] + first_a[r * (kVideos + 1) + a] + k); }
    uint32_t row_b(uint32_t b, uint32_t k) const { return first_b[b] + k; }
};

static Call make_call()
{
    Call c;
    c.first_a.assign(kRates * (kVideos + 1), 0);
    c.rate_first.assign(kRates + 1, 0);
    for (uint32_t r = 0; r < kRates; r++) {
        uint32_t *f = c.first_a.data() + r * (kVideos + 1);
        f[0] = 3 + r;
        for (uint32_t v = 0; v < kVideos; v++) f[v + 1] = f[v] + (v * (2 * r + 3) + 7 * r) % 71;  // 0 .. 70, another count per rate
        c.rate_first[r + 1] = c.rate_first[r] + f[kVideos] + 2;
    }
    c.first_b.assign(kVideos + 1, 4);
    for (uint32_t v = 0; v < kVideos; v++) c.first_b[v + 1] = c.first_b[v] + (v * 9) % 71;
    c.table = align_rates_table(kRateList, kRates, c.rate_first.data(), kVideos, 0);
    return c;
}

struct Record { uint32_t first_a, first_b, n, sum; bool any; };
struct TwinRect { int64_t a_lo, a_hi, b_lo, b_hi; };

// the twin's own rectangle, in its own arithmetic
static TwinRect twin_rect(const Record &w, uint32_t num, uint32_t den, int64_t Na, int64_t Nb)
{
    const int64_t ga = ((int64_t)kGuard * num + den - 1) / den;
    return TwinRect{std::max<int64_t>(0, (int64_t)w.first_a - ga), std::min<int64_t>(Na, (int64_t)w.first_a + (int64_t)num * (w.n - 1) + 1 + ga),
                    std::max<int64_t>(0, (int64_t)w.first_b - kGuard), std::min<int64_t>(Nb, (int64_t)w.first_b + (int64_t)den * (w.n - 1) + 1 + kGuard)};
}
static bool twin_masked(const std::vector<TwinRect> &rects, int64_t ra, int64_t rb)
{
    for (const TwinRect &q : rects)
        if (ra >= q.a_lo && ra < q.a_hi && rb >= q.b_lo && rb < q.b_hi) return true;
    return false;
}

// the twin: every diagonal of every phase of the triple on the cells its rectangles leave, tuples
static Record twin(const Call &c, uint32_t r, uint32_t a, uint32_t b, const std::vector<TwinRect> &rects)
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
                uint32_t dd = 99u;
                if (inside && !twin_masked(rects, p + num * i, den * (i + d))) dd = dist_of(c.row_a(r, a, (uint32_t)(p + num * i)), c.row_b(b, (uint32_t)(den * (i + d))));
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

struct Counts { unsigned long long cells = 0, masked = 0, records[kRounds] = {}, triples[kRounds] = {}; };

// one unit of a round as the kernel walks it, the rectangles read from the upload `up`; twin_rects[t]: the twin's rectangles of triple t
static AlignBandRecord walk_unit(const Call &c, const AlignRatesRound &round, const uint32_t *up, uint32_t unit, std::vector<std::vector<uint32_t>> &visits,
                                 const std::vector<std::vector<TwinRect>> &twin_rects, Counts *n)
{
    const AlignRatesChunk &ch = round.chunk;
    const uint32_t n_triples = (uint32_t)ch.n_triples();
    const uint32_t *unit_offset = up + align_rates_plan_offsets_at(n_triples) / 4, *triples = up + align_rates_plan_triples_at() / 4;
    const AlignRect *rects = reinterpret_cast<const AlignRect *>(up + align_rates_plan_rects_at(n_triples) / 4);
    const uint32_t t = align_unit_pair(unit_offset, n_triples, unit);
    CHECK(t < n_triples && unit_offset[t] <= unit && unit < unit_offset[t + 1], "unit %u -> triple %u", unit, t);
    const uint32_t va = triples[3 * t], vb = triples[3 * t + 1], slot = triples[3 * t + 2];
    CHECK(slot < kRates, "slot %u", slot);
    const AlignRatesSlot sl = reinterpret_cast<const AlignRatesSlot *>(up)[slot];
    const uint32_t *af = c.first_a.data() + sl.first_at;
    const uint32_t fa = sl.row0 + af[va], Na_all = af[va + 1] - af[va];
    const uint32_t fb = c.first_b[vb], Nb_all = c.first_b[vb + 1] - fb;
    CHECK(fa == c.row_a(slot, va, 0) && Na_all == c.na(slot, va) && sl.num == kRateList[slot].num && sl.den == kRateList[slot].den, "the slot of triple %u", t);
    AlignRect rc[kAlignMaxStretches - 1];
    for (uint32_t i = 0; i < kAlignMaxStretches - 1; i++) rc[i] = i < round.n_rects ? rects[(size_t)t * round.n_rects + i] : AlignRect{0u, 0u, 0u, 0u};
    uint32_t phase = ~0u, band = ~0u;
    const AlignRetimedSplit sp = align_retimed_split(Na_all, Nb_all, sl.num, sl.den);
    align_retimed_unit(sp, unit - unit_offset[t], &phase, &band);
    CHECK(phase < sl.num && band < align_retimed_phase_units(sp, phase), "unit %u -> phase %u band %u", unit, phase, band);
    const uint32_t Na = align_retimed_na(Na_all, sl.num, phase), Nb = align_retimed_nb(Nb_all, sl.den);
    const int32_t d0 = align_band_d0(Na, band);
    const uint32_t ka0 = align_ka_begin(d0), ka1 = align_ka_end(Na, Nb, d0);
    CHECK(ka0 < ka1 && ka1 <= Na, "steps %u .. %u", ka0, ka1);
    std::vector<uint32_t> &seen = visits[t];
    const size_t cell0 = [&]() { size_t k = 0; for (uint32_t p = 0; p < phase; p++) k += (size_t)align_retimed_na(Na_all, sl.num, p) * Nb; return k; }();
    int32_t row[kAlignBand];
    uint32_t len[kAlignBand] = {}, sum[kAlignBand] = {};
    uint32_t b_score[kAlignBand] = {}, b_start[kAlignBand] = {}, b_n[kAlignBand] = {}, b_sum[kAlignBand] = {};
    int32_t b_off[kAlignBand] = {};
    for (uint32_t lane = 0; lane < kAlignBand; lane++) row[lane] = align_lane_row(lane, ka0, d0);
    for (uint32_t ka = ka0; ka < ka1; ka++) {
        const uint32_t ra = align_retimed_row_a(phase, sl.num, ka);
        CHECK(ra < Na_all, "row %u of A at or behind %u", ra, Na_all);
        bool in_a = false;
        for (uint32_t i = 0; i < kAlignMaxStretches - 1; i++) in_a = in_a || align_rect_has_a(rc[i], ra);
        for (uint32_t lane = 0; lane < kAlignBand; lane++) {
            const int32_t kb = row[lane];
            const bool row_ok = kb >= 0 && kb < (int32_t)Nb;
            uint32_t d = 99;
            bool match = false;
            if (row_ok) {
                const uint32_t rb = align_retimed_row_b(sl.den, (uint32_t)kb);
                CHECK(rb < Nb_all, "row %u of B at or behind %u", rb, Nb_all);
                d = dist_of(fa + ra, fb + rb);
                seen[cell0 + (size_t)ka * Nb + (uint32_t)kb]++;
                n->cells++;
                match = d <= kTol;
                const bool masked = in_a && align_cell_masked(rc, kAlignMaxStretches - 1, ra, rb);
                CHECK(masked == twin_masked(twin_rects[t], ra, rb), "triple (%u, %u, %u) round %u: cell (%u, %u) masked %d", slot, va, vb, round.n_rects, ra, rb, (int)masked);
                if (masked) { match = false; n->masked++; }
            }
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
        if (ka + 1 < ka1) row[align_reload_lane(ka, d0)] += (int32_t)kAlignBand;
    }
    uint32_t w_score = 0, w_start = 0, w_n = 0, w_sum = 0;
    int32_t w_off = 0;
    for (uint32_t lane = 0; lane < kAlignBand; lane++)
        if (align_better(b_score[lane], b_off[lane], b_start[lane], w_score, w_off, w_start)) {
            w_score = b_score[lane]; w_off = b_off[lane]; w_start = b_start[lane]; w_n = b_n[lane]; w_sum = b_sum[lane];
        }
    return AlignBandRecord{w_off, w_start, w_score ? w_n : 0u, w_sum};
}

struct Rec { uint32_t a, b, rate, first_a, first_b, n_windows; };  // what align_rates_next_round reads of a record

// rounds 0 .. kRounds - 1 of one chunk, as the driver runs them
static void walk_chunk(const Call &c, const AlignRatesChunk &chunk, Counts *n)
{
    AlignRatesRound round, next;
    round.chunk = chunk;
    std::vector<std::vector<TwinRect>> twin_rects(chunk.n_triples());  // per triple of the ROUND
    for (uint32_t k = 0;; k++) {
        CHECK(k < kRounds && round.n_rects == k, "round %u", k);
        const AlignRatesChunk &ch = round.chunk;
        const uint32_t *up = static_cast<const uint32_t *>(align_rates_round_seal(round, c.table));
        CHECK(ch.plan.size() * 4 == align_rates_round_plan_bytes(ch.n_triples(), k) && align_rates_plan_rects_at(ch.n_triples()) % 16 == 0 &&
                  align_rates_plan_rects_at(ch.n_triples()) >= align_rates_plan_bytes(ch.n_triples()) && round.rects.size() == ch.n_triples() * k,
              "the upload of round %u", k);
        std::vector<std::vector<uint32_t>> visits(ch.n_triples());
        for (size_t t = 0; t < ch.n_triples(); t++)
            visits[t].assign((size_t)c.na(ch.triple(t).rate, ch.triple(t).a) * align_retimed_nb(c.nb(ch.triple(t).b), kRateList[ch.triple(t).rate].den), 0);
        std::vector<AlignBandRecord> band_records(ch.n_units());
        for (const AlignLaunchCut &cut : align_launch_cuts(ch.n_groups(), 97))
            for (size_t g = 0; g < cut.n; g++)
                for (uint32_t w = 0; w < kAlignWaves; w++) {
                    const size_t unit = (g + cut.group_base) * kAlignWaves + w;
                    if (unit < ch.n_units()) band_records[unit] = walk_unit(c, round, up, (uint32_t)unit, visits, twin_rects, n);
                }
        std::vector<Rec> recs;
        std::vector<std::vector<TwinRect>> next_rects;
        for (size_t t = 0; t < ch.n_triples(); t++) {
            const AlignRatesTriple tr = ch.triple(t);
            for (size_t i = 0; i < visits[t].size(); i++) CHECK(visits[t][i] == 1, "triple (%u, %u, %u) round %u: cell %zu visited %u times", tr.rate, tr.a, tr.b, k, i, visits[t][i]);
            const uint32_t num = kRateList[tr.rate].num, den = kRateList[tr.rate].den;
            const AlignRetimedSplit sp = align_retimed_split(c.na(tr.rate, tr.a), c.nb(tr.b), num, den);
            CHECK(ch.unit_offset[t + 1] - ch.unit_offset[t] == align_retimed_units(sp), "units of triple %zu in round %u", t, k);
            const AlignRetimedBest got = align_retimed_reduce(band_records.data() + ch.unit_offset[t], sp, den, kTol);
            const Record want = twin(c, tr.rate, tr.a, tr.b, twin_rects[t]);
            CHECK((got.score != 0) == want.any, "triple (%u, %u, %u) rank %u: a record on one side only", tr.rate, tr.a, tr.b, k);
            if (!want.any) continue;
            CHECK(got.first_a == want.first_a && got.first_b == want.first_b && got.n_windows == want.n && got.dist_sum == want.sum,
                  "triple (%u, %u, %u) rank %u: (%u, %u, %u, %u), the twin has (%u, %u, %u, %u)", tr.rate, tr.a, tr.b, k, got.first_a, got.first_b, got.n_windows,
                  got.dist_sum, want.first_a, want.first_b, want.n, want.sum);
            recs.push_back(Rec{tr.a, tr.b, tr.rate, got.first_a, got.first_b, got.n_windows});
            next_rects.push_back(twin_rects[t]);
            next_rects.back().push_back(twin_rect(want, num, den, c.na(tr.rate, tr.a), c.nb(tr.b)));
        }
        n->triples[k] += ch.n_triples();
        n->records[k] += recs.size();
        if (!align_rates_more_rounds(k, recs.size(), kRounds)) {
            CHECK(recs.empty() || k + 1 == kRounds, "the rounds of a chunk end at an empty round or at max_stretches");
            break;
        }
        CHECK(align_rates_next_round(round, recs.data(), recs.size(), c.first_a.data(), kVideos, c.first_b.data(), kRateList, kGuard, next), "next round");
        // the survivors are exactly the triples with a record, in order, with their units
        CHECK(next.chunk.n_triples() == recs.size() && next.n_rects == k + 1 && next.chunk.n_units() <= ch.n_units(), "the survivors of round %u", k);
        for (size_t i = 0, p = 0; i < recs.size(); i++, p++) {
            while (ch.triple(p).a != recs[i].a || ch.triple(p).b != recs[i].b || ch.triple(p).rate != recs[i].rate) p++;
            const AlignRatesTriple s = next.chunk.triple(i);
            CHECK(s.a == recs[i].a && s.b == recs[i].b && s.rate == recs[i].rate, "survivor %zu", i);
            CHECK(next.chunk.unit_offset[i + 1] - next.chunk.unit_offset[i] == ch.unit_offset[p + 1] - ch.unit_offset[p], "units of survivor %zu", i);
            for (uint32_t q = 0; q <= k; q++) {   // the rectangles so far and the new one, equal to the twin's
                const AlignRect &x = next.rects[i * (k + 1) + q];
                const TwinRect &y = next_rects[i][q];
                CHECK(x.a_lo == y.a_lo && x.a_hi == y.a_hi && x.b_lo == y.b_lo && x.b_hi == y.b_hi, "rectangle %u of survivor %zu", q, i);
            }
        }
        std::swap(round, next);
        twin_rects.swap(next_rects);
    }
}

int main()
{
    const Call c = make_call();
    for (uint32_t r = 1; r < kRates; r++) CHECK(c.na(r, 1) != c.na(0, 1), "the window counts differ per rate");
    // chunks of at most 300 triples and 1500 units: they close inside rates and across the rate boundaries
    std::vector<AlignRatesChunk> chunks;
    AlignRatesCursor cur;
    AlignRatesChunk ch;
    bool inside = false, across = false;
    uint32_t last_rate = ~0u;
    while (align_rates_next_chunk(c.first_a.data(), kVideos, c.first_b.data(), kVideos, kRateList, kRates, false, cur, ch, 300, 1500)) {
        if (ch.triple(0).rate == last_rate) inside = true;
        if (ch.triple(0).rate != ch.triple(ch.n_triples() - 1).rate) across = true;
        last_rate = ch.triple(ch.n_triples() - 1).rate;
        chunks.push_back(ch);
    }
    CHECK(inside && across && chunks.size() > kRates, "the chunks close inside a rate and span a rate boundary");
    Counts total;
    std::atomic<size_t> next{0};
    std::mutex mu;
    const auto worker = [&]() {
        Counts n;
        for (size_t i = next++; i < chunks.size(); i = next++) walk_chunk(c, chunks[i], &n);
        std::lock_guard<std::mutex> lk(mu);
        total.cells += n.cells; total.masked += n.masked;
        for (uint32_t k = 0; k < kRounds; k++) { total.records[k] += n.records[k]; total.triples[k] += n.triples[k]; }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < std::min(8u, std::max(1u, std::thread::hardware_concurrency())); t++) pool.emplace_back(worker);
    worker();
    for (std::thread &t : pool) t.join();
    for (uint32_t k = 0; k + 1 < kRounds; k++) CHECK(total.triples[k + 1] == total.records[k], "round %u walks the %llu triples with a record in round %u", k + 1, total.records[k], k);
    CHECK(total.records[0] < total.triples[0] && total.records[kRounds - 1] > 0 && total.records[kRounds - 1] < total.records[0] && total.masked > 0,
          "some triples have no record, some run dry on the way, some reach rank %u", kRounds - 1);
    // no successor of an empty round, none behind the last rank; the rectangle in 64-bit arithmetic, and 4.12's at 1/1
    CHECK(!align_rates_more_rounds(0, 0, 8) && !align_rates_more_rounds(0, 5, 1) && align_rates_more_rounds(0, 5, 2) && !align_rates_more_rounds(7, 5, 8), "more rounds");
    const AlignRect far = align_rates_rect_of(0xFFFFFFF0u, 0xFFFFFFF0u, 0xFFFFFFFFu, 32, 17, 1u << 20, 0xFFFFFFFFu, 0xFFFFFFFFu);
    CHECK(far.a_hi == 0xFFFFFFFFu && far.b_hi == 0xFFFFFFFFu && far.a_lo == 0xFFFFFFF0u - ((32u << 20) + 16) / 17 && far.b_lo == 0xFFFFFFF0u - (1u << 20), "nothing wraps");
    for (uint32_t g : {0u, 1u, 15u, 1u << 20}) {
        const AlignRect x = align_rates_rect_of(10, 7, 5, 1, 1, g, 40, 30), y = align_rect_of(-3, 10, 5, g, 40, 30);
        CHECK(x.a_lo == y.a_lo && x.a_hi == y.a_hi && x.b_lo == y.b_lo && x.b_hi == y.b_hi, "at 1/1 the rectangle is align_rect_of's");
    }
    const AlignRect g65 = align_rates_rect_of(23, 10, 7, 6, 5, 2, 100, 60);
    CHECK(g65.a_lo == 20 && g65.a_hi == 63 && g65.b_lo == 8 && g65.b_hi == 43, "6/5, guard 2: ga = 3");
    std::printf("align rates stretch plan ok: %llu cells (%llu masked) in %zu chunks; triples / records per round:", total.cells, total.masked, chunks.size());
    for (uint32_t k = 0; k < kRounds; k++) std::printf(" %llu / %llu", total.triples[k], total.records[k]);
    std::printf("\n");
    return 0;
}
