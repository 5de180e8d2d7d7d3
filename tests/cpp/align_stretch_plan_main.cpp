// The planner of the align-stretches calls (csrc/align_plan.h: AlignRect, align_rect_of, align_cell_masked, align_next_round)
// replayed on the CPU, built with -fsanitize=address,undefined by tests/test_align_stretch_plan.py.  For every (Na, Nb) in 0 .. 140 x 0 .. 140,
// with stretches in every corner, on every edge and inside the matrix, at guards that clamp nowhere, somewhere and everywhere:
//   - the rectangle rule: align_rect_of against the definition written out cell by cell, and at the ends of the 32-bit ranges (nothing wraps);
//   - the band walk with the mask: the masked kernel's walk (csrc/align.hip: align_bands_kernel<AlignPairUnits<false>, true>), lane by lane with the header's own
//     functions, over a synthetic distance matrix with up to three rectangles, reduced over lanes and bands - against a direct walk of every
//     diagonal in which a masked cell is a miss;
//   - the round builder: for pair lists of mixed lengths in both modes, three rounds of survivors - their order, their unit offsets, exactly r
//     rectangles each (those of the rounds before, then the new one), a subset of the round before.
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

struct Stretch { int32_t offset; uint32_t start_a, n; };
struct Run { uint32_t score; int32_t offset; uint32_t start, n, sum; };
struct Rec { uint32_t a, b; int32_t offset; uint32_t start_a, n_windows, dist_sum; };

constexpr uint32_t kTol = 5;
// a synthetic distance: three cells in four are within kTol, so that runs are long and cut often
static uint32_t dist_of(uint32_t ka, uint32_t kb) { return ((ka * 2654435761u) ^ (kb * 40503u) ^ ((ka + 3 * kb) >> 2)) % 8u; }

// ---- the rectangle rule -----------------------------------------------------------------------------------------------------------------------
static void check_rect(const Stretch &s, uint32_t guard, uint32_t Na, uint32_t Nb, unsigned long long *rects)
{
    const AlignRect r = align_rect_of(s.offset, s.start_a, s.n, guard, Na, Nb);
    CHECK(r.a_lo <= r.a_hi && r.a_hi <= Na && r.b_lo <= r.b_hi && r.b_hi <= Nb, "Na %u Nb %u: [%u, %u) x [%u, %u)", Na, Nb, r.a_lo, r.a_hi, r.b_lo, r.b_hi);
    // the definition, cell by cell: |distance to the stretch's rows| <= guard on both sides, inside the matrix
    const long long sa = s.start_a, sb = sa + s.offset, g = guard, n = s.n;
    for (uint32_t ka = 0; ka < Na; ka++) CHECK(align_rect_has_a(r, ka) == ((long long)ka >= sa - g && (long long)ka < sa + n + g), "row %u of A", ka);
    for (uint32_t kb = 0; kb < Nb; kb++) CHECK(align_rect_has_b(r, kb) == ((long long)kb >= sb - g && (long long)kb < sb + n + g), "row %u of B", kb);
    CHECK(!align_rect_has_b(r, (uint32_t)-1) && !align_rect_has_b(r, (uint32_t)-64) && !align_rect_has_a(r, Na) && !align_rect_has_b(r, Nb), "a row outside the matrix");
    (*rects)++;
}

// ---- the band walk with the mask: what align_bands_kernel<AlignPairUnits<false>, true> does, lane by lane --------------------------------------------------------------
static Run walk_bands(uint32_t Na, uint32_t Nb, const AlignRect *rects, uint32_t n_rects, uint32_t min_run, unsigned long long *steps)
{
    AlignRect rc[kAlignMaxStretches - 1];  // the kernel's slots: those behind n_rects are empty
    for (uint32_t i = 0; i < kAlignMaxStretches - 1; i++) rc[i] = i < n_rects ? rects[i] : AlignRect{0u, 0u, 0u, 0u};
    Run best{0, 0, 0, 0, 0};
    for (uint32_t band = 0; band < align_bands(Na, Nb); band++) {
        const int32_t d0 = align_band_d0(Na, band);
        const uint32_t ka0 = align_ka_begin(d0), ka1 = align_ka_end(Na, Nb, d0);
        int32_t kb[kAlignBand];
        bool row_ok[kAlignBand];
        uint32_t len[kAlignBand] = {}, sum[kAlignBand] = {};
        Run lane_best[kAlignBand];
        for (uint32_t lane = 0; lane < kAlignBand; lane++) {
            kb[lane] = align_lane_row(lane, ka0, d0);
            row_ok[lane] = kb[lane] >= 0 && kb[lane] < (int32_t)Nb;
            lane_best[lane] = Run{0, 0, 0, 0, 0};
        }
        for (uint32_t ka = ka0; ka < ka1; ka++) {
            bool in_a = false;
            for (uint32_t i = 0; i < kAlignMaxStretches - 1; i++) in_a = in_a || align_rect_has_a(rc[i], ka);
            for (uint32_t lane = 0; lane < kAlignBand; lane++) {
                const uint32_t d = row_ok[lane] ? dist_of(ka, (uint32_t)kb[lane]) : 0u;
                bool match = row_ok[lane] && d <= kTol;
                if (in_a) match = match && !align_cell_masked(rc, kAlignMaxStretches - 1, ka, (uint32_t)kb[lane]);
                if (match) { len[lane] += 1; sum[lane] += d; }
                const bool edge = ka + 1 == Na || kb[lane] + 1 == (int32_t)Nb;
                const bool ends = len[lane] != 0 && (!match || edge);
                if (ends && len[lane] >= min_run) {
                    const uint32_t score = len[lane] * (kTol + 1) - sum[lane], start = (match ? ka + 1 : ka) - len[lane];
                    const int32_t off = kb[lane] - (int32_t)ka;
                    Run &b = lane_best[lane];
                    if (align_better(score, off, start, b.score, b.offset, b.start)) b = Run{score, off, start, len[lane], sum[lane]};
                }
                if (ends) { len[lane] = 0; sum[lane] = 0; }
            }
            (*steps)++;
            uint32_t nl[kAlignBand], ns[kAlignBand];
            for (uint32_t lane = 0; lane < kAlignBand; lane++) { nl[lane] = len[align_rotate_source(lane)]; ns[lane] = sum[align_rotate_source(lane)]; }
            for (uint32_t lane = 0; lane < kAlignBand; lane++) { len[lane] = nl[lane]; sum[lane] = ns[lane]; }
            if (ka + 1 < ka1) {
                const uint32_t lane = align_reload_lane(ka, d0);
                kb[lane] += (int32_t)kAlignBand;
                CHECK(kb[lane] == align_reload_row(ka, d0), "the reloaded row");
                row_ok[lane] = kb[lane] < (int32_t)Nb;
            }
        }
        for (uint32_t lane = 0; lane < kAlignBand; lane++)
            if (align_better(lane_best[lane].score, lane_best[lane].offset, lane_best[lane].start, best.score, best.offset, best.start)) best = lane_best[lane];
    }
    return best;
}

// every diagonal walked directly; a masked cell is a miss
static Run walk_diagonals(uint32_t Na, uint32_t Nb, const AlignRect *rects, uint32_t n_rects, uint32_t min_run)
{
    Run best{0, 0, 0, 0, 0};
    for (long long d = -((long long)Na - 1); d <= (long long)Nb - 1; d++) {
        const long long ka0 = d < 0 ? -d : 0, ka1 = (long long)Nb - d < (long long)Na ? (long long)Nb - d : (long long)Na;
        uint32_t len = 0, sum = 0;
        for (long long ka = ka0; ka <= ka1; ka++) {
            bool match = false;
            uint32_t dist = 0;
            if (ka < ka1) {
                bool masked = false;
                for (uint32_t i = 0; i < n_rects; i++)
                    masked = masked || (ka >= rects[i].a_lo && ka < rects[i].a_hi && ka + d >= rects[i].b_lo && ka + d < rects[i].b_hi);
                CHECK(masked == align_cell_masked(rects, n_rects, (uint32_t)ka, (uint32_t)(ka + d)), "cell (%lld, %lld)", ka, ka + d);
                dist = dist_of((uint32_t)ka, (uint32_t)(ka + d));
                match = !masked && dist <= kTol;
            }
            if (match) { len++; sum += dist; continue; }
            if (len >= min_run) {
                const uint32_t score = len * (kTol + 1) - sum, start = (uint32_t)(ka - len);
                if (align_better(score, (int32_t)d, start, best.score, best.offset, best.start)) best = Run{score, (int32_t)d, start, len, sum};
            }
            len = 0; sum = 0;
        }
    }
    return best;
}

// the stretches a pair is given: corners, edges, inside; long and short
static std::vector<Stretch> stretches_of(uint32_t Na, uint32_t Nb)
{
    std::vector<Stretch> s;
    if (Na == 0 || Nb == 0) return s;
    const uint32_t m = Na < Nb ? Na : Nb, n = m > 3 ? m / 3 : 1;
    const auto add = [&](uint32_t sa, uint32_t sb, uint32_t len) { s.push_back(Stretch{(int32_t)sb - (int32_t)sa, sa, len}); };
    add(0, 0, n);                              // the corner (0, 0)
    add(Na - n, Nb - n, n);                    // the corner (Na, Nb)
    add(0, Nb - n, n);                         // row 0 of A and the last row of B
    add(Na - n, 0, n);                         // the last row of A and row 0 of B
    add(0, 0, m);                              // the whole main diagonal
    add((Na - n) / 2, 0, n);                   // on an edge
    add((Na - n) / 2, (Nb - n) / 2, n);        // inside
    add(Na - 1, 0, 1);                         // the first diagonal
    add(0, Nb - 1, 1);                         // the last diagonal
    return s;
}

static void replay_pair(uint32_t Na, uint32_t Nb, bool all, unsigned long long *rects, unsigned long long *walks, unsigned long long *steps, unsigned long long *cut)
{
    const std::vector<Stretch> st = stretches_of(Na, Nb);
    const uint32_t guards[] = {0u, 3u, 70u, kAlignMaxGuard};  // 70: clamps on the sides a stretch is near; 2^20: everywhere
    for (const Stretch &s : st)
        for (uint32_t g : guards) check_rect(s, g, Na, Nb, rects);
    if (st.empty()) {
        const Run r = walk_bands(Na, Nb, nullptr, 0, 1, steps);
        CHECK(r.score == 0, "a run in an empty matrix");
        return;
    }
    // the walks: every pair a few of the combinations (all of them for the pairs named in main), so that every combination meets every size class
    const uint32_t n_combo = (uint32_t)st.size() * 4;
    const uint32_t turns = all ? n_combo : 2;
    for (uint32_t t = 0; t < turns; t++) {
        const uint32_t c = all ? t : (Na * 7 + Nb * 13 + t * 17) % n_combo;
        const uint32_t guard = guards[c % 4], min_run = 1 + (c + Na) % 3;
        AlignRect rc[3];
        const uint32_t n_rects = 1 + (c + Nb) % 3;
        for (uint32_t i = 0; i < n_rects; i++) {
            const Stretch &s = st[(c / 4 + i * 5) % st.size()];
            rc[i] = align_rect_of(s.offset, s.start_a, s.n, i == 0 ? guard : guards[(c + i) % 3], Na, Nb);
        }
        const Run got = walk_bands(Na, Nb, rc, n_rects, min_run, steps), want = walk_diagonals(Na, Nb, rc, n_rects, min_run);
        CHECK(got.score == want.score && got.offset == want.offset && got.start == want.start && got.n == want.n && got.sum == want.sum,
              "Na %u Nb %u combination %u: the bands find (%u, %d, %u, %u), the diagonals (%u, %d, %u, %u)", Na, Nb, c, got.score, got.offset, got.start, got.n,
              want.score, want.offset, want.start, want.n);
        const Run plain = walk_diagonals(Na, Nb, nullptr, 0, min_run);
        if (plain.score != want.score || plain.offset != want.offset || plain.start != want.start) (*cut)++;  // the mask changed the answer
        (*walks)++;
    }
}

// ---- the round builder ------------------------------------------------------------------------------------------------------------------------
static void replay_rounds(const std::vector<uint32_t> &ca, const std::vector<uint32_t> &cb, bool self, size_t max_pairs, size_t max_units, uint32_t guard,
                          unsigned long long *survivors)
{
    std::vector<uint32_t> fa(1, 0), fb(1, 0);
    for (uint32_t n : ca) fa.push_back(fa.back() + n);
    for (uint32_t n : (self ? ca : cb)) fb.push_back(fb.back() + n);
    const size_t n_a = ca.size(), n_b = self ? ca.size() : cb.size();
    AlignCursor cur;
    AlignChunk ch;
    while (align_next_chunk(fa.data(), n_a, fb.data(), n_b, self, cur, ch, max_pairs, max_units)) {
        AlignRound round, next;
        const size_t chunk_pairs = ch.pairs.size(), chunk_units = ch.n_units();
        align_round_zero(ch, round);  // takes the chunk's arrays
        CHECK(round.n_rects == 0 && round.rects.empty() && round.pairs.size() == chunk_pairs && round.n_units() == chunk_units && ch.pairs.empty(), "round 0");
        for (uint32_t r = 1; r < kAlignMaxStretches; r++) {
            // the records of round r - 1: every pair but those whose (a + b + r) is a multiple of 3 has one
            std::vector<Rec> recs;
            for (const AlignPair &p : round.pairs) {
                if ((p.a + p.b + r) % 3 == 0) continue;
                const uint32_t Na = fa[p.a + 1] - fa[p.a], Nb = fb[p.b + 1] - fb[p.b], n = 1 + (p.a + r) % (Na < Nb ? Na : Nb);
                recs.push_back(Rec{p.a, p.b, (int32_t)((p.b + r) % (Nb - n + 1)) - (int32_t)(Na - n), Na - n, n, 0u});
            }
            CHECK(align_next_round(round, recs.data(), recs.size(), fa.data(), fb.data(), guard, next), "round %u", r);
            CHECK(next.n_rects == r && next.pairs.size() == recs.size() && next.unit_offset.size() == recs.size() + 1 && next.unit_offset[0] == 0, "round %u: shape", r);
            CHECK(next.rects.size() == recs.size() * r, "round %u: %zu rectangles for %zu pairs", r, next.rects.size(), recs.size());
            CHECK(next.pairs.size() <= chunk_pairs && next.n_units() <= chunk_units, "round %u leaves its chunk", r);
            size_t at = 0;
            for (size_t i = 0; i < next.pairs.size(); i++) {
                const AlignPair p = next.pairs[i];
                CHECK(p.a == recs[i].a && p.b == recs[i].b, "round %u: survivor %zu", r, i);
                if (i) CHECK(next.pairs[i - 1].a < p.a || (next.pairs[i - 1].a == p.a && next.pairs[i - 1].b < p.b), "round %u: order", r);
                const uint32_t Na = fa[p.a + 1] - fa[p.a], Nb = fb[p.b + 1] - fb[p.b];
                CHECK(next.unit_offset[i + 1] - next.unit_offset[i] == align_bands(Na, Nb), "round %u: units of survivor %zu", r, i);
                while (round.pairs[at].a != p.a || round.pairs[at].b != p.b) at++;  // its place in the round before
                for (uint32_t k = 0; k + 1 < r; k++) {
                    const AlignRect &x = next.rects[i * r + k], &y = round.rects[at * (r - 1) + k];
                    CHECK(x.a_lo == y.a_lo && x.a_hi == y.a_hi && x.b_lo == y.b_lo && x.b_hi == y.b_hi, "round %u: rectangle %u of survivor %zu", r, k, i);
                }
                const AlignRect &x = next.rects[i * r + r - 1], y = align_rect_of(recs[i].offset, recs[i].start_a, recs[i].n_windows, guard, Na, Nb);
                CHECK(x.a_lo == y.a_lo && x.a_hi == y.a_hi && x.b_lo == y.b_lo && x.b_hi == y.b_hi && x.a_hi == Na, "round %u: the new rectangle of survivor %zu", r, i);
                (*survivors)++;
            }
            // a record of a pair the round does not hold, or out of order, is refused
            if (recs.size() >= 2) {
                std::vector<Rec> bad(recs.rbegin(), recs.rend());
                AlignRound scratch;
                CHECK(!align_next_round(round, bad.data(), bad.size(), fa.data(), fb.data(), guard, scratch), "round %u: records out of order accepted", r);
            }
            std::swap(round, next);
            if (round.pairs.empty()) break;
        }
    }
}

int main()
{
    unsigned long long rects = 0, walks = 0, steps = 0, cut = 0, survivors = 0;
    for (uint32_t Na = 0; Na <= 140; Na++)
        for (uint32_t Nb = 0; Nb <= 140; Nb++) {
            const auto edge = [](uint32_t n) { return n == 1 || n == 2 || n == 63 || n == 64 || n == 65 || n == 128 || n == 129 || n == 140; };
            replay_pair(Na, Nb, edge(Na) && edge(Nb), &rects, &walks, &steps, &cut);
        }
    for (uint32_t n : {199u, 200u, 257u}) { replay_pair(n, 70, true, &rects, &walks, &steps, &cut); replay_pair(70, n, true, &rects, &walks, &steps, &cut); }
    CHECK(cut * 4 > walks, "the mask changed the answer in %llu of %llu walks only", cut, walks);
    // nothing wraps at the ends of the ranges
    {
        const AlignRect r = align_rect_of(-2147483647 - 1, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
        CHECK(r.a_lo == 0 && r.a_hi == 0xFFFFFFFFu && r.b_lo == 0 && r.b_hi == 0xFFFFFFFFu, "the widest rectangle");
        const AlignRect q = align_rect_of(2147483647, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 100u, 100u);
        CHECK(q.a_lo <= q.a_hi && q.a_hi <= 100 && q.b_lo <= q.b_hi && q.b_hi <= 100 && !align_rect_has_a(q, 99) && !align_rect_has_b(q, 99), "a stretch behind the matrix");
        const AlignRect e = align_rect_of(-5, 2, 3, 0, 10, 10);  // start_b = -3: rows -3 .. -1 of B do not exist
        CHECK(e.b_lo == 0 && e.b_hi == 0 && e.a_lo == 2 && e.a_hi == 5, "a stretch in front of B");
        const AlignRect g = align_rect_of(0, 1u << 19, 1u << 19, kAlignMaxGuard, kAlignMaxWindows, kAlignMaxWindows);
        CHECK(g.a_lo == 0 && g.a_hi == kAlignMaxWindows && g.b_lo == 0 && g.b_hi == kAlignMaxWindows, "the largest legal guard");
    }
    const std::vector<uint32_t> ca = {1, 2, 63, 64, 65, 0, 127, 128, 129, 200, 0, 5}, cb = {200, 0, 65, 1, 128, 64, 2};
    for (bool self : {false, true})
        for (size_t max_pairs : {(size_t)1, (size_t)5, kAlignChunkPairs})
            for (size_t max_units : {(size_t)7, kAlignChunkUnits})
                for (uint32_t guard : {0u, 4u, kAlignMaxGuard}) replay_rounds(ca, cb, self, max_pairs, max_units, guard, &survivors);
    std::printf("align stretch plan ok: %llu rectangles, %llu masked walks in %llu steps (%llu changed by the mask), %llu survivors\n", rects, walks, steps, cut,
                survivors);
    return 0;
}
