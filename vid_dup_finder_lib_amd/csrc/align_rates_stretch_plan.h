// Every stretch of a retimed pair, ranked, at up to 8 rates in one call (vdf_align_windows_rates_stretches*): the cross product of
// align_plan.h's rounds (rank k of a pair = the best run of its matrix with the rectangles of ranks 0 ... k - 1 as misses) and align_rates_plan.h's
// (rate, a, b) triples.  What the phases add: a reported stretch lies in ONE phase's sub-matrix, but its rectangle is kept in the ROWS OF THE TWO
// VIDEOS and masks the cells of every phase - otherwise rank 1 would be the same stretch seen from the neighbouring phase.  Round 0 of a chunk is
// launch_align_rates_chunk as it is; round k >= 1 lists only the triples that had a record in round k - 1, each with its k rectangles, which go up
// in the chunk's one upload behind table | triples | unit_offset.  Host only apart from the rectangle itself, no HIP calls: api.cpp, align.hip and
// the CPU replay (tests/cpp/align_rates_stretch_plan_main.cpp) share one text.
#pragma once
#include "align_rates_plan.h"

namespace vdf {

// The rectangle of a reported stretch (first_a, first_b, n) of a triple at num / den (lowest terms), in rows of a (Na of them, in the rate's block)
// and rows of b (Nb): its rows p + num i of a and den j of b, widened by guard rows of b - frames of b: B holds plain windows at stride 1 - and
// by as many frames in a's rows, ga = ceil(guard num / den); clipped to the videos.  64-bit arithmetic: nothing wraps for any 32-bit argument.
// At 1/1 it is align_rect_of's rectangle.
VDF_ALIGN_HD AlignRect align_rates_rect_of(uint32_t first_a, uint32_t first_b, uint32_t n, uint32_t num, uint32_t den, uint32_t guard, uint32_t Na, uint32_t Nb)
{
    const int64_t g = (int64_t)guard, ga = (g * (int64_t)num + (int64_t)den - 1) / (int64_t)den, steps = n ? (int64_t)n - 1 : 0;
    const int64_t sa = (int64_t)first_a, sb = (int64_t)first_b;
    const auto clip = [](int64_t v, int64_t hi) { return (uint32_t)(v < 0 ? 0 : v > hi ? hi : v); };
    return AlignRect{clip(sa - ga, (int64_t)Na), clip(sa + (int64_t)num * steps + 1 + ga, (int64_t)Na), clip(sb - g, (int64_t)Nb),
                     clip(sb + (int64_t)den * steps + 1 + g, (int64_t)Nb)};
}
// cell (i, j) of the sub-matrix of phase p is masked iff ONE rectangle holds row p + num i of a and row den j of b: align_cell_masked on those rows

// One round of a chunk: its triples in (rate, a, b) order with their units - an AlignRatesChunk, so that it seals and uploads as one - and
// rects[triple * n_rects + i], the rectangles of ranks 0 ... n_rects - 1.
struct AlignRatesRound {
    AlignRatesChunk chunk;
    std::vector<AlignRect> rects;  // [triples][n_rects]
    uint32_t n_rects = 0;          // = the round's number
};

// the one upload of a masked round, in bytes: table | triples | unit_offset | (pad to 16) | rects
inline size_t align_rates_plan_rects_at(size_t n_triples) { return (align_rates_plan_bytes(n_triples) + 15) & ~(size_t)15; }
inline size_t align_rates_round_plan_bytes(size_t n_triples, uint32_t n_rects) { return align_rates_plan_rects_at(n_triples) + n_triples * n_rects * sizeof(AlignRect); }

// -> the round's upload (align_rates_round_plan_bytes bytes): the chunk sealed, the rectangles behind it
inline const void *align_rates_round_seal(AlignRatesRound &r, const AlignRatesTable &table)
{
    static_assert(sizeof(AlignRect) == 4 * sizeof(uint32_t), "rectangles are counted in dwords");
    if (r.chunk.sealed) return r.chunk.plan.data();
    r.chunk.seal(table);
    r.chunk.plan.resize(align_rates_plan_rects_at(r.chunk.n_triples()) / sizeof(uint32_t), 0u);  // the pad goes up too: round 0 has nothing behind it
    if (r.n_rects) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(r.rects.data());
        r.chunk.plan.insert(r.chunk.plan.end(), w, w + 4 * r.rects.size());
    }
    return r.chunk.plan.data();
}

// Is there a round behind round `rank` (0-based) that left n_recs records?  Only if a triple can reach the next rank: a round without a record
// has no survivor, so NO masked launch follows it - a call whose triples have no record costs what vdf_align_windows_rates* costs.
inline bool align_rates_more_rounds(uint32_t rank, size_t n_recs, uint32_t max_stretches) { return n_recs != 0 && rank + 1 < max_stretches; }

// Round prev.n_rects + 1 from round prev and its records (one per triple of prev that had a record, in (rate, a, b) order; Rec has a, b, rate,
// first_a, first_b, n_windows): the triples with a record survive, in order, each with its rectangles so far and the one of its new record, and
// the units it had.  A round is a subset of its predecessor: it stays inside the chunk's limits and the scratch of round 0 holds it.  False: a
// record names a triple that prev does not hold in that order - not a result of prev.  first_a: n_rates x (n_a + 1).
template <class Rec>
inline bool align_rates_next_round(const AlignRatesRound &prev, const Rec *recs, size_t n_recs, const uint32_t *first_a, size_t n_a, const uint32_t *first_b,
                                   const AlignSeedRate *rates, uint32_t guard, AlignRatesRound &next)
{
    next.n_rects = prev.n_rects + 1;
    next.rects.clear();
    next.rects.reserve(n_recs * next.n_rects);
    next.chunk.begin(n_recs);
    size_t p = 0;
    uint32_t units = 0;
    const size_t n_prev = prev.chunk.n_triples();
    for (size_t i = 0; i < n_recs; i++) {
        for (; p < n_prev; p++) {
            const AlignRatesTriple t = prev.chunk.triple(p);
            if (t.a == recs[i].a && t.b == recs[i].b && t.rate == recs[i].rate) break;
        }
        if (p == n_prev) { next.chunk.end(); return false; }
        const uint32_t r = recs[i].rate, *fa = first_a + (size_t)r * (n_a + 1);
        const uint32_t Na = fa[recs[i].a + 1] - fa[recs[i].a], Nb = first_b[recs[i].b + 1] - first_b[recs[i].b];
        units += prev.chunk.unit_offset[p + 1] - prev.chunk.unit_offset[p];
        next.chunk.push(recs[i].a, recs[i].b, r, units);
        for (uint32_t k = 0; k < prev.n_rects; k++) next.rects.push_back(prev.rects[p * prev.n_rects + k]);
        next.rects.push_back(align_rates_rect_of(recs[i].first_a, recs[i].first_b, recs[i].n_windows, rates[r].num, rates[r].den, guard, Na, Nb));
        p++;
    }
    next.chunk.end();
    return next.chunk.n_triples() <= n_prev && next.chunk.n_units() <= prev.chunk.n_units();
}

}  // namespace vdf
