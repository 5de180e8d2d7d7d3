// Alignment of retimed windows in one call (vdf_align_windows_retimed*): A holds retimed windows at stride 1, B plain windows at
// stride 1, the rate is num / den in lowest terms.  For every phase p < num the SUB-MATRIX of a pair has the cells (i, j) = (row p + num i of a,
// row den j of b); inside it everything is align_plan.h's: bands of 64 diagonals, the ka range of a band, the lane-ownership rules, align_better.
// This header adds what the phases add: the sub-matrix sizes, the rows behind (i, j), which (phase, band) a unit of a pair is, the reduction
// over the phases, and the chunks of a call with up to num x bands units per pair - as __host__ __device__ inline functions, so that the kernel
// (align.hip: align_bands_kernel<AlignPairUnits<true>, false>), the plain C++ definition (api.cpp) and the CPU replay (tests/cpp/align_retimed_plan_main.cpp) share
// one text.  No HIP calls.
#pragma once
#include "align_plan.h"

namespace vdf {

constexpr uint32_t kAlignRetimedMaxNum = 32;  // = VDF_ALIGN_RETIMED_MAX_NUM: above it the sub-matrices degenerate

inline uint32_t align_retimed_gcd(uint32_t a, uint32_t b)
{
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    return a;
}
// The rate of a call, reduced by its gcd.  0: fine; 1: not 1 <= den <= num <= 2 den; 2: the reduced num is above kAlignRetimedMaxNum.
inline int align_retimed_rate(uint32_t rate_num, uint32_t rate_den, uint32_t *num, uint32_t *den)
{
    if (rate_den < 1 || rate_num < rate_den || (uint64_t)rate_num > 2ull * rate_den) return 1;
    const uint32_t g = align_retimed_gcd(rate_num, rate_den);
    *num = rate_num / g;
    *den = rate_den / g;
    return *num > kAlignRetimedMaxNum ? 2 : 0;
}

// ---- the sub-matrix of phase p: Na_p x Nb_0 cells ---------------------------------------------------------------------------------------------
// rows p, p + num, ... of A's video: ceil((Na - p) / num), none if p >= Na
VDF_ALIGN_HD uint32_t align_retimed_na(uint32_t Na, uint32_t num, uint32_t p) { return p >= Na ? 0u : (Na - p + num - 1) / num; }
// rows 0, den, 2 den, ... of B's video: ceil(Nb / den)
VDF_ALIGN_HD uint32_t align_retimed_nb(uint32_t Nb, uint32_t den) { return (Nb + den - 1) / den; }
// the rows behind cell (i, j), counted inside their videos: below Na for i < Na_p, below Nb for j < Nb_0
VDF_ALIGN_HD uint32_t align_retimed_row_a(uint32_t p, uint32_t num, uint32_t i) { return p + num * i; }
VDF_ALIGN_HD uint32_t align_retimed_row_b(uint32_t den, uint32_t j) { return den * j; }

// ---- the units of a pair: (phase, band), phase-major ------------------------------------------------------------------------------------------
// With Na = q num + r (r < num) the phases p < r have q + 1 rows and the phases p >= r have q: two band counts, so a unit's phase is a division.
struct AlignRetimedSplit { uint32_t n_hi, bands_hi, bands_lo, num; };  // phases 0 ... n_hi - 1: bands_hi bands each; n_hi ... num - 1: bands_lo
VDF_ALIGN_HD AlignRetimedSplit align_retimed_split(uint32_t Na, uint32_t Nb, uint32_t num, uint32_t den)
{
    const uint32_t q = Na / num, r = Na % num, nb0 = align_retimed_nb(Nb, den);
    return AlignRetimedSplit{r, align_bands(q + 1, nb0), align_bands(q, nb0), num};
}
VDF_ALIGN_HD uint32_t align_retimed_units(const AlignRetimedSplit &s) { return s.n_hi * s.bands_hi + (s.num - s.n_hi) * s.bands_lo; }
VDF_ALIGN_HD uint32_t align_retimed_pair_units(uint32_t Na, uint32_t Nb, uint32_t num, uint32_t den)
{
    return align_retimed_units(align_retimed_split(Na, Nb, num, den));
}
// unit u of the pair (u < align_retimed_units) -> its phase and its band inside the phase's sub-matrix
VDF_ALIGN_HD void align_retimed_unit(const AlignRetimedSplit &s, uint32_t u, uint32_t *phase, uint32_t *band)
{
    const uint32_t hi = s.n_hi * s.bands_hi;
    if (u < hi) { *phase = u / s.bands_hi; *band = u % s.bands_hi; }
    else { *phase = s.n_hi + (u - hi) / s.bands_lo; *band = (u - hi) % s.bands_lo; }
}
// the first unit of phase p, and how many it has
VDF_ALIGN_HD uint32_t align_retimed_phase_units(const AlignRetimedSplit &s, uint32_t p) { return p < s.n_hi ? s.bands_hi : s.bands_lo; }
VDF_ALIGN_HD uint32_t align_retimed_phase_first(const AlignRetimedSplit &s, uint32_t p)
{
    return p < s.n_hi ? p * s.bands_hi : s.n_hi * s.bands_hi + (p - s.n_hi) * s.bands_lo;
}

// ---- the two-level reduction ------------------------------------------------------------------------------------------------------------------
// Level 1, inside a phase: align_better on (score, offset = j - i, i0) - vdf_align_windows' rule on the sub-matrix.
// Level 2, across the phases: the phase-bests compete by score, then the smaller first_a = p + num i0, then the smaller first_b = den (i0 + offset).
struct AlignRetimedBest { uint32_t score, first_a, first_b, n_windows, dist_sum; };  // score 0: none
VDF_ALIGN_HD bool align_retimed_better(uint32_t score, uint32_t first_a, uint32_t first_b, const AlignRetimedBest &best)
{
    if (score != best.score) return score > best.score;
    if (first_a != best.first_a) return first_a < best.first_a;
    return first_b < best.first_b;
}
// the band records of one pair (units in phase-major order, n_windows = 0: the band has no run) -> the pair's record
template <class Ptr> VDF_ALIGN_HD AlignRetimedBest align_retimed_reduce(Ptr band_records, const AlignRetimedSplit &s, uint32_t den, uint32_t tol)
{
    AlignRetimedBest best{0u, 0u, 0u, 0u, 0u};
    uint32_t u = 0;
    for (uint32_t p = 0; p < s.num; p++) {
        uint32_t ph_score = 0, ph_start = 0, ph_n = 0, ph_sum = 0;
        int32_t ph_off = 0;
        const uint32_t u1 = u + align_retimed_phase_units(s, p);
        for (; u < u1; ++u) {
            const AlignBandRecord r = band_records[u];
            if (r.n_windows == 0) continue;
            const uint32_t score = r.n_windows * (tol + 1) - r.dist_sum;
            if (align_better(score, r.offset, r.start_a, ph_score, ph_off, ph_start)) {
                ph_score = score; ph_off = r.offset; ph_start = r.start_a; ph_n = r.n_windows; ph_sum = r.dist_sum;
            }
        }
        if (ph_score == 0) continue;
        const uint32_t first_a = align_retimed_row_a(p, s.num, ph_start), first_b = align_retimed_row_b(den, (uint32_t)((int32_t)ph_start + ph_off));
        if (align_retimed_better(ph_score, first_a, first_b, best)) best = AlignRetimedBest{ph_score, first_a, first_b, ph_n, ph_sum};
    }
    return best;
}

// ---- the chunks of a call: align_plan.h's limits, a pair now up to num x bands units ----------------------------------------------------------
// all pairs a x b in (a, b) order (there is no self mode); pairs without a unit are skipped
inline bool align_retimed_next_chunk(const uint32_t *first_a, size_t n_a, const uint32_t *first_b, size_t n_b, uint32_t num, uint32_t den, AlignCursor &cur,
                                     AlignChunk &c, size_t max_pairs = kAlignChunkPairs, size_t max_units = kAlignChunkUnits)
{
    c.pairs.clear();
    c.unit_offset.assign(1, 0u);
    if (!cur.started) { cur.started = true; cur.a = 0; cur.b = 0; }
    size_t units = 0;
    while (cur.a < n_a) {
        if (cur.b >= n_b) { cur.a++; cur.b = 0; continue; }
        const uint32_t n = align_retimed_pair_units(first_a[cur.a + 1] - first_a[cur.a], first_b[cur.b + 1] - first_b[cur.b], num, den);
        if (n) {
            if (!c.pairs.empty() && (c.pairs.size() >= max_pairs || units + n > max_units)) return true;
            c.pairs.push_back({(uint32_t)cur.a, (uint32_t)cur.b});
            units += n;
            c.unit_offset.push_back((uint32_t)units);
        }
        cur.b++;
    }
    return !c.pairs.empty();
}
// the same fed from a checked pair list (align_pair_list_check, self = false); cur: the next list entry
template <class P>
inline bool align_retimed_next_chunk_pairs(const uint32_t *first_a, const uint32_t *first_b, const P *list, size_t n_list, uint32_t num, uint32_t den,
                                           size_t &cur, AlignChunk &c, size_t max_pairs = kAlignChunkPairs, size_t max_units = kAlignChunkUnits)
{
    c.pairs.clear();
    c.unit_offset.assign(1, 0u);
    size_t units = 0;
    for (; cur < n_list; cur++) {
        const uint32_t a = list[cur].a, b = list[cur].b;
        const uint32_t n = align_retimed_pair_units(first_a[a + 1] - first_a[a], first_b[b + 1] - first_b[b], num, den);
        if (!n) continue;
        if (!c.pairs.empty() && (c.pairs.size() >= max_pairs || units + n > max_units)) return true;
        c.pairs.push_back({a, b});
        units += n;
        c.unit_offset.push_back((uint32_t)units);
    }
    return !c.pairs.empty();
}

}  // namespace vdf
