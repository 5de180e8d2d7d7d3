// Alignment of retimed windows at up to 8 rates in one call (vdf_align_windows_rates*): A holds one block of retimed windows per
// listed rate - rate-major, as vdf_hash_windows_clips_u8_rates* writes them - B plain windows, and the call walks (rate, a, b) TRIPLES: all of
// them, a caller-given list, or the candidates of vdf_align_seed_pairs_rates*.  Everything about one triple is align_retimed_plan.h's on block
// `rate` at that rate in lowest terms: the sub-matrices, the (phase, band) units in phase-major order, the two-level reduction.  This header adds
// what the rate list adds: the table the kernel reads a unit's rate from, and the chunks of a call, which may span rates - five rates with 20
// candidates each are one launch set, not five.  Host only, no HIP calls: api.cpp, align.hip (the launch side) and the CPU replay
// (tests/cpp/align_rates_plan_main.cpp) share one text.
#pragma once
#include <memory>
#include <utility>

#include "align_seed_rates_plan.h"

namespace vdf {

constexpr uint32_t kAlignRatesMax = kSeedRatesMax;   // = VDF_WINDOWS_MAX_RATES: slots of the table
constexpr uint64_t kAlignRatesMaxTriples = 1ull << 27;  // per call: 8 rates x kAlignMaxPairs

struct AlignRatesTriple { uint32_t a, b, rate; };    // vdf_video_pair_rate's layout: what the seed call writes goes to the kernel unchanged

// One slot of the table, 16 bytes: what a wave needs once it knows its unit's rate.  Window k of video i at slot r is row
// row0 + first_a[first_at + i] + k of the hashes the kernel sees (row0 = a_rate_first[r] minus what a host-array call has cut off in front of its
// upload, in 32-bit arithmetic: the sum is a row of the upload even where row0 alone wraps).
struct AlignRatesSlot { uint32_t num, den, row0, first_at; };
struct AlignRatesTable { AlignRatesSlot slot[kAlignRatesMax]; };

inline AlignRatesTable align_rates_table(const AlignSeedRate *rates, uint32_t n_rates, const size_t *rate_first, size_t n_a, uint64_t a_shift)
{
    AlignRatesTable t{};
    for (uint32_t r = 0; r < kAlignRatesMax; r++) {
        if (r < n_rates) t.slot[r] = AlignRatesSlot{rates[r].num, rates[r].den, (uint32_t)((rate_first ? (uint64_t)rate_first[r] : 0ull) - a_shift), (uint32_t)(r * (n_a + 1))};
        else t.slot[r] = AlignRatesSlot{1u, 1u, 0u, 0u};
    }
    return t;
}

// the units of triple (r, a, b): align_retimed_pair_units with the triple's own reduced rate on the window counts of block r
inline uint32_t align_rates_triple_units(const uint32_t *first_a, size_t n_a, const uint32_t *first_b, const AlignSeedRate *rates, uint32_t r, uint32_t a, uint32_t b)
{
    const uint32_t *fa = first_a + (size_t)r * (n_a + 1);
    return align_retimed_pair_units(fa[a + 1] - fa[a], first_b[b + 1] - first_b[b], rates[r].num, rates[r].den);
}

// A chunk: triples in (rate, a, b) order with at least one unit each, and their units - (triple, phase, band), phase-major inside the triple.
// The triples are written where they are uploaded from: `plan` holds the table's 32 dwords (filled by seal) and then 3 dwords per triple, and
// seal appends unit_offset behind them - the chunk's ONE upload, table | triples | unit_offset, with 4 bytes per triple copied on the host, not 16.
// A call over every triple of a library plans millions of them, and the planner is most of such a call's time: the two arrays are sized once per
// chunk for the most it can hold (begin) and written by index, and their allocator leaves new dwords unset instead of zeroing them.
constexpr size_t kAlignRatesPlanHead = sizeof(AlignRatesTable) / sizeof(uint32_t);
template <class T> struct AlignRatesUnset : std::allocator<T> {  // value-initialisation becomes default-initialisation: resize() does not write
    template <class U> struct rebind { typedef AlignRatesUnset<U> other; };
    template <class U> void construct(U *p) { ::new (static_cast<void *>(p)) U; }
    template <class U, class... A> void construct(U *p, A &&...a) { ::new (static_cast<void *>(p)) U(std::forward<A>(a)...); }
};
typedef std::vector<uint32_t, AlignRatesUnset<uint32_t>> AlignRatesWords;
struct AlignRatesChunk {
    AlignRatesWords plan;         // [32 + 3 triples (+ triples + 1 once sealed)]
    AlignRatesWords unit_offset;  // [triples + 1]
    size_t n = 0;                 // triples
    bool sealed = false;
    void clear() { begin(0); end(); }
    // room for at most `most` triples; push writes by index; end trims to what was pushed
    void begin(size_t most) { n = 0; sealed = false; plan.resize(kAlignRatesPlanHead + 3 * most); unit_offset.resize(most + 1); unit_offset[0] = 0u; }
    void push(uint32_t a, uint32_t b, uint32_t rate, uint32_t units_so_far)
    {
        uint32_t *t = plan.data() + kAlignRatesPlanHead + 3 * n;
        t[0] = a; t[1] = b; t[2] = rate;
        unit_offset[++n] = units_so_far;
    }
    void end() { plan.resize(kAlignRatesPlanHead + 3 * n); unit_offset.resize(n + 1); }
    size_t n_triples() const { return n; }
    bool empty() const { return n == 0; }
    AlignRatesTriple triple(size_t i) const { const uint32_t *t = plan.data() + kAlignRatesPlanHead + 3 * i; return AlignRatesTriple{t[0], t[1], t[2]}; }
    size_t n_units() const { return unit_offset.empty() ? 0 : unit_offset.back(); }
    size_t n_groups() const { return (n_units() + kAlignWaves - 1) / kAlignWaves; }
    // -> the upload (align_rates_plan_bytes(n_triples()) bytes at plan.data()); the chunk stays readable through triple() and unit_offset
    const void *seal(const AlignRatesTable &table)
    {
        static_assert(sizeof(AlignRatesTable) % sizeof(uint32_t) == 0 && sizeof(AlignRatesTriple) == 3 * sizeof(uint32_t), "the plan is counted in dwords");
        if (sealed) return plan.data();
        const uint32_t *t = reinterpret_cast<const uint32_t *>(&table);
        std::copy(t, t + kAlignRatesPlanHead, plan.begin());
        plan.insert(plan.end(), unit_offset.begin(), unit_offset.end());
        sealed = true;
        return plan.data();
    }
};
struct AlignRatesCursor { uint64_t r = 0, a = 0, b = 0; };

// All triples in (rate, a, b) order, without those with a == b under exclude_same; triples without a unit are skipped.  A chunk closes at
// max_pairs triples or max_units units (it always takes one triple), exactly as align_retimed_next_chunk closes - and goes on into the next rate.
// first_a: n_rates x (n_a + 1).  False once the triples are used up (c is then empty).
inline bool align_rates_next_chunk(const uint32_t *first_a, size_t n_a, const uint32_t *first_b, size_t n_b, const AlignSeedRate *rates, uint32_t n_rates,
                                   bool exclude_same, AlignRatesCursor &cur, AlignRatesChunk &c, size_t max_pairs = kAlignChunkPairs,
                                   size_t max_units = kAlignChunkUnits)
{
    const uint64_t left = cur.r < n_rates ? (uint64_t)(n_rates - cur.r) * n_a * n_b : 0;  // an upper bound of the triples still to come
    c.begin((size_t)std::min<uint64_t>(left, max_pairs ? max_pairs : 1));
    size_t units = 0, taken = 0;
    for (; cur.r < n_rates && n_a && n_b; cur.r++, cur.a = 0, cur.b = 0) {
        const uint32_t *fa = first_a + (size_t)cur.r * (n_a + 1);
        const uint32_t num = rates[cur.r].num, den = rates[cur.r].den;
        for (; cur.a < n_a; cur.a++, cur.b = 0) {
            const uint32_t Na = fa[cur.a + 1] - fa[cur.a];
            for (; cur.b < n_b; cur.b++) {
                if (exclude_same && cur.a == cur.b) continue;
                const uint32_t n = align_retimed_pair_units(Na, first_b[cur.b + 1] - first_b[cur.b], num, den);
                if (!n) continue;
                if (taken && (taken >= max_pairs || units + n > max_units)) { c.end(); return true; }
                units += n;
                taken++;
                c.push((uint32_t)cur.a, (uint32_t)cur.b, (uint32_t)cur.r, (uint32_t)units);
            }
        }
    }
    c.end();
    return taken != 0;
}

// the same fed from a checked list (align_rates_list_check); cur: the next list entry
template <class T>
inline bool align_rates_next_chunk_triples(const uint32_t *first_a, size_t n_a, const uint32_t *first_b, const T *list, size_t n_list, const AlignSeedRate *rates,
                                           size_t &cur, AlignRatesChunk &c, size_t max_pairs = kAlignChunkPairs, size_t max_units = kAlignChunkUnits)
{
    c.begin(std::min(n_list - std::min(cur, n_list), max_pairs ? max_pairs : 1));
    size_t units = 0, taken = 0;
    for (; cur < n_list; cur++) {
        const uint32_t n = align_rates_triple_units(first_a, n_a, first_b, rates, list[cur].rate, list[cur].a, list[cur].b);
        if (!n) continue;
        if (taken && (taken >= max_pairs || units + n > max_units)) { c.end(); return true; }
        units += n;
        taken++;
        c.push(list[cur].a, list[cur].b, list[cur].rate, (uint32_t)units);
    }
    c.end();
    return taken != 0;
}

// What a triple list must be - align_triple_list_check with the rate in the variant's place: strictly increasing in (rate, a, b), rate < n_rates,
// a < n_a, b < n_b.  0: fine; 1: not strictly increasing at *at (unsorted or a duplicate); 2: entry *at names a video that does not exist;
// 4: entry *at names a rate that is not in the list.
template <class T> inline int align_rates_list_check(const T *list, size_t n_list, size_t n_a, size_t n_b, uint32_t n_rates, size_t *at)
{
    for (size_t i = 0; i < n_list; i++) {
        *at = i;
        if (i) {
            const T &p = list[i - 1], &q = list[i];
            if (q.rate < p.rate || (q.rate == p.rate && (q.a < p.a || (q.a == p.a && q.b <= p.b)))) return 1;
        }
        if (list[i].rate >= n_rates) return 4;
        if (list[i].a >= n_a || list[i].b >= n_b) return 2;
    }
    return 0;
}

// the scratch of a chunk: 16 B per unit, 32 B + 32 B per triple (the triple records and the dense ones), the block counts and offsets, the total
inline size_t align_rates_scratch_bytes(size_t n_triples, size_t n_units)
{
    const size_t n_blocks = (n_triples + 255) / 256;
    return n_units * sizeof(AlignBandRecord) + 2 * n_triples * 32 + (2 * n_blocks + 4) * sizeof(uint32_t) + 64;
}

// the one upload of a chunk, in bytes: table | triples | unit_offset
inline size_t align_rates_plan_triples_at() { return sizeof(AlignRatesTable); }
inline size_t align_rates_plan_offsets_at(size_t n_triples) { return sizeof(AlignRatesTable) + n_triples * sizeof(AlignRatesTriple); }
inline size_t align_rates_plan_bytes(size_t n_triples) { return align_rates_plan_offsets_at(n_triples) + (n_triples + 1) * sizeof(uint32_t); }

}  // namespace vdf
