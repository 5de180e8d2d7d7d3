// The class-major layout of a window hash for the seeded alignment against the variants (include/vdf.h:
// vdf_align_seed_pairs_variants*).  ONE statement of the permutation for the kernels (align.hip: align_class_layout_kernel,
// align_seed_variants_kernel) and their host twin (api.cpp), replayed under the sanitizers by tests/cpp/window_class_layout_main.cpp.
// Host and device: plain C++, no HIP.
//   bit i = 100 kt + 10 kx + ky < 1000 of a hash has the CLASS c(i) = (kx & 1) | (ky & 1) << 1 | (kt & 1) << 2: 8 classes of 125 bits.
//   M_v (hash_variant.h) is constant on a class: 1 iff popcount(v & c) is odd.  Bits 1000 ... 1023 are a ninth group that no mask touches.
//   A row of the layout is 33 dwords: the never-flipped group - class 0 at bits 0 ... 124, bits 1000 ... 1023 at 125 ... 148 - in dwords
//   0 ... 4, class c = 1 ... 7 at bits 0 ... 124 of dwords 5 + 4 (c - 1) ... 8 + 4 (c - 1).  The 32 positions no bit maps to stay 0.
//   Inside a class the bits keep their order: rank r = 25 (kt >> 1) + 5 (kx >> 1) + (ky >> 1).
// The distance identity (all words arbitrary: padding bits set, bits set in Z, H & Z != 0), with nZ = ~Z, Hz = H & nZ, t = A & nZ, u = t ^ Hz:
//   d(A, (H ^ M_v) & ~Z) = popcount(A) - popcount(t) + popcount(u | group 0) + sum over c = 1 ... 7 of
//                          (popcount(v & c) odd ? popcount(nZ | c) - popcount(u | c) : popcount(u | c))
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VDF_CLASS_LAYOUT_HD __host__ __device__
#else
#define VDF_CLASS_LAYOUT_HD
#endif

namespace vdf {

constexpr uint32_t kClassDwords = 33;        // the permuted bits of a row
constexpr uint32_t kClassGroup0Dwords = 5;   // class 0 + the 24 padding bits: 149 bits
constexpr uint32_t kClassDwordsPer = 4;      // classes 1 ... 7: 125 bits each
constexpr uint32_t kClassNone = 0xFFFFFFFFu;
// Rows as the kernels read them, in dwords.  A seed: [0, 33) its bits, 33 popcount of all 1024 bits, 34 its skip byte, 35 its video.
// A row of B: [0, 33) Hz, 33 / 34 the live counts popcount(nZ | c) of classes 1 ... 4 / 5 ... 7, one byte each from the low byte up,
// 35 its skip byte, [36, 69) nZ, 69 ... 71 zero.  Both strides are multiples of 16 bytes.
constexpr uint32_t kClassSeedStride = 36, kClassRowStride = 72, kClassRowNz = 36;

VDF_CLASS_LAYOUT_HD constexpr uint32_t window_class_of(uint32_t i)  // i < 1000
{
    const uint32_t kt = i / 100, kx = (i / 10) % 10, ky = i % 10;
    return (kx & 1u) | (ky & 1u) << 1 | (kt & 1u) << 2;
}

// bit i < 1024 of a hash -> its position among the 33 x 32 bits of the layout
VDF_CLASS_LAYOUT_HD inline uint32_t window_class_dest(uint32_t i)
{
    if (i >= 1000) return 125 + (i - 1000);
    const uint32_t kt = i / 100, kx = (i / 10) % 10, ky = i % 10;
    const uint32_t c = window_class_of(i), r = 25 * (kt >> 1) + 5 * (kx >> 1) + (ky >> 1);
    return c == 0 ? r : 32 * (kClassGroup0Dwords + kClassDwordsPer * (c - 1)) + r;
}

// position p < 33 x 32 of the layout -> the bit of the hash that lands there, kClassNone for the 32 positions that stay 0
VDF_CLASS_LAYOUT_HD constexpr uint32_t window_class_source(uint32_t p)
{
    uint32_t c = 0, r = p;
    if (p >= 32 * kClassGroup0Dwords) {
        c = (p - 32 * kClassGroup0Dwords) / (32 * kClassDwordsPer) + 1;
        r = (p - 32 * kClassGroup0Dwords) % (32 * kClassDwordsPer);
    } else if (p >= 125) {
        return p < 149 ? 1000 + (p - 125) : kClassNone;
    }
    if (r >= 125) return kClassNone;
    const uint32_t kt = 2 * (r / 25) + (c >> 2 & 1u), kx = 2 * ((r / 5) % 5) + (c & 1u), ky = 2 * (r % 5) + (c >> 1 & 1u);
    return 100 * kt + 10 * kx + ky;
}

// the class (0: the never-flipped group) that dword q < 33 of the layout belongs to
VDF_CLASS_LAYOUT_HD inline uint32_t window_class_of_dword(uint32_t q)
{
    return q < kClassGroup0Dwords ? 0 : (q - kClassGroup0Dwords) / kClassDwordsPer + 1;
}

// does variant v flip class c?
VDF_CLASS_LAYOUT_HD inline bool window_class_flipped(uint32_t v, uint32_t c)
{
    const uint32_t x = v & c;
    return ((x ^ x >> 1 ^ x >> 2) & 1u) != 0;
}

// The same rule as tables, made from the functions above at compile time: src[p] = window_class_source(p) (0xFFFF: none), and mask[c] = the
// bits of class c = 1 ... 7 in a hash's own 32 dwords.  The layout kernel reads them from device memory instead of recomputing a position
// by integer divisions for every bit it moves; the functions below take them as optional arguments and are the same functions without.
struct ClassTables {
    uint16_t src[32 * kClassDwords];
    uint32_t mask[8][32];
};
constexpr ClassTables make_class_tables()
{
    ClassTables t{};
    for (uint32_t p = 0; p < 32 * kClassDwords; p++) t.src[p] = (uint16_t)(window_class_source(p) == kClassNone ? 0xFFFFu : window_class_source(p));
    for (uint32_t i = 0; i < 1000; i++) t.mask[window_class_of(i)][i >> 5] |= 1u << (i & 31);
    return t;
}
inline constexpr ClassTables kClassTables = make_class_tables();

// dword q < 33 of the layout of a row of 32 dwords (bit i of the hash = bit i & 31 of dword i >> 5)
VDF_CLASS_LAYOUT_HD inline uint32_t window_class_dword(const uint32_t *row, uint32_t q, bool invert = false, const ClassTables *tables = nullptr)
{
    uint32_t out = 0;
    for (uint32_t k = 0; k < 32; k++) {
        const uint32_t i = tables ? (tables->src[32 * q + k] == 0xFFFFu ? kClassNone : tables->src[32 * q + k]) : window_class_source(32 * q + k);
        if (i == kClassNone) continue;
        const uint32_t w = invert ? ~row[i >> 5] : row[i >> 5];
        out |= (w >> (i & 31) & 1u) << k;
    }
    return out;
}

// dword q < 36 of a seed's row: hash = the window's 32 dwords
VDF_CLASS_LAYOUT_HD inline uint32_t window_class_seed_dword(const uint32_t *hash, uint32_t skip, uint32_t video, uint32_t q, const ClassTables *tables = nullptr)
{
    if (q < kClassDwords) return window_class_dword(hash, q, false, tables);
    if (q == 34) return skip ? 1u : 0u;
    if (q == 35) return video;
    uint32_t n = 0;
    for (uint32_t w = 0; w < 32; w++) n += (uint32_t)__builtin_popcount(hash[w]);
    return n;
}

// dword q < 72 of a row of B: hash and zero = the window's 32 dwords each
VDF_CLASS_LAYOUT_HD inline uint32_t window_class_row_dword(const uint32_t *hash, const uint32_t *zero, uint32_t skip, uint32_t q,
                                                           const ClassTables *tables = nullptr)
{
    if (q < kClassDwords) return window_class_dword(hash, q, false, tables) & window_class_dword(zero, q, true, tables);
    if (q >= kClassRowNz) return q < kClassRowNz + kClassDwords ? window_class_dword(zero, q - kClassRowNz, true, tables) : 0u;
    if (q == 35) return skip ? 1u : 0u;
    uint32_t packed = 0;  // q == 33: classes 1 ... 4, q == 34: classes 5 ... 7
    for (uint32_t c = (q == 33 ? 1 : 5); c <= (q == 33 ? 4u : 7u); c++) {
        uint32_t live = 0;  // popcount(nZ | c): counted in the layout, or - the same bits - in the hash's own dwords under the class's mask
        if (tables) {
            for (uint32_t w = 0; w < 32; w++) live += (uint32_t)__builtin_popcount(~zero[w] & tables->mask[c][w]);
        } else {
            for (uint32_t k = 0; k < kClassDwordsPer; k++)
                live += (uint32_t)__builtin_popcount(window_class_dword(zero, kClassGroup0Dwords + kClassDwordsPer * (c - 1) + k, true));
        }
        packed |= live << (8 * ((c - 1) & 3u));
    }
    return packed;
}

// d(A, (H ^ M_v) & ~Z) from a seed's row and a row of B in the layout above: the identity, as the seed kernel evaluates it
VDF_CLASS_LAYOUT_HD inline uint32_t window_class_distance(const uint32_t *seed, const uint32_t *row, uint32_t v)
{
    uint32_t sub = 0, acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t q = 0; q < kClassDwords; q++) {
        const uint32_t t = seed[q] & row[kClassRowNz + q], u = t ^ row[q];
        sub += (uint32_t)__builtin_popcount(t);
        acc[window_class_of_dword(q)] += (uint32_t)__builtin_popcount(u);
    }
    uint32_t d = seed[33] - sub + acc[0];
    for (uint32_t c = 1; c < 8; c++) {
        const uint32_t live = row[33 + ((c - 1) >> 2)] >> (8 * ((c - 1) & 3u)) & 0xFFu;
        d += window_class_flipped(v, c) ? live - acc[c] : acc[c];
    }
    return d;
}

}  // namespace vdf
