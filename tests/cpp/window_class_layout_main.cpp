// Replays csrc/window_class_layout.h (the class-major layout of the seeded alignment against the variants) on the CPU, built
// with -fsanitize=address,undefined by tests/test_window_class_layout.py:
//   - the permutation maps the 1024 bits of a hash one to one into the 33 x 32 positions, and window_class_source is its inverse; exactly 32
//     positions stay empty;
//   - the classes are where the header says: group 0 = class 0 + bits 1000 ... 1023 in dwords 0 ... 4, class c in dwords 5 + 4 (c - 1) ...,
//     125 bits each, and M_v (hash_variant.h) is constant on a class with the value window_class_flipped(v, c);
//   - the distance identity: window_class_distance on the rows the layout functions make equals the brute-force distance to the row
//     (H ^ M_v) & ~Z - the rule of vdf_window_variants_host - for all 7 variants over random and adversarial words: padding bits set in A,
//     in H, in Z, H & Z != 0, all ones, all zeros, single bits, one class only;
//   - the tables the layout kernel reads (kClassTables) say what the functions say, and the table-driven forms give the same words;
//   - the bound the seed kernel exits on is never above the smallest distance to a requested variant, for every mask, and is that distance
//     itself when one variant is requested.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "hash_variant.h"
#include "window_class_layout.h"

#define CHECK(c)                                                                \
    do {                                                                        \
        if (!(c)) {                                                             \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);                  \
            return 1;                                                           \
        }                                                                       \
    } while (0)

using namespace vdf;

static uint32_t brute(const uint32_t *a, const uint32_t *h, const uint32_t *z, uint32_t v)
{
    uint32_t d = 0;
    for (int w = 0; w < 32; w++) {
        const uint64_t m64 = kVariantMasks.m[v][w >> 1];
        const uint32_t m = (uint32_t)(w & 1 ? m64 >> 32 : m64);
        d += (uint32_t)__builtin_popcount(a[w] ^ ((h[w] ^ m) & ~z[w]));
    }
    return d;
}

static int check_words(const uint32_t *a, const uint32_t *h, const uint32_t *z)
{
    std::vector<uint32_t> seed(kClassSeedStride), row(kClassRowStride);
    for (uint32_t q = 0; q < kClassSeedStride; q++) seed[q] = window_class_seed_dword(a, 0, 7, q);
    for (uint32_t q = 0; q < kClassRowStride; q++) row[q] = window_class_row_dword(h, z, 3, q);
    // the table-driven forms the layout kernel uses give the same words
    for (uint32_t q = 0; q < kClassSeedStride; q++) CHECK(seed[q] == window_class_seed_dword(a, 0, 7, q, &kClassTables));
    for (uint32_t q = 0; q < kClassRowStride; q++) CHECK(row[q] == window_class_row_dword(h, z, 3, q, &kClassTables));
    CHECK(seed[34] == 0 && seed[35] == 7 && row[35] == 1 && row[69] == 0 && row[70] == 0 && row[71] == 0);
    uint32_t dmin = 0xFFFFFFFFu;
    for (uint32_t v = 1; v < 8; v++) {
        const uint32_t want = brute(a, h, z, v), got = window_class_distance(seed.data(), row.data(), v);
        if (want != got) std::printf("variant %u: identity %u, brute force %u\n", v, got, want);
        CHECK(want == got);
        dmin = want < dmin ? want : dmin;
    }
    // the exit bound, as the kernel forms it
    uint32_t sub = 0, acc[8] = {0};
    for (uint32_t q = 0; q < kClassDwords; q++) {
        const uint32_t t = seed[q] & row[kClassRowNz + q];
        sub += (uint32_t)__builtin_popcount(t);
        acc[window_class_of_dword(q)] += (uint32_t)__builtin_popcount(t ^ row[q]);
    }
    CHECK(seed[33] >= sub);
    uint32_t bound = seed[33] - sub + acc[0];
    for (uint32_t c = 1; c < 8; c++) {
        const uint32_t live = row[33 + ((c - 1) >> 2)] >> (8 * ((c - 1) & 3)) & 0xFFu;
        CHECK(live <= 125 && acc[c] <= live);
        bound += acc[c] < live - acc[c] ? acc[c] : live - acc[c];
    }
    CHECK(bound <= dmin);
    // ... and the bound over the REQUESTED variants as align_seed_variants_kernel forms it: never above a requested distance, never below the
    // all-variants bound, and with one variant requested that variant's distance itself
    for (uint32_t mask = 2; mask < 256; mask += 2) {
        uint32_t flip_any = 0, keep_any = 0, want = 0xFFFFFFFFu, n = 0;
        for (uint32_t v = 1; v < 8; v++) {
            if (!(mask >> v & 1u)) continue;
            n++;
            const uint32_t d = window_class_distance(seed.data(), row.data(), v);
            want = d < want ? d : want;
            for (uint32_t c = 1; c < 8; c++) (window_class_flipped(v, c) ? flip_any : keep_any) |= 1u << c;
        }
        uint32_t b = seed[33] - sub + acc[0];
        for (uint32_t c = 1; c < 8; c++) {
            const uint32_t live = row[33 + ((c - 1) >> 2)] >> (8 * ((c - 1) & 3)) & 0xFFu, kept = acc[c], flipped = live - acc[c];
            b += (flip_any >> c & 1u) ? ((keep_any >> c & 1u) ? (kept < flipped ? kept : flipped) : flipped) : kept;
        }
        CHECK(b <= want && b >= bound && (n != 1 || b == want));
    }
    return 0;
}

int main()
{
    // the permutation
    std::vector<int> hit(32 * kClassDwords, 0);
    for (uint32_t i = 0; i < 1024; i++) {
        const uint32_t p = window_class_dest(i);
        CHECK(p < 32 * kClassDwords);
        hit[p]++;
        CHECK(window_class_source(p) == i);
        const uint32_t c = i < 1000 ? window_class_of(i) : 0;
        CHECK(window_class_of_dword(p >> 5) == c);
        if (c == 0) CHECK(p < 149 && (i < 1000) == (p < 125));
        else CHECK(p >= 32 * (5 + 4 * (c - 1)) && p < 32 * (5 + 4 * (c - 1)) + 125);
        for (uint32_t v = 0; v < 8; v++) {
            const bool m = (kVariantMasks.m[v][i >> 6] >> (i & 63) & 1u) != 0;
            CHECK(m == (i < 1000 && window_class_flipped(v, c)));
        }
    }
    uint32_t empty = 0;
    for (uint32_t p = 0; p < 32 * kClassDwords; p++) {
        CHECK(hit[p] <= 1);
        if (!hit[p]) { empty++; CHECK(window_class_source(p) == kClassNone); }
    }
    CHECK(empty == 32);
    for (uint32_t p = 0; p < 32 * kClassDwords; p++) CHECK(kClassTables.src[p] == (window_class_source(p) == kClassNone ? 0xFFFFu : window_class_source(p)));
    for (uint32_t c = 0; c < 8; c++)
        for (uint32_t i = 0; i < 1024; i++) CHECK((kClassTables.mask[c][i >> 5] >> (i & 31) & 1u) == (i < 1000 && window_class_of(i) == c ? 1u : 0u));
    uint32_t per_class[8] = {0};
    for (uint32_t i = 0; i < 1000; i++) per_class[window_class_of(i)]++;
    for (uint32_t c = 0; c < 8; c++) CHECK(per_class[c] == 125);
    CHECK(kClassSeedStride % 4 == 0 && kClassRowStride % 4 == 0 && kClassRowNz % 4 == 0);

    // the identity
    std::mt19937_64 rng(20260419);
    uint32_t a[32], h[32], z[32];
    auto fill = [&](uint32_t *w, int kind) {
        for (int k = 0; k < 32; k++) {
            const uint32_t r = (uint32_t)rng();
            w[k] = kind == 0 ? r : kind == 1 ? r & (uint32_t)rng() & (uint32_t)rng() : kind == 2 ? 0xFFFFFFFFu : kind == 3 ? 0u : r | (uint32_t)rng();
        }
    };
    long cases = 0;
    for (int ka = 0; ka < 5; ka++)
        for (int kh = 0; kh < 5; kh++)
            for (int kz = 0; kz < 5; kz++)
                for (int rep = 0; rep < 40; rep++) {
                    fill(a, ka); fill(h, kh); fill(z, kz);  // arbitrary words: padding bits anywhere, H & Z != 0
                    if (check_words(a, h, z)) return 1;
                    cases++;
                }
    // single bits of A, H and Z at every position, against random rows
    for (uint32_t i = 0; i < 1024; i++) {
        for (int which = 0; which < 3; which++) {
            fill(a, 0); fill(h, 0); fill(z, 1);
            uint32_t *w = which == 0 ? a : which == 1 ? h : z;
            for (int k = 0; k < 32; k++) w[k] = 0;
            w[i >> 5] = 1u << (i & 31);
            if (check_words(a, h, z)) return 1;
            cases++;
        }
    }
    // one class only live, one class only dead; the padding bits set in A only, in H only, in both, and in Z
    for (uint32_t c = 0; c < 8; c++)
        for (int dead = 0; dead < 2; dead++) {
            fill(a, 0); fill(h, 0);
            for (int k = 0; k < 32; k++) z[k] = dead ? 0u : 0xFFFFFFFFu;
            for (uint32_t i = 0; i < 1000; i++)
                if (window_class_of(i) == c) z[i >> 5] ^= 1u << (i & 31);
            if (check_words(a, h, z)) return 1;
            cases++;
        }
    for (int pa = 0; pa < 2; pa++)
        for (int ph = 0; ph < 2; ph++)
            for (int pz = 0; pz < 2; pz++) {
                fill(a, 0); fill(h, 0); fill(z, 1);
                a[31] = (a[31] & 0xFFu) | (pa ? 0xFFFFFF00u : 0u);
                h[31] = (h[31] & 0xFFu) | (ph ? 0xFFFFFF00u : 0u);
                z[31] = (z[31] & 0xFFu) | (pz ? 0xFFFFFF00u : 0u);
                if (check_words(a, h, z)) return 1;
                cases++;
            }
    std::printf("window class layout ok: %ld word triples x 7 variants\n", cases);
    return 0;
}
