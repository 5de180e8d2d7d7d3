// The index rule of the variant of a set of window hashes (csrc/window_variant.h) replayed on the CPU, built with
// -fsanitize=address,undefined by tests/test_window_variant_rule.py.  The kernel (csrc/dct_hash.hip: window_variants_kernel) and the host twin
// (csrc/api.cpp) call the same function.  For first arrays with empty videos in every position (in front, in runs, at the end), one-window
// videos, sets that begin behind row 0 and the last video of the set, for every variant 0 ... 7 and every row of [first[0], first[n]):
//   - the source row lies in the video that owns the row - the array is exactly n + 1 entries long, so a read beyond it is the sanitizer's;
//   - without bit 2 it is the row itself, with bit 2 the row's mirror image within its video;
//   - per video the map is a bijection onto the video's rows, and applying it twice gives the row back.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "window_variant.h"

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

static unsigned long long replay(const std::vector<uint32_t> &counts, uint32_t row0)
{
    const uint32_t n = (uint32_t)counts.size();
    // a heap array of exactly n + 1 entries: one read past either end is reported
    uint32_t *first = new uint32_t[n + 1];
    first[0] = row0;
    for (uint32_t v = 0; v < n; v++) first[v + 1] = first[v] + counts[v];
    unsigned long long rows = 0;
    for (uint32_t variant = 0; variant < 8; variant++) {
        std::vector<uint32_t> hit(first[n] - row0, 0);
        for (uint32_t v = 0; v < n; v++)
            for (uint32_t j = 0; j < counts[v]; j++) {
                const uint32_t row = first[v] + j;
                const uint32_t src = window_variant_source(first, n, row, variant);
                CHECK(src >= first[v] && src < first[v + 1], "variant %u video %u of %u row %u: source %u outside [%u, %u)", variant, v, n, row, src, first[v],
                      first[v + 1]);
                CHECK(src == ((variant & 4u) ? first[v] + counts[v] - 1 - j : row), "variant %u video %u row %u: source %u", variant, v, row, src);
                CHECK(window_variant_source(first, n, src, variant) == row, "variant %u row %u: not an involution", variant, row);
                hit[src - row0]++;
                rows++;
            }
        for (size_t i = 0; i < hit.size(); i++) CHECK(hit[i] == 1, "variant %u: row %zu is the source of %u rows", variant, row0 + i, hit[i]);
    }
    delete[] first;
    return rows;
}

int main()
{
    unsigned long long rows = 0, sets = 0;
    const std::vector<std::vector<uint32_t>> shapes = {
        {1}, {5}, {0, 1}, {1, 0}, {0, 0, 3}, {3, 0, 0}, {0, 0, 1, 0, 0}, {1, 1, 1, 1}, {2, 0, 1, 0, 0, 7, 1}, {7, 1, 0}, {0, 64, 0, 65, 1, 0},
        {1, 0, 1, 0, 1, 0, 1}, {100, 1}, {1, 100}, {3, 3, 3, 3, 3, 3, 3, 3, 3}};
    for (const auto &counts : shapes)
        for (uint32_t row0 : {0u, 1u, 17u, 0xFFFFFF00u - 200u}) {  // (the last: rows near the top of the 32-bit range do not wrap)
            rows += replay(counts, row0);
            sets++;
        }
    // every set of up to 6 videos of 0 ... 2 windows: empty videos in every position, the last video empty or not
    for (uint32_t n = 1; n <= 6; n++) {
        uint32_t total = 1;
        for (uint32_t i = 0; i < n; i++) total *= 3;
        for (uint32_t code = 0; code < total; code++) {
            std::vector<uint32_t> counts(n);
            uint32_t c = code;
            bool any = false;
            for (uint32_t i = 0; i < n; i++) { counts[i] = c % 3; c /= 3; any |= counts[i] != 0; }
            if (!any) continue;  // a set without rows has no row to ask about
            rows += replay(counts, code % 5);
            sets++;
        }
    }
    std::printf("window variant rule ok: %llu sets, %llu (row, variant) checked\n", sets, rows);
    return 0;
}
