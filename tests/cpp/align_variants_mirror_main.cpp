// host/vdf.hpp: VideoHash::align_windows_variants on the CPU (a tiny input and no context: vdf_align_windows_variants_host) - video a holds ten
// windows of video b mirrored and reversed; two-set mode and self mode, the flips asked for and not asked for, a flipped side without zero
// planes, and vdf_window_variants_host through the C header.
#include <cstdio>
#include <random>

#include "vdf.hpp"

int main()
{
    std::mt19937_64 rng(2);
    auto random_hash = [&] {
        std::array<uint64_t, 16> h;
        for (auto &x : h) x = rng();
        h[15] &= (1ull << 40) - 1;
        return h;
    };
    std::vector<std::array<uint64_t, 16>> hb, zb;
    for (int i = 0; i < 20; i++) {
        std::array<uint64_t, 16> h = random_hash(), z = random_hash();
        for (int k = 0; k < 16; k++) { z[k] &= rng() & rng() & rng(); h[k] &= ~z[k]; }  // about an eighth of the coefficients exactly zero
        hb.push_back(h);
        zb.push_back(z);
    }
    const uint32_t flip = 5;  // mirrored along W and reversed in time
    std::vector<std::vector<vdf::VideoHash>> a(1), b(1);
    for (int i = 0; i < 20; i++) b[0].emplace_back(hb[i], "b", 1, zb[i]);
    for (int i = 0; i < 30; i++) {
        std::array<uint64_t, 16> h = random_hash();
        if (i >= 8 && i < 18) {  // derived row 3 + (i - 8) of b = its window 19 - that, flipped
            const int src = 19 - (3 + (i - 8));
            if (vdf_hash_variant(hb[src].data(), zb[src].data(), flip, h.data()) != VDF_OK) return 2;
        }
        a[0].emplace_back(h, "a", 1, zb[0]);
    }
    int bad = 0;
    auto is = [&](const std::vector<vdf_alignment_variant> &r, uint32_t va, uint32_t vb, int32_t off, uint32_t start, uint32_t n, uint32_t variant) {
        const bool ok = r.size() == 1 && r[0].a == va && r[0].b == vb && r[0].offset == off && r[0].start_a == start && r[0].n_windows == n && r[0].dist_sum == 0 &&
                        r[0].variant == variant;
        if (!ok) { std::printf("unexpected: %zu records\n", r.size()); bad++; }
    };
    is(vdf::VideoHash::align_windows_variants(a, &b, 350, {1, flip, 7}, 2), 0, 0, -5, 8, 10, flip);
    if (!vdf::VideoHash::align_windows_variants(a, &b, 350, {1, 2, 3, 4, 6, 7}, 2).empty()) { std::printf("found under a flip that was not planted\n"); bad++; }
    if (!vdf::VideoHash::align_windows(a, &b, 350, 2).empty()) { std::printf("found unflipped\n"); bad++; }
    std::vector<std::vector<vdf::VideoHash>> both = {a[0], b[0]};
    is(vdf::VideoHash::align_windows_variants(both, nullptr, 350, {flip}, 2), 0, 1, -5, 8, 10, flip);
    // the set's variant through the C header: row j of the derived b is what a holds at 8 + (j - 3)
    std::vector<uint64_t> words, zero, derived(20 * 16);
    for (int i = 0; i < 20; i++) { words.insert(words.end(), hb[i].begin(), hb[i].end()); zero.insert(zero.end(), zb[i].begin(), zb[i].end()); }
    const uint32_t first[2] = {0, 20};
    if (vdf_window_variants_host(words.data(), zero.data(), first, 1, nullptr, flip, derived.data(), nullptr) != VDF_OK) bad++;
    for (int j = 3; j < 13; j++)
        if (!std::equal(derived.begin() + 16 * j, derived.begin() + 16 * (j + 1), a[0][8 + j - 3].words().begin())) { std::printf("derived row %d\n", j); bad++; }
    std::vector<std::vector<vdf::VideoHash>> plain(1);
    for (int i = 0; i < 20; i++) plain[0].emplace_back(hb[i], "b", 1);
    try {
        vdf::VideoHash::align_windows_variants(a, &plain, 350, {1});
        bad++;
    } catch (const vdf::Error &) {
    }
    try {
        vdf::VideoHash::align_windows_variants(a, &b, 350, {8});
        bad++;
    } catch (const std::invalid_argument &) {
    }
    std::printf(bad ? "align variants mirror FAILED\n" : "align variants mirror ok\n");
    return bad;
}
