// host/vdf.hpp: VideoHash::align_seed_pairs_variants and align_windows_variants_pairs on the CPU (a tiny input and no context: the *_host forms) -
// video a holds ten windows of video b mirrored and reversed: the pair is a candidate under that flip only, the listed call gives the all-pairs
// call's record, a list that is out of order or names variant 0 is refused.
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
        for (int k = 0; k < 16; k++) { z[k] &= rng() & rng() & rng(); h[k] &= ~z[k]; }
        hb.push_back(h);
        zb.push_back(z);
    }
    const uint32_t flip = 5;
    std::vector<std::vector<vdf::VideoHash>> a(1), b(1);
    for (int i = 0; i < 20; i++) b[0].emplace_back(hb[i], "b", 1, zb[i]);
    for (int i = 0; i < 30; i++) {
        std::array<uint64_t, 16> h = random_hash();
        if (i >= 8 && i < 18) {
            const int src = 19 - (3 + (i - 8));
            if (vdf_hash_variant(hb[src].data(), zb[src].data(), flip, h.data()) != VDF_OK) return 2;
        }
        a[0].emplace_back(h, "a", 1, zb[0]);
    }
    int bad = 0;
    auto expect = [&](bool ok, const char *what) {
        if (!ok) { std::printf("unexpected: %s\n", what); bad++; }
    };
    const auto cand = vdf::VideoHash::align_seed_pairs_variants(a, &b, 350, {1, 4, flip, 7}, 2);
    expect(cand.size() == 1 && cand[0].a == 0 && cand[0].b == 0 && cand[0].variant == flip, "the candidates of two sets");
    expect(vdf::VideoHash::align_seed_pairs_variants(a, &b, 350, {1, 2, 3, 4, 6, 7}, 2).empty(), "a candidate under a flip that was not planted");
    const auto whole = vdf::VideoHash::align_windows_variants(a, &b, 350, {1, 4, flip, 7}, 2);
    const auto listed = vdf::VideoHash::align_windows_variants_pairs(a, &b, cand, 350, 2);
    expect(whole.size() == 1 && listed.size() == 1 && listed[0].a == whole[0].a && listed[0].b == whole[0].b && listed[0].offset == whole[0].offset &&
               listed[0].start_a == whole[0].start_a && listed[0].n_windows == whole[0].n_windows && listed[0].dist_sum == whole[0].dist_sum &&
               listed[0].variant == flip && listed[0].n_windows == 10 && listed[0].offset == -5,
           "the listed record");
    expect(vdf::VideoHash::align_windows_variants_pairs(a, &b, {{0, 0, 1}, {0, 0, 4}}, 350, 2).empty(), "a record under a listed flip that was not planted");
    expect(vdf::VideoHash::align_windows_variants_pairs(a, &b, {}, 350, 2).empty(), "an empty list");
    std::vector<std::vector<vdf::VideoHash>> both = {a[0], b[0]};
    const auto self = vdf::VideoHash::align_seed_pairs_variants(both, nullptr, 350, {flip}, 2);
    expect(self.size() == 1 && self[0].a == 0 && self[0].b == 1 && self[0].variant == flip, "the candidates in self mode");
    expect(vdf::VideoHash::align_windows_variants_pairs(both, nullptr, self, 350, 2).size() == 1, "the listed record in self mode");
    for (const std::vector<vdf_video_pair_variant> &list :
         {std::vector<vdf_video_pair_variant>{{0, 0, 4}, {0, 0, 1}}, std::vector<vdf_video_pair_variant>{{0, 0, 0}}, std::vector<vdf_video_pair_variant>{{0, 1, 5}}}) {
        try {
            vdf::VideoHash::align_windows_variants_pairs(a, &b, list, 350, 2);
            expect(false, "a bad list was taken");
        } catch (const std::invalid_argument &) {
        }
    }
    std::vector<std::vector<vdf::VideoHash>> plain(1);
    for (int i = 0; i < 20; i++) plain[0].emplace_back(hb[i], "b", 1);
    try {
        vdf::VideoHash::align_seed_pairs_variants(a, &plain, 350, {1});
        expect(false, "a flipped side without planes was taken");
    } catch (const vdf::Error &) {
    }
    try {
        vdf::VideoHash::align_seed_pairs_variants(a, &b, 350, {8});
        expect(false, "flip 8 was taken");
    } catch (const std::invalid_argument &) {
    }
    std::printf(bad ? "align seed variants mirror FAILED\n" : "align seed variants mirror ok\n");
    return bad;
}
