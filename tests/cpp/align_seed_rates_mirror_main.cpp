// host/vdf.hpp: VideoHash::align_seed_pairs_rates_host on the CPU (vdf_align_seed_pairs_rates_host, the definition in plain C++) - video b0 holds
// windows 4, 7, 10, ... of a0's 3/2 block at its windows 0, 2, 4, ... and window 9 of a1's 2/1 block at its window 1; b1 is unrelated.  Two rates in
// one call, each with its slot; a skip byte, min_run, exclude_same and the refusals.
#include <cstdio>
#include <random>

#include "vdf.hpp"

int main()
{
    std::mt19937_64 rng(3);
    auto noise = [&]() {
        std::array<uint64_t, 16> h;
        for (auto &x : h) x = rng();
        h[15] &= (1ull << 40) - 1;
        return h;
    };
    std::vector<std::vector<std::array<uint64_t, 16>>> block(2, std::vector<std::array<uint64_t, 16>>());   // [rate][window]: a0 (40 windows) then a1 (12)
    for (auto &b : block)
        for (int i = 0; i < 52; i++) b.push_back(noise());
    std::vector<std::array<uint64_t, 16>> b0(20);
    for (int j = 0; j < 20; j++) b0[j] = (j % 2 == 0 && 4 + 3 * (j / 2) < 40) ? block[0][4 + 3 * (j / 2)] : noise();
    b0[1] = block[1][40 + 9];
    std::vector<std::vector<std::vector<vdf::VideoHash>>> A(2, std::vector<std::vector<vdf::VideoHash>>(2));
    std::vector<std::vector<vdf::VideoHash>> B(2);
    for (int r = 0; r < 2; r++)
        for (int i = 0; i < 52; i++) A[r][i < 40 ? 0 : 1].emplace_back(block[r][i], i < 40 ? "a0" : "a1", 1);
    for (const auto &h : b0) B[0].emplace_back(h, "b0", 1);
    for (int j = 0; j < 9; j++) B[1].emplace_back(noise(), "b1", 1);
    const std::vector<std::pair<uint32_t, uint32_t>> rates = {{6, 4}, {2, 1}};
    int bad = 0;
    auto is = [&](const std::vector<vdf_video_pair_rate> &got, const std::vector<vdf_video_pair_rate> &want) {
        bool ok = got.size() == want.size();
        for (size_t i = 0; ok && i < got.size(); i++) ok = got[i].a == want[i].a && got[i].b == want[i].b && got[i].rate == want[i].rate;
        if (!ok) { std::printf("unexpected: %zu triples\n", got.size()); bad++; }
    };
    // 3/2: the seeds of a0 at min_run 2 are ka = 0 .. 2, 6 .. 8, ...: 7 matches window 2 of b0.  2/1: window 9 of a1 is a seed ((9 / 2) % 2 == 0)
    is(vdf::VideoHash::align_seed_pairs_rates_host(A, B, rates, 350, 2), {{0, 0, 0}, {1, 0, 1}});
    is(vdf::VideoHash::align_seed_pairs_rates_host(A, B, rates, 350, 2, nullptr, nullptr, true), {{1, 0, 1}});   // exclude_same: (0, 0) goes
    is(vdf::VideoHash::align_seed_pairs_rates_host(A, B, rates, 350, 3), {{0, 0, 0}});                           // (9 / 2) % 3 != 0
    std::vector<uint8_t> skip_a(104, 0);
    skip_a[52 + 40 + 9] = 1;  // rate-major: block 1, video a1, window 9
    is(vdf::VideoHash::align_seed_pairs_rates_host(A, B, rates, 350, 2, &skip_a), {{0, 0, 0}});
    is(vdf::VideoHash::align_seed_pairs_rates_host({A[1]}, B, {{2, 1}}, 350, 1), {{1, 0, 0}});
    for (int which = 0; which < 5; which++) {
        try {
            if (which == 0) vdf::VideoHash::align_seed_pairs_rates_host(A, B, rates, 350, 0);
            if (which == 1) vdf::VideoHash::align_seed_pairs_rates_host(A, B, {{3, 2}, {5, 2}}, 350, 1);
            if (which == 2) vdf::VideoHash::align_seed_pairs_rates_host(A, B, {{33, 32}, {1, 1}}, 350, 1);
            if (which == 3) vdf::VideoHash::align_seed_pairs_rates_host(A, B, {{3, 2}}, 350, 1);       // one set of windows per rate
            if (which == 4) vdf::VideoHash::align_seed_pairs_rates_host({}, B, {}, 350, 1);            // no rate
            bad++;
        } catch (const std::invalid_argument &) {
        }
    }
    std::printf(bad ? "align seed rates mirror FAILED\n" : "align seed rates mirror ok\n");
    return bad;
}
