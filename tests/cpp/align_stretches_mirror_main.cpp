// host/vdf.hpp: VideoHash::align_windows_stretches on the CPU (a tiny input and no context: vdf_align_windows_stretches_host) - a video and its
// re-upload with windows 14 ... 19 cut out: two stretches at two offsets; self mode and two-library mode, max_stretches = 1 (align_windows'
// record), a stretch that the guard swallows, skip bytes, and the refusal of max_stretches = 0 and 9 and of a guard above 2^20.
#include <cstdio>
#include <random>

#include "vdf.hpp"

int main()
{
    std::mt19937_64 rng(2);
    std::vector<std::array<uint64_t, 16>> hs;
    for (int i = 0; i < 60; i++) {
        std::array<uint64_t, 16> h;
        for (auto &x : h) x = rng();
        h[15] &= (1ull << 40) - 1;
        hs.push_back(h);
    }
    std::vector<std::vector<vdf::VideoHash>> w(2);
    for (int i = 0; i < 30; i++) w[0].emplace_back(hs[i], "a", 1);
    // b: windows 0 .. 13 of a, then 20 .. 29 (14 .. 19 cut out), then 4 windows of its own
    for (int i = 0; i < 14; i++) w[1].emplace_back(hs[i], "b", 1);
    for (int i = 20; i < 30; i++) w[1].emplace_back(hs[i], "b", 1);
    for (int i = 0; i < 4; i++) w[1].emplace_back(hs[40 + i], "b", 1);
    int bad = 0;
    struct Want { uint32_t a, b; int32_t off; uint32_t start, n, rank; };
    auto is = [&](const std::vector<vdf_alignment_stretch> &r, std::vector<Want> want) {
        bool ok = r.size() == want.size();
        for (size_t i = 0; ok && i < r.size(); i++)
            ok = r[i].a == want[i].a && r[i].b == want[i].b && r[i].offset == want[i].off && r[i].start_a == want[i].start && r[i].n_windows == want[i].n &&
                 r[i].dist_sum == 0 && r[i].rank == want[i].rank;
        if (!ok) { std::printf("unexpected: %zu records\n", r.size()); bad++; }
    };
    is(vdf::VideoHash::align_windows_stretches(w, nullptr, 350, 2, 4, 2), {{0, 1, 0, 0, 14, 0}, {0, 1, -6, 20, 10, 1}});
    is(vdf::VideoHash::align_windows_stretches(w, nullptr, 350, 2, 1, 2), {{0, 1, 0, 0, 14, 0}});
    is(vdf::VideoHash::align_windows_stretches(w, nullptr, 350, 2, 4, 20), {{0, 1, 0, 0, 14, 0}});  // every row of a x every row of b: nothing is left
    const std::vector<std::vector<vdf::VideoHash>> a(w.begin(), w.begin() + 1), b(w.begin() + 1, w.end());
    is(vdf::VideoHash::align_windows_stretches(b, &a, 350, 2, 8, 0), {{0, 0, 0, 0, 14, 0}, {0, 0, 6, 14, 10, 1}});
    std::vector<uint8_t> skip(58, 0);
    skip[22] = 1;  // window 22 of video a: the second stretch falls into 20 .. 21 | 23 .. 29
    is(vdf::VideoHash::align_windows_stretches(w, nullptr, 350, 2, 4, 0, &skip), {{0, 1, 0, 0, 14, 0}, {0, 1, -6, 23, 7, 1}, {0, 1, -6, 20, 2, 2}});
    for (uint32_t ms : {0u, 9u}) {
        try {
            vdf::VideoHash::align_windows_stretches(w, nullptr, 350, 2, ms, 0);
            bad++;
        } catch (const std::invalid_argument &) {
        }
    }
    try {
        vdf::VideoHash::align_windows_stretches(w, nullptr, 350, 2, 4, (1u << 20) + 1);
        bad++;
    } catch (const std::invalid_argument &) {
    }
    std::printf(bad ? "align stretches mirror FAILED\n" : "align stretches mirror ok\n");
    return bad;
}
