// host/vdf.hpp: VideoHash::align_windows on the CPU (a tiny input and no context: vdf_align_windows_host) - two videos, the second holding ten
// windows of the first three windows later; self mode and two-library mode, skip bytes, and the refusal of min_run = 0.
#include <cstdio>
#include <random>

#include "vdf.hpp"

int main()
{
    std::mt19937_64 rng(1);
    std::vector<std::array<uint64_t, 16>> hs;
    for (int i = 0; i < 30; i++) {
        std::array<uint64_t, 16> h;
        for (auto &x : h) x = rng();
        h[15] &= (1ull << 40) - 1;
        hs.push_back(h);
    }
    std::vector<std::vector<vdf::VideoHash>> w(2);
    for (int i = 0; i < 30; i++) w[0].emplace_back(hs[i], "a", 1);
    for (int i = 0; i < 20; i++) w[1].emplace_back(i >= 5 && i < 15 ? hs[i + 3] : hs[(i * 7 + 1) % 5 + 25], "b", 1);
    int bad = 0;
    auto is = [&](const std::vector<vdf_alignment> &r, uint32_t a, uint32_t b, int32_t off, uint32_t start, uint32_t n) {
        const bool ok = r.size() == 1 && r[0].a == a && r[0].b == b && r[0].offset == off && r[0].start_a == start && r[0].n_windows == n && r[0].dist_sum == 0;
        if (!ok) { std::printf("unexpected: %zu records\n", r.size()); bad++; }
    };
    is(vdf::VideoHash::align_windows(w, nullptr, 350, 2), 0, 1, -3, 8, 10);
    const std::vector<std::vector<vdf::VideoHash>> a(w.begin(), w.begin() + 1), b(w.begin() + 1, w.end());
    is(vdf::VideoHash::align_windows(b, &a, 350, 2), 0, 0, 3, 5, 10);
    std::vector<uint8_t> skip(50, 0);
    skip[12] = 1;  // window 12 of video a: 8 .. 11 | 13 .. 17
    is(vdf::VideoHash::align_windows(w, nullptr, 350, 2, &skip), 0, 1, -3, 13, 5);
    try {
        vdf::VideoHash::align_windows(w, nullptr, 350, 0);
        bad++;
    } catch (const std::invalid_argument &) {
    }
    std::printf(bad ? "align mirror FAILED\n" : "align mirror ok\n");
    return bad;
}
