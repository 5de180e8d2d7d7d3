// host/vdf.hpp: VideoHash::align_windows_retimed[_pairs] on the CPU (a tiny input and no context: vdf_align_windows_retimed[_pairs]_host) - video b0
// holds windows 4, 7, 10, ... of a0 at its windows 0, 2, 4, ... (rate 3/2, phase 1 from i0 = 1), b1 is unrelated; the pair list, a skip byte that
// cuts the run, a rate that is not in lowest terms, and the refusals.
#include <cstdio>
#include <random>

#include "vdf.hpp"

int main()
{
    std::mt19937_64 rng(2);
    auto noise = [&]() {
        std::array<uint64_t, 16> h;
        for (auto &x : h) x = rng();
        h[15] &= (1ull << 40) - 1;
        return h;
    };
    std::vector<std::array<uint64_t, 16>> a0, b0(20);
    for (int i = 0; i < 40; i++) a0.push_back(noise());
    for (int j = 0; j < 20; j++) b0[j] = (j % 2 == 0 && 4 + 3 * (j / 2) < 40) ? a0[4 + 3 * (j / 2)] : noise();  // j = 0 .. 18: ten cells
    std::vector<std::vector<vdf::VideoHash>> A(1), B(2);
    for (const auto &h : a0) A[0].emplace_back(h, "a0", 1);
    for (const auto &h : b0) B[0].emplace_back(h, "b0", 1);
    for (int j = 0; j < 9; j++) B[1].emplace_back(noise(), "b1", 1);
    int bad = 0;
    auto is = [&](const std::vector<vdf_alignment_retimed> &r, uint32_t first_a, uint32_t first_b, uint32_t n) {
        const bool ok = r.size() == 1 && r[0].a == 0 && r[0].b == 0 && r[0].first_a == first_a && r[0].first_b == first_b && r[0].n_windows == n && r[0].dist_sum == 0;
        if (!ok) { std::printf("unexpected: %zu records\n", r.size()); bad++; }
    };
    is(vdf::VideoHash::align_windows_retimed(A, B, 3, 2, 350, 2), 4, 0, 10);
    is(vdf::VideoHash::align_windows_retimed(A, B, 6, 4, 350, 2), 4, 0, 10);
    is(vdf::VideoHash::align_windows_retimed_pairs(A, B, {{0, 0}}, 3, 2, 350, 2), 4, 0, 10);
    if (!vdf::VideoHash::align_windows_retimed_pairs(A, B, {{0, 1}}, 3, 2, 350, 2).empty()) bad++;
    if (!vdf::VideoHash::align_windows_retimed_pairs(A, B, {}, 3, 2, 350, 2).empty()) bad++;
    std::vector<uint8_t> skip_b(29, 0);
    skip_b[6] = 1;  // window 6 of b0, cell 3 of the run: 0 .. 2 | 4 .. 9
    is(vdf::VideoHash::align_windows_retimed(A, B, 3, 2, 350, 2, nullptr, &skip_b), 4 + 3 * 4, 8, 6);
    for (int which = 0; which < 4; which++) {
        try {
            if (which == 0) vdf::VideoHash::align_windows_retimed(A, B, 3, 2, 350, 0);
            if (which == 1) vdf::VideoHash::align_windows_retimed(A, B, 5, 2, 350, 1);
            if (which == 2) vdf::VideoHash::align_windows_retimed(A, B, 33, 32, 350, 1);
            if (which == 3) vdf::VideoHash::align_windows_retimed_pairs(A, B, {{0, 1}, {0, 0}}, 3, 2, 350, 1);
            bad++;
        } catch (const std::invalid_argument &) {
        }
    }
    std::printf(bad ? "align retimed mirror FAILED\n" : "align retimed mirror ok\n");
    return bad;
}
