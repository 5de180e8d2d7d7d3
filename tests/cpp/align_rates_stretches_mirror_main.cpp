// host/vdf.hpp: VideoHash::align_windows_rates_stretches_host on the CPU against the C call it wraps (vdf_align_windows_rates_stretches_host, the
// definition in plain C++).  Video b0 is a copy of a0 at 6/5 with a part cut out - windows 0, 6 .. 42 of a0's 6/5 block at its windows 0, 5 .. 35,
// windows 75, 81 .. 105 at its windows 50, 55 .. 75 - and b1 holds windows 3, 5, 7, 9 of a1's 2/1 block at its windows 2 .. 5.  Two rates in one
// call; the mirror's records must be the C call's on a job built here by hand, field for field, in all three triple modes, and hold both stretches.
#include <cstdio>
#include <random>

#include "vdf.hpp"

int main()
{
    std::mt19937_64 rng(5);
    auto noise = [&]() {
        std::array<uint64_t, 16> h;
        for (auto &x : h) x = rng();
        h[15] &= (1ull << 40) - 1;
        return h;
    };
    const int na0 = 112, na1 = 14, nb0 = 80, nb1 = 9;
    std::vector<std::vector<std::array<uint64_t, 16>>> block(2);   // [rate][window]: a0 then a1
    for (auto &b : block)
        for (int i = 0; i < na0 + na1; i++) b.push_back(noise());
    std::vector<std::array<uint64_t, 16>> b0(nb0), b1(nb1);
    for (auto &h : b0) h = noise();
    for (auto &h : b1) h = noise();
    for (int m = 0; m < 8; m++) b0[5 * m] = block[0][6 * m];
    for (int m = 0; m < 6; m++) b0[50 + 5 * m] = block[0][75 + 6 * m];
    for (int m = 0; m < 4; m++) b1[2 + m] = block[1][na0 + 3 + 2 * m];
    std::vector<std::vector<std::vector<vdf::VideoHash>>> A(2, std::vector<std::vector<vdf::VideoHash>>(2));
    std::vector<std::vector<vdf::VideoHash>> B(2);
    for (int r = 0; r < 2; r++)
        for (int i = 0; i < na0 + na1; i++) A[r][i < na0 ? 0 : 1].emplace_back(block[r][i], i < na0 ? "a0" : "a1", 1);
    for (const auto &h : b0) B[0].emplace_back(h, "b0", 1);
    for (const auto &h : b1) B[1].emplace_back(h, "b1", 1);
    const std::vector<std::pair<uint32_t, uint32_t>> rates = {{12, 10}, {2, 1}};

    // the C call on a job built by hand
    std::vector<uint64_t> wa, wb;
    for (int r = 0; r < 2; r++)
        for (const auto &h : block[r]) wa.insert(wa.end(), h.begin(), h.end());
    for (const auto &h : b0) wb.insert(wb.end(), h.begin(), h.end());
    for (const auto &h : b1) wb.insert(wb.end(), h.begin(), h.end());
    const uint32_t fa[6] = {0, (uint32_t)na0, (uint32_t)(na0 + na1), 0, (uint32_t)na0, (uint32_t)(na0 + na1)}, fb[3] = {0, (uint32_t)nb0, (uint32_t)(nb0 + nb1)};
    const size_t rate_first[3] = {0, (size_t)(na0 + na1), (size_t)(2 * (na0 + na1))};
    const uint32_t num[2] = {12, 2}, den[2] = {10, 1};
    int bad = 0;
    auto c_call = [&](uint32_t min_run, uint32_t most, uint32_t guard, const std::vector<vdf_video_pair_rate> *triples, bool seed, bool exclude_same) {
        std::vector<vdf_alignment_rate_stretch> out(64);
        size_t found = 0;
        static const vdf_video_pair_rate none{};
        const vdf_align_rates_stretches_job job{wa.data(), fa, rate_first, nullptr, 2, wb.data(), fb, nullptr, 2, 2, num, den, 350, min_run,
                                                triples ? (triples->empty() ? &none : triples->data()) : nullptr, triples ? triples->size() : 0, seed ? 1u : 0u,
                                                exclude_same ? 1u : 0u, most, guard, out.data(), out.size(), &found, nullptr};
        if (vdf_align_windows_rates_stretches_host(&job) != VDF_OK || found > out.size()) { std::printf("the C call failed\n"); bad++; found = 0; }
        out.resize(found);
        return out;
    };
    auto same = [&](const std::vector<vdf_alignment_rate_stretch> &got, const std::vector<vdf_alignment_rate_stretch> &want, const char *what) {
        bool ok = got.size() == want.size();
        for (size_t i = 0; ok && i < got.size(); i++)
            ok = got[i].a == want[i].a && got[i].b == want[i].b && got[i].rate == want[i].rate && got[i].first_a == want[i].first_a && got[i].first_b == want[i].first_b &&
                 got[i].n_windows == want[i].n_windows && got[i].dist_sum == want[i].dist_sum && got[i].n_frames_b == want[i].n_frames_b && got[i].rank == want[i].rank;
        if (!ok) { std::printf("%s: the mirror has %zu records, the C call %zu\n", what, got.size(), want.size()); bad++; }
    };
    const auto all = vdf::VideoHash::align_windows_rates_stretches_host(A, B, rates, 350, 2, 4, 15);
    same(all, c_call(2, 4, 15, nullptr, false, false), "all triples");
    // both stretches of the cut copy, then the 2/1 line
    const vdf_alignment_rate_stretch want[3] = {{0, 0, 0, 0, 0, 8, 0, 51, 0}, {0, 0, 0, 75, 50, 6, 0, 41, 1}, {1, 1, 1, 3, 2, 4, 0, 19, 0}};
    same(all, std::vector<vdf_alignment_rate_stretch>(want, want + 3), "the planted stretches");
    same(vdf::VideoHash::align_windows_rates_stretches_host(A, B, rates, 350, 2, 4, 15, nullptr, true), c_call(2, 4, 15, nullptr, true, false), "seeded");
    same(vdf::VideoHash::align_windows_rates_stretches_host(A, B, rates, 350, 2, 4, 15, nullptr, true), all, "seeded against unseeded");
    const std::vector<vdf_video_pair_rate> list = {{0, 0, 0}, {0, 1, 0}, {0, 0, 1}}, empty;
    same(vdf::VideoHash::align_windows_rates_stretches_host(A, B, rates, 350, 2, 4, 15, &list), c_call(2, 4, 15, &list, false, false), "listed");
    same(vdf::VideoHash::align_windows_rates_stretches_host(A, B, rates, 350, 2, 4, 15, &list), std::vector<vdf_alignment_rate_stretch>(want, want + 2), "listed: the copy");
    same(vdf::VideoHash::align_windows_rates_stretches_host(A, B, rates, 350, 2, 4, 15, &empty), {}, "an empty list");
    same(vdf::VideoHash::align_windows_rates_stretches_host(A, B, rates, 350, 2, 1, 15), c_call(2, 1, 15, nullptr, false, false), "max_stretches 1");
    same(vdf::VideoHash::align_windows_rates_stretches_host(A, B, rates, 350, 2, 1, 15), {want[0], want[2]}, "max_stretches 1: rank 0 alone");
    same(vdf::VideoHash::align_windows_rates_stretches_host(A, B, rates, 350, 1, 8, 0, nullptr, false, nullptr, nullptr, true), c_call(1, 8, 0, nullptr, false, true),
         "exclude_same, guard 0");
    for (int which = 0; which < 6; which++) {
        try {
            if (which == 0) vdf::VideoHash::align_windows_rates_stretches_host(A, B, rates, 350, 0);
            if (which == 1) vdf::VideoHash::align_windows_rates_stretches_host(A, B, rates, 350, 1, 0);
            if (which == 2) vdf::VideoHash::align_windows_rates_stretches_host(A, B, rates, 350, 1, 9);
            if (which == 3) vdf::VideoHash::align_windows_rates_stretches_host(A, B, rates, 350, 1, 4, (1u << 20) + 1);
            if (which == 4) vdf::VideoHash::align_windows_rates_stretches_host(A, B, rates, 350, 1, 4, 15, &list, true);      // a list together with seed
            if (which == 5) vdf::VideoHash::align_windows_rates_stretches_host(A, B, {{3, 2}, {5, 2}}, 350, 1);
            bad++;
        } catch (const std::invalid_argument &) {
        }
    }
    std::printf(bad ? "align rates stretches mirror FAILED\n" : "align rates stretches mirror ok\n");
    return bad;
}
