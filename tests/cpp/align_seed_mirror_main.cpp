// host/vdf.hpp: VideoHash::align_seed_pairs, align_windows_pairs and align_windows_stretches_pairs on the CPU (tiny inputs and no context: the
// *_host forms) - a video, its re-upload with windows 14 ... 19 cut out, and an unrelated video that shares ONE window with the first, at a seed:
// the candidates hold the pair with the record and the pairs with the lone cell; the align calls on the candidates are the all-pairs calls; a
// sublist gives its part; skip bytes on the seeds; and the refusal of an unsorted list, of a video that does not exist and of a >= b.
#include <cstdio>
#include <random>

#include "vdf.hpp"

int main()
{
    std::mt19937_64 rng(2);
    std::vector<std::array<uint64_t, 16>> hs;
    for (int i = 0; i < 80; i++) {
        std::array<uint64_t, 16> h;
        for (auto &x : h) x = rng();
        h[15] &= (1ull << 40) - 1;
        hs.push_back(h);
    }
    std::vector<std::vector<vdf::VideoHash>> w(3);
    for (int i = 0; i < 30; i++) w[0].emplace_back(hs[i], "a", 1);
    for (int i = 0; i < 14; i++) w[1].emplace_back(hs[i], "b", 1);      // b: windows 0 .. 13 of a, then 20 .. 29, then 4 of its own
    for (int i = 20; i < 30; i++) w[1].emplace_back(hs[i], "b", 1);
    for (int i = 0; i < 4; i++) w[1].emplace_back(hs[40 + i], "b", 1);
    for (int i = 0; i < 12; i++) w[2].emplace_back(hs[50 + i], "c", 1);  // c: its own, but window 5 is window 9 of a - a seed at min_run 3
    w[2][5] = vdf::VideoHash(hs[9], "c", 1);
    int bad = 0;
    auto pairs_are = [&](const std::vector<vdf_video_pair> &p, std::vector<std::pair<uint32_t, uint32_t>> want) {
        bool ok = p.size() == want.size();
        for (size_t i = 0; ok && i < p.size(); i++) ok = p[i].a == want[i].first && p[i].b == want[i].second;
        if (!ok) { std::printf("unexpected: %zu pairs\n", p.size()); bad++; }
    };
    auto same = [&](const std::vector<vdf_alignment> &x, const std::vector<vdf_alignment> &y) {
        bool ok = x.size() == y.size();
        for (size_t i = 0; ok && i < x.size(); i++)
            ok = x[i].a == y[i].a && x[i].b == y[i].b && x[i].offset == y[i].offset && x[i].start_a == y[i].start_a && x[i].n_windows == y[i].n_windows &&
                 x[i].dist_sum == y[i].dist_sum;
        if (!ok) { std::printf("unexpected: %zu records for %zu\n", x.size(), y.size()); bad++; }
    };
    const auto cand = vdf::VideoHash::align_seed_pairs(w, nullptr, 350, 3);
    pairs_are(cand, {{0, 1}, {0, 2}, {1, 2}});                                    // (0, 2), (1, 2): the lone cell at ka = 9 of a and of its copy b
    pairs_are(vdf::VideoHash::align_seed_pairs(w, nullptr, 350, 4), {{0, 1}});    // ka = 9 is no seed at min_run 4
    const auto whole = vdf::VideoHash::align_windows(w, nullptr, 350, 3);
    if (whole.size() != 1 || whole[0].n_windows != 14) { std::printf("the all-pairs call: %zu records\n", whole.size()); bad++; }
    same(vdf::VideoHash::align_windows_pairs(w, nullptr, cand, 350, 3), whole);
    same(vdf::VideoHash::align_windows_pairs(w, nullptr, {{0, 2}, {1, 2}}, 350, 3), {});
    same(vdf::VideoHash::align_windows_pairs(w, nullptr, {}, 350, 3), {});
    const auto st = vdf::VideoHash::align_windows_stretches(w, nullptr, 350, 3, 4, 2), st_cand = vdf::VideoHash::align_windows_stretches_pairs(w, nullptr, cand, 350, 3, 4, 2);
    bool ok = st.size() == 2 && st_cand.size() == 2;
    for (size_t i = 0; ok && i < 2; i++)
        ok = st[i].a == st_cand[i].a && st[i].b == st_cand[i].b && st[i].offset == st_cand[i].offset && st[i].start_a == st_cand[i].start_a &&
             st[i].n_windows == st_cand[i].n_windows && st[i].rank == st_cand[i].rank;
    if (!ok) { std::printf("stretches on the candidates: %zu records for %zu\n", st_cand.size(), st.size()); bad++; }
    // two libraries, and skip bytes on every seed of the re-upload: its unskipped windows still match a, but no seed does
    const std::vector<std::vector<vdf::VideoHash>> a(w.begin(), w.begin() + 1), b(w.begin() + 1, w.end());
    pairs_are(vdf::VideoHash::align_seed_pairs(b, &a, 350, 3), {{0, 0}});         // c's window 5 is no seed of c
    std::vector<uint8_t> skip(40, 0);
    for (int k = 0; k < 28; k += 3) skip[k] = 1;
    pairs_are(vdf::VideoHash::align_seed_pairs(b, &a, 350, 3, &skip), {});
    for (const std::vector<vdf_video_pair> &list : {std::vector<vdf_video_pair>{{0, 2}, {0, 1}}, std::vector<vdf_video_pair>{{0, 1}, {0, 1}},
                                                    std::vector<vdf_video_pair>{{0, 3}}, std::vector<vdf_video_pair>{{1, 1}}, std::vector<vdf_video_pair>{{2, 1}}}) {
        try {
            vdf::VideoHash::align_windows_pairs(w, nullptr, list, 350, 3);
            bad++;
        } catch (const std::invalid_argument &) {
        }
        try {
            vdf::VideoHash::align_windows_stretches_pairs(w, nullptr, list, 350, 3);
            bad++;
        } catch (const std::invalid_argument &) {
        }
    }
    std::printf(bad ? "align seed mirror FAILED\n" : "align seed mirror ok\n");
    return bad;
}
