// Host-only check of what the flipped hashes rest on: the dense 16 x n table of i16 resize coefficients that
// csrc/resize_tables.cpp builds (the values before the i8 split) is its own mirror image, M[o][x] == M[15 - o][n - 1 - x], for
// every axis size n of the range given on the command line.  The comparison here is written out on its own, from build_axis_table's
// output, and must agree with the library's own predicate (axis_table_mirror_symmetric: what the planes calls ask before they run).
// Prints one line per asymmetric axis and a summary; exit code 1 if any axis fails or the two disagree.  Built with g++ (no HIP).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vid_dup_finder_lib_amd/csrc/resize_tables.h"

int main(int argc, char **argv)
{
    const unsigned lo = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1, hi = argc > 2 ? (unsigned)std::atoi(argv[2]) : 4200;
    unsigned bad = 0, disagree = 0;
    for (unsigned n = lo; n <= hi; n++) {
        std::vector<int> dense((size_t)16 * n, 0);
        if (n == 16) {
            for (unsigned o = 0; o < 16; o++) dense[(size_t)o * n + o] = 256;
        } else {
            vdf::HostAxisTable h;
            if (!vdf::build_axis_table(n, 16, h)) { std::printf("axis %u: no table\n", n); bad++; continue; }
            for (unsigned o = 0; o < 16; o++) {
                if (h.start[o] < 0 || h.size[o] < 0 || h.size[o] > h.window || (unsigned)(h.start[o] + h.size[o]) > n) { std::printf("axis %u: output %u out of range\n", n, o); bad++; continue; }
                for (int k = 0; k < h.size[o]; k++) dense[(size_t)o * n + (size_t)(h.start[o] + k)] = h.w[(size_t)o * h.window + (size_t)k];
            }
        }
        bool sym = true;
        for (unsigned o = 0; o < 16 && sym; o++)
            for (unsigned x = 0; x < n; x++)
                if (dense[(size_t)o * n + x] != dense[(size_t)(15 - o) * n + (n - 1 - x)]) {
                    std::printf("axis %u: M[%u][%u] = %d != M[%u][%u] = %d\n", n, o, x, dense[(size_t)o * n + x], 15 - o, n - 1 - x, dense[(size_t)(15 - o) * n + (n - 1 - x)]);
                    sym = false;
                    break;
                }
        if (!sym) bad++;
        if (sym != vdf::axis_table_mirror_symmetric(n)) { std::printf("axis %u: the library's predicate says %d\n", n, (int)!sym); disagree++; }
    }
    std::printf("axes %u..%u: %u asymmetric, %u disagreements\n", lo, hi, bad, disagree);
    return bad || disagree ? 1 : 0;
}
