// align_seed_check_words (csrc/align_plan.h) for every tolerance 0 ... 1024, one number each: tests/test_align_fuzz_host.py holds
// tests/alignfuzz.py's restatement - and the edges in its tolerance list - against it.
#include <cstdio>

#include "align_plan.h"

int main()
{
    for (uint32_t tol = 0; tol <= 1024; tol++) std::printf("%u\n", vdf::align_seed_check_words(tol));
    return 0;
}
