// dct_hash_windows_mixed_rates_kernel (csrc/dct_hash.hip) run on the CPU, from its own source text: tests/test_hash_windows_mixed_rates_kernel_host.py
// cuts the DCT butterflies, WindowsRetimedShared and the kernel out of dct_hash.hip into windows_mixed_rates_kernel.inc, and this program supplies what HIP
// would: 256 host threads per workgroup, a barrier for __syncthreads, wave ballots, LDS as a static.  Built once with -fsanitize=address,undefined (every index
// the kernel forms: the segment table, the records, row0, `small`, the ring, the output rows) and once with -fsanitize=thread (a barrier missing between a
// write and a read of LDS is a data race here).  Several 16 x 16 videos of different lengths in ONE call at several rates: planned by
// plan_windows_mixed_rates exactly as api.cpp plans them, `small` of exactly the planned size filled pseudo-clip by pseudo-clip as the resize kernels would
// fill it (16 x 16 -> 16 x 16 is a copy), seg_first and row0 of exactly their planned sizes, every (video, segment) workgroup run.
// usage: windows_mixed_rates_kernel_host in.bin stride num/den,num/den,... out.bin F_0 F_1 ...   (in.bin: the videos' frames one after the other, 256 bytes each)
// out.bin: hashes [rows][16] u64, don't-care counts [rows] u32, rows = rate_first[n_rates]; every row prefilled with ones
#include <algorithm>
#include <atomic>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "windows_mixed_rates_plan.h"
struct Idx { uint32_t x; };
static thread_local Idx threadIdx, blockIdx;
static std::barrier<> *g_block_barrier;
static std::barrier<> *g_wave_barrier[4];
static uint8_t g_pred[4][64];
#define __device__
#define __forceinline__ inline
#define __global__
#define __launch_bounds__(n)
#define __shared__ static
#define __restrict__
typedef const double *const_f64_ptr;
static inline void __syncthreads() { g_block_barrier->arrive_and_wait(); }
static inline unsigned long long __builtin_amdgcn_ballot_w64(bool p)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    g_pred[wave][lane] = p;
    g_wave_barrier[wave]->arrive_and_wait();
    unsigned long long m = 0;
    for (int i = 0; i < 64; i++) m |= (unsigned long long)g_pred[wave][i] << i;
    g_wave_barrier[wave]->arrive_and_wait();
    return m;
}
static inline uint32_t atomicOr(uint32_t *p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
using std::max;
using std::min;
static inline unsigned long long min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
namespace vdf {
#include "windows_mixed_rates_kernel.inc"
}
int main(int argc, char **argv)
{
    using namespace vdf;
    if (argc < 6) return 2;
    const uint32_t stride = atoi(argv[2]);
    uint32_t num[kWindowsMaxRates + 1], den[kWindowsMaxRates + 1], n_rates = 0;
    for (const char *s = argv[3]; *s && n_rates <= kWindowsMaxRates; n_rates++) {
        char *e;
        num[n_rates] = (uint32_t)strtoul(s, &e, 10);
        if (*e != '/') return 2;
        den[n_rates] = (uint32_t)strtoul(e + 1, &e, 10);
        s = *e == ',' ? e + 1 : e;
    }
    const size_t n = argc - 5;
    std::vector<uint32_t> nf(n);
    std::vector<MixedClip> clips(n);
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        nf[i] = atoi(argv[5 + i]);
        clips[i] = MixedClip{at, 256, 16, 16, {0, 0, 0, 0}};
        at += (uint64_t)nf[i] * 256;
    }
    std::vector<uint8_t> buf(at);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(buf.data(), 1, buf.size(), f) != buf.size()) return 2;
    fclose(f);
    if (check_windows_mixed(clips.data(), nf.data(), n, stride, buf.size()).error != WindowsMixedError::kNone) return 3;
    if (check_windows_mixed_rates(nf.data(), n, stride, n_rates, num, den).error != WindowsMixedRatesError::kNone) return 3;
    const WindowsMixedRatesPlan plan = plan_windows_mixed_rates(clips.data(), nf.data(), n, stride, n_rates, num, den);
    if (plan.kind != WindowsMixedRatesPlan::kMixed) return 4;  // (equal lengths would be the uniform call's kernel)
    // the resize stage: exactly small_bytes, so that a frame address past the last pseudo-clip is an AddressSanitizer finding
    std::vector<uint8_t> small(plan.small_bytes);
    for (const MixedLaunch &l : plan.launches)
        for (size_t s = l.first; s < l.first + l.count; s++)
            for (uint32_t fr = 0; fr < 16; fr++)
                std::memcpy(&small[(s * 16 + fr) * 256], &buf[plan.descs[s].offset + fr * plan.descs[s].frame_stride], 256);
    double tab[16 * 16 + 17] = {0};
    int ti = 256;
    auto twiddle = [&](int i, int fft_len) {
        const double angle_constant = M_PI * -2.0 / (double)fft_len;
        const double angle = angle_constant * (double)i;
        tab[ti++] = std::cos(angle);
        tab[ti++] = -std::sin(angle);
    };
    for (int i = 0; i < 4; i++) twiddle(2 * i + 1, 64);
    for (int i = 0; i < 2; i++) twiddle(2 * i + 1, 32);
    twiddle(1, 16);
    tab[ti++] = M_SQRT1_2;
    const size_t rows = (size_t)plan.rate_first[n_rates];
    std::vector<uint64_t> out(rows * 16, ~0ull);
    std::vector<uint32_t> dc(rows, ~0u);
    std::barrier<> bb(256), w0(64), w1(64), w2(64), w3(64);
    g_block_barrier = &bb;
    g_wave_barrier[0] = &w0; g_wave_barrier[1] = &w1; g_wave_barrier[2] = &w2; g_wave_barrier[3] = &w3;
    const uint32_t groups = plan.seg_first[n];
    for (uint32_t g = 0; g < groups; g++) {
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < 256; t++)
            th.emplace_back([&, t] {
                threadIdx.x = t;
                blockIdx.x = g & 1u;  // the launcher's split: first_group + blockIdx.x
                dct_hash_windows_mixed_rates_kernel(small.data(), plan.videos.data(), plan.seg_first.data(), plan.row0.data(), (uint32_t)n, plan.stride, plan.a,
                                                    plan.per_seg, g - (g & 1u), tab, out.data(), dc.data());
            });
        for (auto &x : th) x.join();
    }
    f = fopen(argv[4], "wb");
    fwrite(out.data(), 8, out.size(), f);
    fwrite(dc.data(), 4, dc.size(), f);
    fclose(f);
    return 0;
}
