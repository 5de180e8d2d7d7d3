// dct_hash_windows_rates_kernel (csrc/dct_hash.hip) run on the CPU, from its own source text: tests/test_hash_windows_rates_kernel_host.py cuts the
// DCT butterflies, WindowsSource, WindowsRetimedShared and the kernel out of dct_hash.hip into windows_rates_kernel.inc, and this program supplies what
// HIP would: 256 host threads per workgroup, a barrier for __syncthreads, wave ballots, LDS as a static.  Built once with -fsanitize=address,undefined
// (every index the kernel forms: LDS, frames, outputs) and once with -fsanitize=thread (a barrier missing between a write and a read of LDS is a data
// race here); the hashes and don't-care counts it writes, rate-major, are held against the oracle by the Python side.  Contraction off
// (-ffp-contract=off), as the kernel's pragma has it.
// usage: windows_rates_kernel_host in.bin n_clips F stride num/den,num/den,... frame_stride clip_stride dwords out.bin   (16 x 16 frames, read in place)
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
#include "windows_rates_plan.h"
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
#include "windows_rates_kernel.inc"
}
int main(int argc, char **argv)
{
    using namespace vdf;
    if (argc != 10) return 2;
    const size_t n_clips = atoll(argv[2]);
    const uint32_t F = atoi(argv[3]), stride = atoi(argv[4]);
    uint32_t num[kWindowsMaxRates + 1], den[kWindowsMaxRates + 1], n_rates = 0;
    for (const char *s = argv[5]; *s && n_rates <= kWindowsMaxRates; n_rates++) {
        char *e;
        num[n_rates] = (uint32_t)strtoul(s, &e, 10);
        if (*e != '/') return 2;
        den[n_rates] = (uint32_t)strtoul(e + 1, &e, 10);
        s = *e == ',' ? e + 1 : e;
    }
    const size_t fs = atoll(argv[6]), cs = atoll(argv[7]);
    const int dwords = atoi(argv[8]);
    FILE *f = fopen(argv[1], "rb");
    std::vector<uint8_t> buf((n_clips - 1) * cs + (size_t)(F - 1) * fs + 256);
    if (fread(buf.data(), 1, buf.size(), f) != buf.size()) return 2;
    fclose(f);
    double tab[16 * 16 + 17] = {0};
    int at = 256;
    auto twiddle = [&](int i, int fft_len) {
        const double angle_constant = M_PI * -2.0 / (double)fft_len;
        const double angle = angle_constant * (double)i;
        tab[at++] = std::cos(angle);
        tab[at++] = -std::sin(angle);
    };
    for (int i = 0; i < 4; i++) twiddle(2 * i + 1, 64);
    for (int i = 0; i < 2; i++) twiddle(2 * i + 1, 32);
    twiddle(1, 16);
    tab[at++] = M_SQRT1_2;
    const WindowsRatesPlan plan = plan_windows_rates(n_clips, F, stride, n_rates, num, den);
    if (!plan.ok) return 3;
    std::vector<uint64_t> out(plan.n_out * 16, ~0ull);
    std::vector<uint32_t> dc(plan.n_out, ~0u);
    WindowsSource src{buf.data(), buf.data(), cs, 16 * fs, fs, 0, F, 0};
    std::barrier<> bb(256), w0(64), w1(64), w2(64), w3(64);
    g_block_barrier = &bb;
    g_wave_barrier[0] = &w0; g_wave_barrier[1] = &w1; g_wave_barrier[2] = &w2; g_wave_barrier[3] = &w3;
    const uint64_t groups = rates_groups(n_clips, plan);
    for (uint64_t g = 0; g < groups; g++) {
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < 256; t++)
            th.emplace_back([&, t] {
                threadIdx.x = t;
                blockIdx.x = 0;
                if (dwords) dct_hash_windows_rates_kernel<true>(src, stride, plan.a, plan.per_seg, plan.n_seg, g, tab, out.data(), dc.data());
                else dct_hash_windows_rates_kernel<false>(src, stride, plan.a, plan.per_seg, plan.n_seg, g, tab, out.data(), dc.data());
            });
        for (auto &x : th) x.join();
    }
    f = fopen(argv[9], "wb");
    fwrite(out.data(), 8, out.size(), f);
    fwrite(dc.data(), 4, dc.size(), f);
    fclose(f);
    return 0;
}
