// The PLANES form of dct_hash_windows_kernel (csrc/dct_hash.hip) run on the CPU from its own source text, as
// windows_kernel_host_main.cpp runs the plain form: tests/test_hash_windows_planes_kernel_host.py cuts the same stretch of dct_hash.hip into a
// windows_kernel.inc of its own directory, and this program takes the HIP stand-ins (256 host threads per workgroup, a barrier for
// __syncthreads, wave ballots, LDS as statics) from that file - included here with its main renamed - and launches
// dct_hash_windows_kernel<DWORDS, true> with a zero-plane buffer.  Built once with -fsanitize=address,undefined and once with
// -fsanitize=thread; hashes, planes and don't-care counts are held against the oracle by the Python side.
// usage: windows_planes_kernel_host in.bin n_clips F stride frame_stride clip_stride dwords out.bin   (out: hashes, planes, counts)
#define main windows_kernel_host_plain_main
#include "windows_kernel_host_main.cpp"
#undef main

int main(int argc, char **argv)
{
    using namespace vdf;
    if (argc != 9) return 2;
    const size_t n_clips = atoll(argv[2]);
    const uint32_t F = atoi(argv[3]), stride = atoi(argv[4]);
    const size_t fs = atoll(argv[5]), cs = atoll(argv[6]);
    const int dwords = atoi(argv[7]);
    FILE *f = fopen(argv[1], "rb");
    std::vector<uint8_t> buf((n_clips - 1) * cs + (size_t)(F - 1) * fs + 256);
    if (!f || fread(buf.data(), 1, buf.size(), f) != buf.size()) return 2;
    fclose(f);
    double tab[16 * 16 + 17] = {0};  // the twiddles dct16_pruned reads, in cos_table's order (t16, t8, t4, h from entry 256 on)
    int at = 256;
    auto twiddle = [&](int i, int fft_len) {
        const double angle = (M_PI * -2.0 / (double)fft_len) * (double)i;
        tab[at++] = std::cos(angle);
        tab[at++] = -std::sin(angle);
    };
    for (int i = 0; i < 4; i++) twiddle(2 * i + 1, 64);
    for (int i = 0; i < 2; i++) twiddle(2 * i + 1, 32);
    twiddle(1, 16);
    tab[at++] = M_SQRT1_2;
    const WindowsPlan plan = plan_windows(F, stride);
    // exactly n_clips x n_win entries each, pre-filled: a store outside them is the sanitizer's, a window left out shows as ~0
    std::vector<uint64_t> out(n_clips * plan.n_win * 16, ~0ull), zero(n_clips * plan.n_win * 16, ~0ull);
    std::vector<uint32_t> dc(n_clips * plan.n_win, ~0u);
    WindowsSource src{buf.data(), buf.data(), cs, 16 * fs, fs, 0, F, 0};
    std::barrier<> bb(256), w0(64), w1(64), w2(64), w3(64);
    g_block_barrier = &bb;
    g_wave_barrier[0] = &w0; g_wave_barrier[1] = &w1; g_wave_barrier[2] = &w2; g_wave_barrier[3] = &w3;
    const uint64_t groups = (uint64_t)n_clips * plan.n_seg;
    for (uint64_t g = 0; g < groups; g++) {
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < 256; t++)
            th.emplace_back([&, t] {
                threadIdx.x = t;
                blockIdx.x = 0;
                if (dwords) dct_hash_windows_kernel<true, true>(src, stride, plan.n_win, plan.per_seg, plan.n_seg, g, tab, out.data(), dc.data(), zero.data());
                else dct_hash_windows_kernel<false, true>(src, stride, plan.n_win, plan.per_seg, plan.n_seg, g, tab, out.data(), dc.data(), zero.data());
            });
        for (auto &x : th) x.join();
    }
    f = fopen(argv[8], "wb");
    fwrite(out.data(), 8, out.size(), f);
    fwrite(zero.data(), 8, zero.size(), f);
    fwrite(dc.data(), 4, dc.size(), f);
    fclose(f);
    return 0;
}
