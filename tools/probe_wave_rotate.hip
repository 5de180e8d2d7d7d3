// Confirms on gfx950 what align_bands_kernel (csrc/align.hip) relies on: v_mov_b32_dpp wave_ror:1 gives every lane the value of the lane
// below it and lane 0 that of lane 63 - the same as __shfl(v, (lane - 1) & 63) - with all 64 lanes active.
//   hipcc --offload-arch=gfx950 -O3 tools/probe_wave_rotate.hip -o tools/probe_wave_rotate && tools/probe_wave_rotate
#include <hip/hip_runtime.h>
#include <cstdio>

__global__ void k(const int *in, int *dpp, int *shfl)
{
    const int v = in[threadIdx.x];
    dpp[threadIdx.x] = __builtin_amdgcn_update_dpp(0, v, 0x13C, 0xF, 0xF, false);
    shfl[threadIdx.x] = __shfl(v, (threadIdx.x - 1) & 63, 64);
}

int main()
{
    int h_in[64], h_dpp[64], h_shfl[64], *d_in, *d_dpp, *d_shfl;
    for (int l = 0; l < 64; l++) h_in[l] = 1000 + 7 * l;
    if (hipMalloc(&d_in, 256) != hipSuccess || hipMalloc(&d_dpp, 256) != hipSuccess || hipMalloc(&d_shfl, 256) != hipSuccess) { printf("no device memory\n"); return 2; }
    hipMemcpy(d_in, h_in, 256, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, d_in, d_dpp, d_shfl);
    if (hipMemcpy(h_dpp, d_dpp, 256, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(h_shfl, d_shfl, 256, hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel failed\n"); return 2; }
    int bad_dpp = 0, bad_shfl = 0;
    for (int l = 0; l < 64; l++) {
        bad_dpp += h_dpp[l] != h_in[(l + 63) & 63];
        bad_shfl += h_shfl[l] != h_in[(l + 63) & 63];
    }
    printf("wave_ror:1: %d of 64 lanes differ from lane - 1 (mod 64); __shfl: %d; lane 0 got %d (lane 63 holds %d), lane 1 got %d (lane 0 holds %d)\n", bad_dpp, bad_shfl,
           h_dpp[0], h_in[63], h_dpp[1], h_in[0]);
    return bad_dpp || bad_shfl ? 1 : 0;
}
