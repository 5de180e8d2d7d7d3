// Hashes of the mirrored / flipped / reversed clip from the clip's own hash and zero plane (include/vdf.h: vdf_hash_variant).
// Host and device: plain constexpr C++, no HIP.
//   variant v: bit 0 = mirror along W, bit 1 = flip along H, bit 2 = reverse the 16 frames
//   M_v[i] = 1 iff i < 1000 and ((v & 1) kx + ((v >> 1) & 1) ky + ((v >> 2) & 1) kt) is odd,  i = 100 kt + 10 kx + ky   (dct_3d.rs:55-66)
//   H_v = (H ^ M_v) & ~Z
#pragma once
#include <stdint.h>

namespace vdf {

constexpr uint32_t kHashVariants = 8;

struct VariantMasks {
    uint64_t m[kHashVariants][16];
};

constexpr VariantMasks make_variant_masks()
{
    VariantMasks t{};
    for (uint32_t v = 0; v < kHashVariants; v++)
        for (uint32_t i = 0; i < 1000; i++) {
            const uint32_t kt = i / 100, kx = (i / 10) % 10, ky = i % 10;
            const uint32_t odd = ((v & 1u) * kx + ((v >> 1) & 1u) * ky + ((v >> 2) & 1u) * kt) & 1u;
            if (odd) t.m[v][i >> 6] |= uint64_t(1) << (i & 63);
        }
    return t;
}

inline constexpr VariantMasks kVariantMasks = make_variant_masks();

}  // namespace vdf
