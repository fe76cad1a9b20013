// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the counter-based generator of every
// random draw in the library (input_ops.hip, k_train.hip, k_pair.hip, affine.hip, dose.hip).  key = (seed lo, seed hi); counter word 3 carries a stream tag, so
// that the entry points draw independent sequences under one seed.
#pragma once

#include <hip/hip_runtime.h>

namespace emd {

constexpr unsigned kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
// stream tags (counter word 3)
constexpr unsigned kPhiloxTagRaw = 0u, kPhiloxTagScale = 1u, kPhiloxTagChoice = 2u, kPhiloxTagPoisson = 3u, kPhiloxTagKCrop = 4u, kPhiloxTagSCrop = 5u,
                   kPhiloxTagKPair = 6u, kPhiloxTagMiSamples = 7u, kPhiloxTagAffineNormal = 8u, kPhiloxTagDose = 9u;

struct U4 {
    unsigned x, y, z, w;
};

__host__ __device__ inline U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)kPhiloxM0 * c.x, p1 = (unsigned long long)kPhiloxM1 * c.z;
        const U4 n = {(unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0};
        c = n;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    return c;
}

}  // namespace emd
