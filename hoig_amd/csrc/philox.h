// Philox4x32-10 (Salmon et al. 2011, Random123): the one counter-based generator of the library, shared by the discriminator
// augmentation (d_augment.h) and the patch positions of the sliced Wasserstein distance (swd.h).  Integer arithmetic only: the host
// and the device give the same words.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HOIG_PHILOX_HD __host__ __device__
#else
#define HOIG_PHILOX_HD
#endif

HOIG_PHILOX_HD inline void hoig_philox4x32_10(const uint32_t ctr[4], uint32_t k0, uint32_t k1, uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// a draw below n: (w * n) >> 32
HOIG_PHILOX_HD inline int hoig_philox_below(uint32_t w, int n) { return (int)(((uint64_t)w * (uint64_t)(uint32_t)n) >> 32); }
