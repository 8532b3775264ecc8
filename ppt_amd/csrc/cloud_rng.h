// cloud_rng.h -- the counter-based generator of the device-resident input pipeline (cloud_prep.hip: ppt_cloud_draws;
// cloud_augment.hip: ppt_cloud_draws_aug).  counter = (sample index, epoch, slot | attempt << 8, block), key = the seed.
#pragma once
#include "ppt_common.h"

// ---- Philox4x32-10 (Salmon et al., SC'11; the constants and round structure of Random123's philox.h) -----------------------------
struct philox_out { uint32_t w[4]; };

__device__ __forceinline__ philox_out philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return philox_out{{c0, c1, c2, c3}};
}

// draw slots (counter word 2).  0-3: ppt_cloud_draws; 4-10: ppt_cloud_draws_aug (the layout of each is stated in include/ppt_hip.h)
enum { SLOT_START = 0, SLOT_AFFINE = 1, SLOT_PERM = 2, SLOT_SEL = 3,
       SLOT_DROP_RATIO = 4, SLOT_DROP_MASK = 5, SLOT_SCALE = 6, SLOT_SHIFT = 7, SLOT_PERTURB = 8, SLOT_ROTATE = 9, SLOT_JITTER = 10 };

__device__ __forceinline__ double uniform53(uint32_t hi, uint32_t lo)        // [0, 1) from 53 random bits (27 + 26)
{
    return (double)(((uint64_t)(hi >> 5) << 26) | (uint64_t)(lo >> 6)) * (1.0 / 9007199254740992.0);
}

// An integer in [0, range) without modulo bias (Lemire 2019: multiply-shift, reject the short residue class).  The four words of
// one Philox block are four attempts; a rejection has probability range / 2^32 <= 4e-6 each, further blocks follow on the
// `attempt` field of the counter.  16 blocks bound the loop; reaching the bound has probability below 1e-300.
__device__ __forceinline__ uint32_t bounded(uint32_t idx, uint32_t epoch, uint32_t slot, uint32_t block, uint32_t k0, uint32_t k1,
                                            uint32_t range)
{
    const uint32_t thresh = (0u - range) % range;
    uint32_t res = 0;
    for (uint32_t attempt = 0; attempt < 16; ++attempt) {
        const philox_out r = philox4x32_10(idx, epoch, slot | (attempt << 8), block, k0, k1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t mm = (uint64_t)r.w[j] * range;
            if ((uint32_t)mm >= thresh) return (uint32_t)(mm >> 32);
            res = (uint32_t)(mm >> 32);
        }
    }
    return res;
}
