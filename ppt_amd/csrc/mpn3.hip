// mpn3.hip -- the middle conv of the PointBERT mini-PointNet (Encoder.second_conv[0] on cat(global, local), dvae.py:194-195,
// 211-212), in the split form engine.mini_pointnet uses:  y3[m, :] = W3b . y2[m, :] + gterm[m / 32, :]  (gterm = the global
// half of the conv per group, bias included), y2 [M,256] 16-bit, W3b [512,256], y3 [M,512], plus the BatchNorm partials of y3 per
// 32-row chunk.  537 MB of output + 268 MB of input at C2's size; ppt_gemm's 128 x 128 tile loop needs 311 us for it.
// The kernel is group_lds.h's at K = 256 with two column tiles per wave (wave w: columns 64 w .. 64 w + 63 of W3b in 128 VGPRs),
// the plain prologue and the group-term epilogue: a group's 16 KB go to LDS once (by LDS-DMA, three groups ahead in a ring of four
// images, the group term with them), every wave adds the group term, forms the chunk statistics in registers and sends its
// 32 x 64 block out as 128-byte row pieces.  Same k order as the generic path: y3 is bit-identical.
// NOT HBM-bound (profiles/r24_group_lds_pipeline.md; alone, 16 384 groups, f16): statistics + store 220-225 us = 3.6 TB/s, store
// only 187 us = 4.3 TB/s, against 6.0 TB/s for a plain sweep -- and the statistics pass, which writes next to nothing, still takes
// 153-158 us for its 268 MB (1.7 TB/s; MFMA floor 55 us).  With three groups of requests in flight no HBM latency is left in the
// loop, so what remains is on the chip: the fragment reads + MFMAs and the epilogue of two waves per SIMD between the barriers.
// y == NULL -- the statistics pass alone: the BatchNorm partials of y3 without y3 itself, for the training step whose second pass
// is the fused conv3 + BN + ReLU + conv4 + max kernel (csrc/mpn34.hip).
#include "group_lds.h"

namespace {
using G3 = group_lds<256, 2>;
template <typename F, int EP> constexpr auto mpn3_kernel = group_lds_kernel<F, G3::K, G3::TJ, false, EP>;
}  // namespace

extern "C" int ppt_mini_pointnet_conv3_half(const void *A, int64_t M, int K, const void *W, const float *gterm, int N, void *y,
                                            float *part_sum, float *part_m2, int dtype, void *stream)
{
    if (dtype != PPT_BF16 && dtype != PPT_F16) return PPT_EINVAL;
    if (!A || !W || !gterm || M <= 0 || ((part_sum == nullptr) != (part_m2 == nullptr)) || (!y && !part_sum)) return PPT_EINVAL;
    if (K != G3::K || N != G3::N || M % 32) return PPT_EUNSUPPORTED;
    if (((uintptr_t)A | (uintptr_t)W | (uintptr_t)y | (uintptr_t)gterm) & 15) return PPT_EINVAL;    // (gterm: read in 16-byte pieces)
    constexpr int lds = G3::RING + G3::TERMS + 8 * G3::TR, ST = GL_STATS, SO = GL_STORE;
    PPT_RAISE_LDS_ONCE(lds, (const void *)mpn3_kernel<bf16_t, ST | SO>, (const void *)mpn3_kernel<bf16_t, SO>, (const void *)mpn3_kernel<bf16_t, ST>,
                       (const void *)mpn3_kernel<f16_t, ST | SO>, (const void *)mpn3_kernel<f16_t, SO>, (const void *)mpn3_kernel<f16_t, ST>);
    const int64_t tiles = M / 32;
    // ONE persistent workgroup per CU: there is no second -- 186-224 VGPRs at 512 threads are two waves per SIMD, all of one
    // workgroup, and the ring takes 110 KB of the CU's LDS
    const int grid = ppt_persistent_grid(tiles, 1, ppt_stream(stream));
    ppt_launch16(dtype, [&](auto f) {
        using F = decltype(f);
        const auto k = !y ? mpn3_kernel<F, ST> : part_sum ? mpn3_kernel<F, ST | SO> : mpn3_kernel<F, SO>;
        hipLaunchKernelGGL(k, dim3(grid), dim3(512), lds, ppt_stream(stream), (const bf16_t *)A, (int)tiles, (const float *)nullptr,
                           (const float *)nullptr, (const bf16_t *)W, gterm, (bf16_t *)y, part_sum, part_m2);
    });
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" int ppt_mini_pointnet_conv3_bf16(const void *A, int64_t M, int K, const void *W, const float *gterm, int N, void *y,
                                            float *part_sum, float *part_m2, void *stream)
{
    return ppt_mini_pointnet_conv3_half(A, M, K, W, gterm, N, y, part_sum, part_m2, PPT_BF16, stream);
}
