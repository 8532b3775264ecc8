// mpn4.hip -- the last conv of the PointBERT mini-PointNet with its group max (Encoder.second_conv[1:] + max, dvae.py:194-199,
// 213-214):  tok[g, :] = max over the 32 points of group g of  W4 . relu(scale * y3 + shift) + bias,  y3 [M,512] 16-bit (the raw
// conv3 output whose folded BatchNorm + ReLU is applied while it is read), W4 [256,512]; nothing but tok is written.
// ppt_gemm runs this on 128 x 128 tiles through its register-staged A-prologue loop: 305 us for M = 524 288 (16 384 groups),
// against 90 us that reading y3 once costs at the 6.0 TB/s of a plain sweep.  The kernel is group_lds.h's at K = 512 with one column
// tile per wave (wave w: columns 32 w .. 32 w + 31 of W4 -- 32 k-steps x 16 bytes = 128 VGPRs), the group's 32 KB requested by
// LDS-DMA two groups ahead into a ring of three images (row pitch 1040 B), the affine + ReLU prologue applied to an image in place
// by the waves that requested its rows, and the group-max epilogue (32 reads, 32 MFMA, the max over the rows out of the
// accumulator).  Same affine expression and k order as the generic path: bit-identical maxima.
// NOT HBM-bound (profiles/r24_group_lds_pipeline.md; alone, 16 384 groups, f16): 157-159 us = 3.4 TB/s with 64 KB of requests in
// flight per CU all the time (162-164 us with one group's loads issued late, before); MFMA floor 55 us.  What remains is on the
// chip: per group and SIMD two waves each run 32 dependent (ds_read_b128, MFMA) steps, the in-place pass and the barrier.
#include "group_lds.h"

namespace {
using G4 = group_lds<512, 1>;
template <typename F> constexpr auto mpn4_kernel = group_lds_kernel<F, G4::K, G4::TJ, true, GL_POOL>;
}  // namespace

extern "C" int ppt_mini_pointnet_conv4_half(const void *A, int64_t M, int K, const float *a_scale, const float *a_shift, const void *W,
                                            const float *bias, int N, void *tok, int dtype, void *stream)
{
    if (dtype != PPT_BF16 && dtype != PPT_F16) return PPT_EINVAL;
    if (!A || !a_scale || !a_shift || !W || !tok || M <= 0) return PPT_EINVAL;
    if (K != G4::K || N != G4::N || M % 32) return PPT_EUNSUPPORTED;
    if (((uintptr_t)A | (uintptr_t)W) & 15) return PPT_EINVAL;
    constexpr int lds = G4::RING;
    PPT_RAISE_LDS_ONCE(lds, (const void *)mpn4_kernel<bf16_t>, (const void *)mpn4_kernel<f16_t>);
    const int64_t tiles = M / 32;
    // ONE persistent workgroup per CU: there is no second -- 176 VGPRs at 512 threads are two waves per SIMD, all of one
    // workgroup, and the ring takes 98 KB of the CU's LDS
    const int grid = ppt_persistent_grid(tiles, 1, ppt_stream(stream));
    ppt_launch16(dtype, [&](auto f) {
        hipLaunchKernelGGL(mpn4_kernel<decltype(f)>, dim3(grid), dim3(512), lds, ppt_stream(stream), (const bf16_t *)A, (int)tiles, a_scale,
                           a_shift, (const bf16_t *)W, bias, (bf16_t *)tok, (float *)nullptr, (float *)nullptr);
    });
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" int ppt_mini_pointnet_conv4_bf16(const void *A, int64_t M, int K, const float *a_scale, const float *a_shift, const void *W,
                                            const float *bias, int N, void *tok, void *stream)
{
    return ppt_mini_pointnet_conv4_half(A, M, K, a_scale, a_shift, W, bias, N, tok, PPT_BF16, stream);
}
