// group_lds.h -- the LDS-staged group kernel: out = epilogue( prologue(A) . W^T ) with A [32 n_tiles, K] 16-bit read ONCE from HBM
// and W [256 TJ, K] never moving.  A workgroup is 8 waves; wave w keeps columns 32 TJ w .. 32 TJ (w + 1) - 1 of W in 8 TJ K / 32 VGPRs
// for the whole kernel (128 in both instantiated shapes).  One group of 32 points is one MFMA row tile: the 512 threads load its
// 64 K bytes (K / 8 chunks of 16 bytes per row; a thread always owns the same chunk column cc and K / 128 rows, so with the affine
// prologue its 8 (scale, shift) pairs live in registers), apply the prologue once and park the tile in LDS (row pitch 2 K + 16 B:
// the 16 lanes of a ds_read_b128 phase hit 64 distinct banks); every wave then reads its A fragments from there.  Two LDS buffers,
// one barrier per group; the next group's global loads are issued before the MFMA loop.  Persistent grid: workgroup b takes groups
// b, b + grid, ...  Same expressions and k order as ppt_gemm's path for the same product: results are bit-identical to it.
//   prologue  AFFINE: a = relu(a_scale[k] * a + a_shift[k]) (affine_relu_chunk16), else the rows as they are
//   epilogue  GL_POOL:  out[g, n] = max over the group's rows of (acc + add[n])   (`add` = the bias [N], may be null)
//             otherwise v = acc + add[g, n] (`add` = the per-group term [n_tiles, N]), then
//             GL_STATS: BatchNorm partials of v per group (PPT_GT_CHUNK_STATS) and / or GL_STORE: out[32 g + r, n] = v, through a
//             wave-private LDS transpose (8 tiles behind the two A buffers) as 64 TJ-byte row pieces.
// Used by mpn3.hip (K 256, TJ 2, plain, STATS / STORE) and mpn4.hip (K 512, TJ 1, AFFINE, POOL).
#pragma once
#include "group_tile.h"

namespace {

enum { GL_POOL = 1, GL_STATS = 2, GL_STORE = 4 };

template <int K_, int TJ_> struct group_lds {                                                  // a shape and what follows from it
    static constexpr int K = K_, TJ = TJ_, N = 256 * TJ, KS = K / 16, PITCH = 2 * K + 16, BUF = 32 * PITCH;      // A buffer: 32 rows
    static constexpr int TP = 64 * TJ + 16, TR = 32 * TP;                                      // a wave's transpose tile
    static constexpr int CPR = K / 8, RSTEP = 512 / CPR, NV = K / 128;                         // loader: chunks per row, row step, rows per thread
};

template <typename F, int K, int TJ, bool AFFINE, int EP>
__global__ __launch_bounds__(512, 2) void group_lds_kernel(const bf16_t *__restrict__ A, int n_tiles, const float *__restrict__ a_scale,
                                                            const float *__restrict__ a_shift, const bf16_t *__restrict__ W,
                                                            const float *__restrict__ add, bf16_t *__restrict__ out,
                                                            float *__restrict__ part_sum, float *__restrict__ part_m2)
{
    using G = group_lds<K, TJ>;
    constexpr bool POOL = EP & GL_POOL, STATS = EP & GL_STATS, STORE = EP & GL_STORE;
    static_assert((G::NV == 2 || G::NV == 4) && POOL != (STATS || STORE), "one output pointer; two or four rows per loader thread");
    extern __shared__ __align__(16) unsigned char smem[];          // 2 A buffers, then (STORE) 8 transpose tiles
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 31, h = lane >> 5;
    const int n_w = 32 * TJ * w;                                    // first column of this wave
    uint4 bfrag[TJ][G::KS];
    float bias[TJ];
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
        PPT_GT_LOAD_WEIGHTS(bfrag[j], G::KS, W, n_w + 32 * j + col, h);
        if constexpr (POOL) bias[j] = add ? add[n_w + 32 * j + col] : 0.f;
    }
    unsigned char *tr = smem + 2 * G::BUF + w * G::TR;
    const int cc = threadIdx.x % G::CPR, rb = threadIdx.x / G::CPR; // loader: 16-byte chunk cc of rows rb + RSTEP i, i < NV
    float sc[8], sh[8];
    if constexpr (AFFINE)
#pragma unroll
        for (int e = 0; e < 8; ++e) { sc[e] = a_scale[8 * cc + e]; sh[e] = a_shift[8 * cc + e]; }
    // The rows in flight are NAMED values, not an array: an array that lives across the wavefront fences of the store epilogue is
    // kept in scratch memory.  For the same reason the prefetch below is unconditional (its tile index clamped): under a branch
    // the values are parked in scratch as well.
    uint4 v0, v1, v2, v3;
    auto load = [&](int tile) {
        const bf16_t *p = A + ((size_t)tile * 32 + rb) * K + 8 * cc;
        v0 = *reinterpret_cast<const uint4 *>(p);
        v1 = *reinterpret_cast<const uint4 *>(p + (size_t)G::RSTEP * K);
        if constexpr (G::NV == 4) {
            v2 = *reinterpret_cast<const uint4 *>(p + (size_t)2 * G::RSTEP * K);
            v3 = *reinterpret_cast<const uint4 *>(p + (size_t)3 * G::RSTEP * K);
        }
    };
    auto stage = [&](int buf) {
        unsigned char *d = smem + buf * G::BUF + rb * G::PITCH + cc * 16;
        if constexpr (AFFINE) {
            affine_relu_chunk16<F>(v0, sc, sh);
            affine_relu_chunk16<F>(v1, sc, sh);
            if constexpr (G::NV == 4) { affine_relu_chunk16<F>(v2, sc, sh); affine_relu_chunk16<F>(v3, sc, sh); }
        }
        *reinterpret_cast<uint4 *>(d) = v0;
        *reinterpret_cast<uint4 *>(d + G::RSTEP * G::PITCH) = v1;
        if constexpr (G::NV == 4) {
            *reinterpret_cast<uint4 *>(d + 2 * G::RSTEP * G::PITCH) = v2;
            *reinterpret_cast<uint4 *>(d + 3 * G::RSTEP * G::PITCH) = v3;
        }
    };
    int t = blockIdx.x;
    if (t >= n_tiles) return;
    load(t);
    stage(0);
    __syncthreads();
    for (int it = 0; t < n_tiles; t += gridDim.x, ++it) {
        const int cur = it & 1;
        load(min(t + (int)gridDim.x, n_tiles - 1));
        const unsigned char *at = smem + cur * G::BUF + col * G::PITCH + 16 * h;
        ppt_f32x16 acc[TJ];
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
#pragma unroll
        for (int s = 0; s < G::KS; ++s) {
            const uint4 a = *reinterpret_cast<const uint4 *>(at + 32 * s);
#pragma unroll
            for (int j = 0; j < TJ; ++j) acc[j] = h16<F>::mfma32(a, bfrag[j][s], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const size_t o = (size_t)t * G::N + n_w + 32 * j + col;
            if constexpr (POOL) {
                float mx = -INFINITY;
#pragma unroll
                for (int e = 0; e < 16; ++e) mx = fmaxf(mx, acc[j][e] + bias[j]);
                mx = xor32_max(mx);
                if (h == 0) out[o] = h16<F>::from_f32(mx);
            } else {
                const float gt = add[o];
                float sm = 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    acc[j][e] += gt;
                    sm += acc[j][e];
                }
                if constexpr (STATS) PPT_GT_CHUNK_STATS(acc[j], sm, h, part_sum, part_m2, o);
                if constexpr (STORE) PPT_GT_TILE_TO_LDS(F, acc[j], tr, G::TP, j, lane, col, h);
            }
        }
        if constexpr (STORE) PPT_GT_TILE_OUT(TJ, tr, G::TP, out, (size_t)t * 32, G::N, n_w, lane);
        stage(cur ^ 1);                                             // last read in iteration it - 1, before its barrier
        __syncthreads();
    }
}

}  // namespace
