// group_tile.h -- the pieces shared by the kernels that take one GROUP of 32 points as one MFMA row tile while the weight stays
// in registers: mpn1.hip, affpool.hip and the LDS-staged kernel of group_lds.h (mpn3.hip, mpn4.hip).
// One wave, one 32 x 32 accumulator (ppt_f32x16) per column tile; C layout of h16<F>::mfma32: lane holds column col = lane & 31,
// rows (e & 3) + 8 (e >> 2) + 4 h with h = lane >> 5.
// The pieces are MACROS (locals carry a trailing underscore): as __forceinline__ functions (accumulator by reference or by value,
// pitches as arguments or as template parameters) each of them changed the instruction order of every kernel it was used in (tools/kernel_isa_diff.py;
// profiles/r13_group_tile.md).  For the same reason their index arguments are written out at the call, not put in a variable.
#pragma once
#include "ppt_common.h"

// The stationary operand of one column tile: row n (the lane's column) of W [N, 16 KS] (16-bit, row-major) as the MFMA B fragments
// of the KS k-steps -- uint4 bfrag[KS], 4 KS VGPRs -- loaded once per kernel.
#define PPT_GT_LOAD_WEIGHTS(bfrag, KS, W, n, h)                                                                         \
    do {                                                                                                                \
        _Pragma("unroll") for (int s_ = 0; s_ < (KS); ++s_)                                                             \
            (bfrag)[s_] = *reinterpret_cast<const uint4 *>((W) + (size_t)(n) * (16 * (KS)) + 16 * s_ + 8 * (h));        \
    } while (0)

// BatchNorm partials of the 32-row chunk an accumulator holds, for this lane's column: part_sum[o] = sum, part_m2[o] = sum (v -
// chunk mean)^2, the layout ppt_bn_finalize_ws takes with rows_per_partial = 32.  `sm` (a float variable; changed) is the lane's
// own sum of its 16 values.
#define PPT_GT_CHUNK_STATS(acc, sm, h, part_sum, part_m2, o)                                                            \
    do {                                                                                                                \
        sm = xor32_sum(sm);                                                                                             \
        const float mean_ = sm * (1.0f / 32.0f);                                                                        \
        float q_ = 0.f;                                                                                                 \
        _Pragma("unroll") for (int e_ = 0; e_ < 16; ++e_) { const float d_ = (acc)[e_] - mean_; q_ = fmaf(d_, d_, q_); } \
        q_ = xor32_sum(q_);                                                                                             \
        if ((h) == 0) {                                                                                                 \
            (part_sum)[o] = sm;                                                                                         \
            (part_m2)[o] = q_;                                                                                          \
        }                                                                                                               \
    } while (0)

// An accumulator -> columns 32 j .. 32 j + 31 of the wave-private LDS tile `tr` (32 rows, PITCH bytes apart) in the 16-bit format
// F.  Neighbour lanes trade one value per register pair, so that a lane owns two adjacent columns of one row: even lanes keep
// row(e0), odd lanes row(e1) -- 4-byte LDS writes instead of 2-byte ones.
#define PPT_GT_TILE_TO_LDS(F, acc, tr, PITCH, j, lane, col, h)                                                          \
    do {                                                                                                                \
        _Pragma("unroll") for (int q_ = 0; q_ < 8; ++q_) {                                                              \
            const int e0_ = 2 * q_, e1_ = 2 * q_ + 1;                                                                   \
            const float send_ = ((lane) & 1) ? (acc)[e0_] : (acc)[e1_];                                                 \
            const float recv_ = __uint_as_float(dpp_mov<0xB1, 0xf>(__float_as_uint(send_)));   /* quad_perm [1,0,3,2] */ \
            const uint32_t packed_ = ((lane) & 1) ? h16<F>::pack2(recv_, (acc)[e1_]) : h16<F>::pack2((acc)[e0_], recv_); \
            const int e_ = ((lane) & 1) ? e1_ : e0_;                                                                    \
            const int row_ = (e_ & 3) + 8 * (e_ >> 2) + 4 * (h);                                                        \
            *reinterpret_cast<uint32_t *>((tr) + row_ * (PITCH) + (32 * (j) + ((col) & ~1)) * 2) = packed_;             \
        }                                                                                                               \
    } while (0)

// The wave's 32 x (32 TJ) tile leaves LDS as 64 TJ-byte row pieces (4 TJ lanes x 16 bytes per row, non-temporal stores): row r
// goes to y[(row0 + r) * N + n0 ...].  The wavefront fences order the tile's LDS writes before the reads.
#define PPT_GT_TILE_OUT(TJ, tr, PITCH, y, row0, N, n0, lane)                                                            \
    do {                                                                                                                \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                                          \
        __builtin_amdgcn_wave_barrier();                                                                                \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");                                                          \
        constexpr int LPR_ = 4 * (TJ), RPI_ = 64 / LPR_, NIT_ = (32 + RPI_ - 1) / RPI_;   /* lanes per row, rows per instruction */ \
        _Pragma("unroll") for (int q_ = 0; q_ < NIT_; ++q_) {                                                           \
            const int row_ = RPI_ * q_ + (lane) / LPR_, ch_ = (lane) % LPR_;                                            \
            if (row_ < 32 && (lane) < RPI_ * LPR_) {                                                                    \
                const uint4 v_ = *reinterpret_cast<const uint4 *>((tr) + row_ * (PITCH) + ch_ * 16);                    \
                ppt_store16_stream((y) + ((row0) + row_) * (N) + (n0) + ch_ * 8, v_);                                   \
            }                                                                                                           \
        }                                                                                                               \
    } while (0)
