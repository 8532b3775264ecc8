// attn_bwd16.h -- the inner pieces of the 16-bit attention backward (attention_mfma.hip): the dK / dV tile step and the dQ
// sub-step that attn_bwd_dkv_body, attn_bwd_dq_body and attn_bwd_tiny_mfma run, and the row stores of their results.
// The two steps are MACROS expanded in the caller's scope: as __forceinline__ functions they kept the VGPR count, LDS and scratch
// but not the register allocation (tools/kernel_isa_diff.py; profiles/r14_attention_bwd.md).  Their locals carry a trailing
// underscore.  The stores are functions: those compile to the written-out loops' instructions.
#pragma once
#include "attn_common.h"

// One 32-query tile against this wave's 32 keys: S = Q K^T, dP = dO V^T, P = exp2(S c - lse2), dS = P (dP - delta) scale, then
// dV^T += dO^T P and dK^T += Q^T dS.
//   Qr, Gr   row images of Q and dO (k_off);  Qt, Gt  their transposed-read images (v_off);  L2, DL  the lse2 / delta rows (float);
//   row0     first row of the tile inside the images and the two rows;  q_first  the tile's first query index (causal diagonal).
// From the caller's scope: F, CAUSAL, r, h, key, k0, c, scale, kf[4], vf[4], dvt[2], dkt[2], tr_row, tr_dbyte.
#define ATTN_BWD_DKV_STEP(Qr, Qt, Gr, Gt, L2, DL, row0, q_first)                                                        \
    do {                                                                                                                \
        f32x16_t sa_, dp_;                                                                                              \
        ATTN_ZERO2(sa_, dp_);                                                                                           \
        _Pragma("unroll") for (int kk_ = 0; kk_ < 4; ++kk_) {                                                           \
            const uint4 qa_ = *reinterpret_cast<const uint4 *>((Qr) + k_off((row0) + r, 2 * kk_ + h));                  \
            const uint4 ga_ = *reinterpret_cast<const uint4 *>((Gr) + k_off((row0) + r, 2 * kk_ + h));                  \
            sa_ = h16<F>::mfma32(qa_, kf[kk_], sa_);                                                                    \
            dp_ = h16<F>::mfma32(ga_, vf[kk_], dp_);                                                                    \
        }                                                                                                               \
        const bool diag_ = CAUSAL && (q_first) < k0 + 32;        /* some (q, key) pairs of this tile are masked */      \
        _Pragma("unroll") for (int gq_ = 0; gq_ < 4; ++gq_) {                                                           \
            const float4 l4_ = *reinterpret_cast<const float4 *>((L2) + (row0) + 8 * gq_ + 4 * h);                      \
            const float4 d4_ = *reinterpret_cast<const float4 *>((DL) + (row0) + 8 * gq_ + 4 * h);                      \
            const float lv_[4] = {l4_.x, l4_.y, l4_.z, l4_.w}, dv_[4] = {d4_.x, d4_.y, d4_.z, d4_.w};                   \
            _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) {                                                          \
                const int e_ = 4 * gq_ + j_;                                                                            \
                float pv_ = __builtin_amdgcn_exp2f(fmaf(sa_[e_], c, -lv_[j_]));                                         \
                if (diag_ && key > (q_first) + 8 * gq_ + 4 * h + j_) pv_ = 0.f;                                         \
                sa_[e_] = pv_;                                                                                          \
                dp_[e_] = pv_ * (dp_[e_] - dv_[j_]) * scale;                                                            \
            }                                                                                                           \
        }                                                                                                               \
        _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_) {                                                              \
            const uint4 pf_ = pack8<F>(sa_, s_), df_ = pack8<F>(dp_, s_);                                               \
            _Pragma("unroll") for (int dtile_ = 0; dtile_ < 2; ++dtile_) {                                              \
                const uint4 gt_ = tr_frag((Gt), (row0) + 16 * s_ + tr_row, tr_dbyte + 64 * dtile_);      /* dO^T */     \
                dvt[dtile_] = h16<F>::mfma32(gt_, pf_, dvt[dtile_]);                                                    \
                const uint4 qt_ = tr_frag((Qt), (row0) + 16 * s_ + tr_row, tr_dbyte + 64 * dtile_);      /* Q^T */      \
                dkt[dtile_] = h16<F>::mfma32(qt_, df_, dkt[dtile_]);                                                    \
            }                                                                                                           \
        }                                                                                                               \
    } while (0)

// 32 keys against this wave's 32 queries: S^T = K Q^T, dP^T = V dO^T, dS^T = P^T (dP^T - delta) scale with the keys at or past T
// and (CAUSAL) past the query masked when need_mask, then dQ^T += K^T dS^T.
//   Kr, Vr   row images of K and V (k_off);  Kt  K's transposed-read image (v_off);  row0  first row of the 32 keys inside the
//   images;  key_first  their first key index;  need_mask  wave-uniform.
// From the caller's scope: F, CAUSAL, r, h, qrow, T, c, scale, l2, dl, qf[4], gf[4], dqt[2], tr_row, tr_dbyte.
#define ATTN_BWD_DQ_STEP(Kr, Kt, Vr, row0, key_first, need_mask)                                                        \
    do {                                                                                                                \
        f32x16_t sa_, dp_;                                                                                              \
        ATTN_ZERO2(sa_, dp_);                                                                                           \
        _Pragma("unroll") for (int kk_ = 0; kk_ < 4; ++kk_) {                                                           \
            const uint4 ka_ = *reinterpret_cast<const uint4 *>((Kr) + k_off((row0) + r, 2 * kk_ + h));                  \
            const uint4 va_ = *reinterpret_cast<const uint4 *>((Vr) + k_off((row0) + r, 2 * kk_ + h));                  \
            sa_ = h16<F>::mfma32(ka_, qf[kk_], sa_);     /* S^T  [key][q] */                                            \
            dp_ = h16<F>::mfma32(va_, gf[kk_], dp_);     /* dP^T [key][q] */                                            \
        }                                                                                                               \
        _Pragma("unroll") for (int e_ = 0; e_ < 16; ++e_) {                                                             \
            float pv_ = __builtin_amdgcn_exp2f(fmaf(sa_[e_], c, -l2));                                                  \
            if (need_mask) {                                                                                            \
                const int kx_ = (key_first) + (e_ & 3) + 8 * (e_ >> 2) + 4 * h;                                         \
                if (kx_ >= T || (CAUSAL && kx_ > qrow)) pv_ = 0.f;                                                      \
            }                                                                                                           \
            dp_[e_] = pv_ * (dp_[e_] - dl) * scale;                                                                     \
        }                                                                                                               \
        _Pragma("unroll") for (int s_ = 0; s_ < 2; ++s_) {                                                              \
            const uint4 df_ = pack8<F>(dp_, s_);                                                                        \
            _Pragma("unroll") for (int dtile_ = 0; dtile_ < 2; ++dtile_) {                                              \
                const uint4 kt_ = tr_frag((Kt), (row0) + 16 * s_ + tr_row, tr_dbyte + 64 * dtile_);      /* K^T */      \
                dqt[dtile_] = h16<F>::mfma32(kt_, df_, dqt[dtile_]);                                                    \
            }                                                                                                           \
        }                                                                                                               \
    } while (0)

// ---- row stores: the lane's row of a transposed accumulator pair (C layout: dimensions 32 dtile + 8 gq + 4 h .. + 3 in elements
// 4 gq .. 4 gq + 3).  dK and dV go out interleaved, piece by piece.
// rounded to the 16-bit format F
template <typename F>
__device__ __forceinline__ void attn_store_dkdv16(bf16_t *ok, bf16_t *ov, const f32x16_t (&dkt)[2], const f32x16_t (&dvt)[2], int h)
{
#pragma unroll
    for (int dtile = 0; dtile < 2; ++dtile)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int d = 32 * dtile + 8 * gq + 4 * h;
            *reinterpret_cast<uint2 *>(ok + d) = make_uint2(h16<F>::pack2(dkt[dtile][4 * gq], dkt[dtile][4 * gq + 1]),
                                                             h16<F>::pack2(dkt[dtile][4 * gq + 2], dkt[dtile][4 * gq + 3]));
            *reinterpret_cast<uint2 *>(ov + d) = make_uint2(h16<F>::pack2(dvt[dtile][4 * gq], dvt[dtile][4 * gq + 1]),
                                                             h16<F>::pack2(dvt[dtile][4 * gq + 2], dvt[dtile][4 * gq + 3]));
        }
}
// a SHARED key of the prefix layout: this virtual sequence's contribution as fp32, to its partial slot [b][key][K | V][H * HD]; the
// slots are folded in a fixed order by attn_prefix_reduce (no atomics)
__device__ __forceinline__ void attn_store_dkdv_part(float *pk, float *pv, const f32x16_t (&dkt)[2], const f32x16_t (&dvt)[2], int h)
{
#pragma unroll
    for (int dtile = 0; dtile < 2; ++dtile)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int d = 32 * dtile + 8 * gq + 4 * h;
            *reinterpret_cast<float4 *>(pk + d) = make_float4(dkt[dtile][4 * gq], dkt[dtile][4 * gq + 1], dkt[dtile][4 * gq + 2], dkt[dtile][4 * gq + 3]);
            *reinterpret_cast<float4 *>(pv + d) = make_float4(dvt[dtile][4 * gq], dvt[dtile][4 * gq + 1], dvt[dtile][4 * gq + 2], dvt[dtile][4 * gq + 3]);
        }
}
// dQ rounded to the 16-bit format F
template <typename F>
__device__ __forceinline__ void attn_store_dq16(bf16_t *oq, const f32x16_t (&dqt)[2], int h)
{
#pragma unroll
    for (int dtile = 0; dtile < 2; ++dtile)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
            *reinterpret_cast<uint2 *>(oq + 32 * dtile + 8 * gq + 4 * h) =
                make_uint2(h16<F>::pack2(dqt[dtile][4 * gq], dqt[dtile][4 * gq + 1]),
                           h16<F>::pack2(dqt[dtile][4 * gq + 2], dqt[dtile][4 * gq + 3]));
}
