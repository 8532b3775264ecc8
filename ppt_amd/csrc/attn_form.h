// attn_form.h -- AttnForm<FORM>: what differs between the operand forms of the streaming attention forward kernels
// (attention_mfma.hip: attn_fwd_stream; attention_ragged.hip: attn_fwd_ragged).  FORM = PPT_BF16 / PPT_F16: the 16-bit q / k / v
// as they are, one LDS image of K and of V, one MFMA per fragment; FORM = PPT_F32 (split16): fp32 q / k / v with every operand
// of the two products split into hi + lo IEEE-half pairs (attn_common.h), two LDS images, three MFMAs per fragment.  Both
// kernels compute S^T = K . Q^T and O^T = V^T . P with these members, so a key tile laid out the same way gives the same bits.
// Internal: nothing here is part of include/ppt_hip.h.
#pragma once
#include <type_traits>
#include "attn_common.h"

namespace {

template <int FORM> struct AttnForm {                              // the 16-bit forms
    using F = typename std::conditional<FORM == PPT_BF16, bf16_t, f16_t>::type;
    using T = bf16_t;                                              // element of qkv / out (raw 16 bits of either format)
    using chunk_t = uint4;                                         // 16 staged bytes: 8 elements
    static constexpr int IMAGES = 1, CH_SHIFT = 3;                 // LDS images per K or V tile; log2(16-byte chunks per row)
    static constexpr float P_PRE = 1.0f;
    // Q^T: lane (r, h) holds dimensions 16 kk + 8 h .. + 7 of its query row as raw[kk][..]; here that is the B fragment itself
    struct Q { chunk_t raw[4][1]; };

    static __device__ __forceinline__ chunk_t zero() { return make_uint4(0, 0, 0, 0); }
    static __device__ __forceinline__ void prep_q(Q &, int) {}
    static __device__ __forceinline__ void write(unsigned char *kimg, unsigned char *vimg, int row, int ch, const chunk_t &k, const chunk_t &v)
    {
        *reinterpret_cast<uint4 *>(kimg + k_off(row, ch)) = k;
        *reinterpret_cast<uint4 *>(vimg + v_off(row, ch * 16)) = v;
    }
    // this lane's 32 of the 64 terms of q . k_last
    static __device__ __forceinline__ float peel_dot(const T *kl, const Q &q, int h)
    {
        float dot = 0.f;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const uint4 kv = *reinterpret_cast<const uint4 *>(kl + 16 * kk + 8 * h);
            const uint4 qv = q.raw[kk][0];
            const uint32_t kw[4] = {kv.x, kv.y, kv.z, kv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dot = fmaf(h16<F>::lo(kw[e]), h16<F>::lo(qw[e]), dot);
                dot = fmaf(h16<F>::hi(kw[e]), h16<F>::hi(qw[e]), dot);
            }
        }
        return dot;
    }
    static __device__ __forceinline__ void peel_o(const T *vl, int h, f32x16_t (&ot)[2])
    {
#pragma unroll
        for (int dtile = 0; dtile < 2; ++dtile)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const uint2 vv = *reinterpret_cast<const uint2 *>(vl + 32 * dtile + 8 * gq + 4 * h);
                ot[dtile][4 * gq + 0] = h16<F>::lo(vv.x); ot[dtile][4 * gq + 1] = h16<F>::hi(vv.x);
                ot[dtile][4 * gq + 2] = h16<F>::lo(vv.y); ot[dtile][4 * gq + 3] = h16<F>::hi(vv.y);
            }
    }
    static __device__ __forceinline__ void qk(f32x16_t (&st)[2], const unsigned char *Kc, const Q &q, int r, int h)
    {
        // all eight K fragments first (independent ds_read_b128, one wait), then the MFMAs: loaded one by one, each
        // MFMA waited for its own LDS round trip
        uint4 kf[4][2];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) kf[kk][sub] = *reinterpret_cast<const uint4 *>(Kc + k_off(32 * sub + r, 2 * kk + h));
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) st[sub] = h16<F>::mfma32(kf[kk][sub], q.raw[kk][0], st[sub]);
    }
    // P (still in the S^T accumulator layout) -> B fragments of the 16-key k-steps, then O^T += V^T . P
    static __device__ __forceinline__ void pv(f32x16_t (&ot)[2], const f32x16_t (&st)[2], const unsigned char *Vc, int tr_key, int tr_dbyte)
    {
        uint4 pf[2][2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int s = 0; s < 2; ++s) pf[sub][s] = pack8<F>(st[sub], s);
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int dtile = 0; dtile < 2; ++dtile)
                    ot[dtile] = h16<F>::mfma32(tr_frag(Vc, 32 * sub + 16 * s + tr_key, tr_dbyte + 64 * dtile), pf[sub][s], ot[dtile]);
    }
    static __device__ __forceinline__ void store_o(T *ob, const f32x16_t (&ot)[2], float inv, int h)
    {
#pragma unroll
        for (int dtile = 0; dtile < 2; ++dtile)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const uint2 u = make_uint2(h16<F>::pack2(ot[dtile][4 * gq + 0] * inv, ot[dtile][4 * gq + 1] * inv),
                                           h16<F>::pack2(ot[dtile][4 * gq + 2] * inv, ot[dtile][4 * gq + 3] * inv));
                *reinterpret_cast<uint2 *>(ob + 32 * dtile + 8 * gq + 4 * h) = u;
            }
    }
};

template <> struct AttnForm<PPT_F32> {                             // split16: the same members over hi + lo half pairs
    using T = float;
    using chunk_t = float4;                                        // 16 staged bytes: 4 elements
    static constexpr int IMAGES = 2, CH_SHIFT = 4;
    static constexpr float P_PRE = 1024.0f;                        // P is split as P x 2^10, O carries the factor to the end
    struct Q { chunk_t raw[4][2]; uint4 h[4], l[4]; };             // the fp32 values (for the peel) and their hi and lo halves

    static __device__ __forceinline__ chunk_t zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
    static __device__ __forceinline__ void prep_q(Q &q, int kk) { split8(q.raw[kk][0], q.raw[kk][1], q.h[kk], q.l[kk]); }
    // the split: 4 floats -> 8 bytes of the hi image + 8 of the lo image
    static __device__ __forceinline__ void write(unsigned char *kimg, unsigned char *vimg, int row, int ch, const chunk_t &k, const chunk_t &v)
    {
        uint2 hi, lo;
        split2(k.x, k.y, hi.x, lo.x); split2(k.z, k.w, hi.y, lo.y);
        const int ko = k_off(row, ch >> 1) + (ch & 1) * 8;
        *reinterpret_cast<uint2 *>(kimg + ko) = hi;
        *reinterpret_cast<uint2 *>(kimg + TILE + ko) = lo;
        split2(v.x, v.y, hi.x, lo.x); split2(v.z, v.w, hi.y, lo.y);
        const int vo = v_off(row, ch * 8);
        *reinterpret_cast<uint2 *>(vimg + vo) = hi;
        *reinterpret_cast<uint2 *>(vimg + TILE + vo) = lo;
    }
    static __device__ __forceinline__ float peel_dot(const T *kl, const Q &q, int h)      // fp32 throughout
    {
        float dot = 0.f;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const float4 k0 = *reinterpret_cast<const float4 *>(kl + 16 * kk + 8 * h);
            const float4 k1 = *reinterpret_cast<const float4 *>(kl + 16 * kk + 8 * h + 4);
            dot = fmaf(k0.x, q.raw[kk][0].x, dot); dot = fmaf(k0.y, q.raw[kk][0].y, dot);
            dot = fmaf(k0.z, q.raw[kk][0].z, dot); dot = fmaf(k0.w, q.raw[kk][0].w, dot);
            dot = fmaf(k1.x, q.raw[kk][1].x, dot); dot = fmaf(k1.y, q.raw[kk][1].y, dot);
            dot = fmaf(k1.z, q.raw[kk][1].z, dot); dot = fmaf(k1.w, q.raw[kk][1].w, dot);
        }
        return dot;
    }
    static __device__ __forceinline__ void peel_o(const T *vl, int h, f32x16_t (&ot)[2])
    {
#pragma unroll
        for (int dtile = 0; dtile < 2; ++dtile)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const float4 vv = *reinterpret_cast<const float4 *>(vl + 32 * dtile + 8 * gq + 4 * h);
                ot[dtile][4 * gq + 0] = vv.x * P_PRE; ot[dtile][4 * gq + 1] = vv.y * P_PRE;
                ot[dtile][4 * gq + 2] = vv.z * P_PRE; ot[dtile][4 * gq + 3] = vv.w * P_PRE;
            }
    }
    static __device__ __forceinline__ void qk(f32x16_t (&st)[2], const unsigned char *Kh, const Q &q, int r, int h)
    {
        const unsigned char *Kl = Kh + TILE;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            uint4 kh[2], kl[2];
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                const int o = k_off(32 * sub + r, 2 * kk + h);
                kh[sub] = *reinterpret_cast<const uint4 *>(Kh + o);
                kl[sub] = *reinterpret_cast<const uint4 *>(Kl + o);
            }
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) st[sub] = mfma3(kh[sub], kl[sub], q.h[kk], q.l[kk], st[sub]);
        }
    }
    static __device__ __forceinline__ void pv(f32x16_t (&ot)[2], const f32x16_t (&st)[2], const unsigned char *Vh, int tr_key, int tr_dbyte)
    {
        const unsigned char *Vl = Vh + TILE;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                uint4 ph, pl;
                split_acc(st[sub], s, ph, pl);
#pragma unroll
                for (int dtile = 0; dtile < 2; ++dtile) {
                    const uint4 vh = tr_frag(Vh, 32 * sub + 16 * s + tr_key, tr_dbyte + 64 * dtile);
                    const uint4 vl = tr_frag(Vl, 32 * sub + 16 * s + tr_key, tr_dbyte + 64 * dtile);
                    ot[dtile] = mfma3(vh, vl, ph, pl, ot[dtile]);
                }
            }
    }
    static __device__ __forceinline__ void store_o(T *ob, const f32x16_t (&ot)[2], float inv, int h)
    {
#pragma unroll
        for (int dtile = 0; dtile < 2; ++dtile)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
                *reinterpret_cast<float4 *>(ob + 32 * dtile + 8 * gq + 4 * h) =
                    make_float4(ot[dtile][4 * gq + 0] * inv, ot[dtile][4 * gq + 1] * inv, ot[dtile][4 * gq + 2] * inv, ot[dtile][4 * gq + 3] * inv);
    }
};

}  // namespace
