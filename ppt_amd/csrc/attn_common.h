// attn_common.h -- what the attention translation units (attention.hip, attention_mfma.hip, attention_split.hip) share besides the
// row addressing of attn_rowmap.h: tile constants, the two swizzled LDS images, the transposed read and its lane geometry, accumulator
// zeroing, the XCD block map, the hi + lo half split of the split16 form, and the launchers that cross from one file to another.  Internal: nothing here is part of include/ppt_hip.h.
#pragma once
#include "ppt_common.h"
#include "attn_rowmap.h"

typedef __attribute__((ext_vector_type(4))) short s4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

constexpr int HD = 64, KVT = 64, QB = 128, TILE = KVT * 128;   // bytes per image of a K or V tile (64 keys x 128 B of 16-bit values)
constexpr int QT = 32, QTILE = QT * 128;                       // query rows per staged tile of the dK / dV kernels, bytes per 32-row image

// row image (read row-wise, ds_read_b128) and transposed-read image (ds_read_b64_tr_b16): each with the swizzle that makes its
// read conflict-free
__device__ __forceinline__ int k_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
__device__ __forceinline__ int v_off(int key, int dbyte) { return key * 128 + (dbyte ^ (((key >> 1) & 1) << 6)); }

__device__ __forceinline__ uint4 tr_frag(const unsigned char *img, int row0, int dbyte)
{
    struct { s4_t a, b; } f;
    f.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4_t *)(img + v_off(row0, dbyte)));
    f.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4_t *)(img + v_off(row0 + 8, dbyte)));
    return __builtin_bit_cast(uint4, f);
}
// per-lane constant part of tr_frag's arguments: lane = 16 g + 4 q + p supplies row q, columns 4 p .. 4 p + 3.  Used by the 16-bit
// backward kernels; the forward kernels and attention_split.hip keep these three lines written out, because with the call their
// register allocation changed (tools/kernel_isa_diff.py, profiles/r14_attention_bwd.md).
__device__ __forceinline__ void tr_lane(int lane, int &tr_row, int &tr_dbyte)
{
    const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    tr_row = 4 * (g >> 1) + tq;                 // + the 16-row step's first row
    tr_dbyte = (16 * (g & 1) + 4 * tp) * 2;     // + 64 * dtile
}

// Two accumulators to zero, element by element (four: a loop over the pairs).  A macro: as a function (accumulators or arrays
// of them by reference) and as `= {}` at the declaration it moved the scalar set-up code of the backward kernels.
#define ATTN_ZERO2(a, b)                                                                            \
    do {                                                                                            \
        _Pragma("unroll") for (int e_ = 0; e_ < 16; ++e_) { (a)[e_] = 0.f; (b)[e_] = 0.f; }         \
    } while (0)

// Workgroup -> (query block, batch x head): the dispatcher deals consecutive workgroups round-robin to the 8 XCDs, each with an
// L2 of its own.  With the query blocks of one (batch, head) on consecutive workgroup ids its K / V rows were fetched from HBM
// by up to five XCDs (PMC: 139 MB read per launch at T = 513, B = 32 for 38 MB of qkv).  When the number of (batch, head)
// pairs is a multiple of 8 the ids are dealt so that all query blocks of a pair land on ONE XCD, next to each other in time.
__device__ __forceinline__ void attn_xcd_map(int xcd_map, int &qblk, int &bh)
{
    bh = blockIdx.y, qblk = blockIdx.x;
    if (xcd_map && (gridDim.y & 7) == 0) {
        const int lin = blockIdx.y * gridDim.x + blockIdx.x, slot = lin >> 3;
        bh = (slot / (int)gridDim.x) * 8 + (lin & 7);
        qblk = slot % (int)gridDim.x;
    }
}

// accumulator x (rows = the A operand's rows, column = lane & 31) -> the 16-bit B-operand fragment of 16-row step s
template <typename F>
__device__ __forceinline__ uint4 pack8(const f32x16_t &x, int s)
{
    return make_uint4(h16<F>::pack2(x[8 * s + 0], x[8 * s + 1]), h16<F>::pack2(x[8 * s + 2], x[8 * s + 3]),
                      h16<F>::pack2(x[8 * s + 4], x[8 * s + 5]), h16<F>::pack2(x[8 * s + 6], x[8 * s + 7]));
}

// ---- split16 (gemm_common.h): x = half(x) + half(x - half(x)), 22 significand bits; a product is three MFMAs, lo x lo dropped.
// (Unlike the GEMMs' split this one does not saturate beyond 65 504: the hi half of such a value is +-inf.)
typedef _Float16 h2_t __attribute__((ext_vector_type(2)));

// two fp32 values -> packed halves of their hi parts and of their lo parts
__device__ __forceinline__ void split2(float a, float b, uint32_t &hi, uint32_t &lo)
{
    const _Float16 ha = (_Float16)a, hb = (_Float16)b;
    const h2_t hh = {ha, hb};
    const h2_t ll = {(_Float16)(a - (float)ha), (_Float16)(b - (float)hb)};
    hi = __builtin_bit_cast(uint32_t, hh);
    lo = __builtin_bit_cast(uint32_t, ll);
}
__device__ __forceinline__ void split8(const float4 &u, const float4 &v, uint4 &hi, uint4 &lo)
{
    split2(u.x, u.y, hi.x, lo.x); split2(u.z, u.w, hi.y, lo.y);
    split2(v.x, v.y, hi.z, lo.z); split2(v.z, v.w, hi.w, lo.w);
}
__device__ __forceinline__ f32x16_t mfma3(uint4 ah, uint4 al, uint4 bh, uint4 bl, f32x16_t c)
{
    c = h16<f16_t>::mfma32(al, bh, c);
    c = h16<f16_t>::mfma32(ah, bl, c);
    return h16<f16_t>::mfma32(ah, bh, c);
}
// pack8's split16 form: hi / lo B-operand fragments of 16-row step s
__device__ __forceinline__ void split_acc(const f32x16_t &x, int s, uint4 &hi, uint4 &lo)
{
    split2(x[8 * s + 0], x[8 * s + 1], hi.x, lo.x); split2(x[8 * s + 2], x[8 * s + 3], hi.y, lo.y);
    split2(x[8 * s + 4], x[8 * s + 5], hi.z, lo.z); split2(x[8 * s + 6], x[8 * s + 7], hi.w, lo.w);
}

// ---- launchers that cross files.  fmt: PPT_BF16 or PPT_F16, the 16-bit operand format; form: those two or PPT_F32 (split16).
extern "C" {
// attention_mfma.hip
int ppt_attention_fwd_stream(const void *qkv, void *out, float *lse, int Bt, int T, int H, float scale, int causal, int P, int form,
                             hipStream_t s);
int ppt_attention_fwd_mfma_bf16(const void *qkv, void *out, float *lse, int Bt, int T, int H, float scale, int causal, int P, int fmt,
                                hipStream_t s);
int ppt_attention_bwd_mfma_bf16(const void *qkv, const void *dout, const float *lse, const float *delta, void *dqkv, int Bt, int T,
                                int H, float scale, int causal, int P, float *part, int fmt, hipStream_t s);
int ppt_attention_bwd_short_mfma_bf16(const void *qkv, const void *out, const void *dout, const float *lse, void *dqkv, int Bt, int T,
                                      int H, float scale, int causal, int P, float *part, int fmt, hipStream_t s);
// attention.hip
int ppt_attention_fwd_quad_bf16(const void *qkv, void *out, float *lse, int Bt, int T, int H, float scale, int causal, int P, int fmt,
                                hipStream_t s);
// fp32 dK / dV of the P shared rows = the Bt + 1 partial slots of `part` added in sequence order (attn_prefix_reduce<float>)
int ppt_attention_prefix_reduce_f32(const float *part, void *dqkv, int Bt, int P, int H, int prio, hipStream_t s);
}
