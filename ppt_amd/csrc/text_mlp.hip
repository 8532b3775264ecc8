// text_mlp.hip -- round 6: the MLP half of a CLIP text-tower layer as ONE launch per direction (ULIP_models.py:41-42, 49-51:
//     mlp = Sequential(c_fc: Linear(512, 2048), QuickGELU, c_proj: Linear(2048, 512));  x = x + mlp(ln_2(x))).
// On the prompt chain (817 rows with the shared prefix) the two linears were two dependent launches of the 64 x 64 tile loop --
// c_fc 12 us, c_proj (split-K 4) 10 us, and the 817 x 2048 hidden tensor written and read back in between -- in each direction,
// twelve layers deep, on the step's critical path.  What bounds such a launch is not FLOPs (13.7 GFLOP) but what ONE CU can pull
// out of L2 (48 B/clk with eight waves, tools/wstream_bench.hip) times how little of the weight each workgroup needs.
//
// Here a workgroup takes a 32-row block AND a 256-unit slice of the hidden dimension:
//     U[32, 256]   = act( A[32, 512] . W1[slice, :]^T (+ b1) )           16 k-steps, a wave owns 32 hidden units (2 x 1 register blocking)
//     P_s[32, 512] = U . W2[:, slice]^T                                  8 k-steps, a wave owns 64 output columns
// so it streams 2 x 256 KB of weights (5 us at the CU's rate), the hidden activation never leaves LDS, and the eight slices'
// partial products [8, M, 512] fp32 are added up -- with the residual and the bias -- by the LayerNorm kernel that reads the result
// anyway (ppt_layernorm_fwd_sum / ppt_layernorm_bwd_sum: fixed slice order, no atomics).  26 row blocks x 8 slices = 208 workgroups;
// blockIdx % 8 is the slice, so the workgroups of one XCD share one slice of the weights in its L2.  Measured alone at 817 rows
// (tools/text_mlp_bench.py): 20.2 us for the two launches -> 15.9 us with 64-row blocks (104 workgroups) -> 11.4 us with 32-row
// blocks; ring depths 4 / 8 make no difference (the workgroup's lifetime is its 2 x 128 MFMAs per wave plus four memory round trips).
//   forward  (mode 0): act = QuickGELU, W1 = c_fc.weight [2048, 512], W2 = c_proj.weight [512, 2048]; the pre-activation is saved
//                      (`pre`) when a backward will follow;
//   backward (mode 1): A = d out, W1 = c_proj.weight^T [2048, 512], W2 = c_fc.weight^T [512, 2048],
//                      U = (A . W1^T) * QuickGELU'(pre): the input gradient of the whole branch (the tower is frozen: no dW).
// Both weights arrive in fragment order (ppt_text_mlp_retile / ppt_text_mlp_retile_split), each wave's fragments of a slice
// contiguous, through register rings fed from one running scalar offset (csrc/mlp_fused3.hip).
//
// Two operand forms of one kernel template (FORM), as in csrc/text_lin.hip:
//   * PPT_BF16 / PPT_F16: the 16-bit operands of the mixed mode as they are -- one LDS image of A and of U, one MFMA per fragment
//     pair, the bias seeds the accumulator, `pre` is 16-bit;
//   * PPT_F32 (split16): fp32 operands multiplied as hi + lo IEEE-half pairs (gemm_common.h) -- the whole-model split16 mode, and the
//     mixed mode on weights whose text tower failed its load-time self-check (ULIP_WITH_IMAGE.calibrate_text_precision;
//     tools/ckpt_like_text_halves.py shows that BOTH halves of a layer need the fp32-grade products there).  The rows of A are
//     multiplied by 2^a_pow2, saturated to half's range (counted: ppt_text_mlp_params.split_overflow) and split ONCE while they are
//     staged: a hi image and a lo image; both weights are split ONCE per weight version by ppt_text_mlp_retile_split (x 2^b_pow2),
//     a fragment's hi KiB followed by its lo KiB; every product is three MFMAs (w_hi a_lo + w_lo a_hi + w_hi a_hi; lo x lo,
//     < 2^-22 relative, dropped), the accumulator is multiplied by 2^-(a_pow2 + b_pow2) afterwards and THEN the bias is added; the
//     activation's output is split the same way into the U images; `pre` is fp32.  2 x 512 KB of weight halves per workgroup and
//     102 KB of LDS: one workgroup per CU.
#include "ppt_common.h"
#include "gemm_common.h"

namespace {

constexpr int D = 512, HID = 2048, SL = 256, NS = HID / SL;        // model width, hidden width, hidden slice, slices
#ifndef PPT_TMLP_RB
#define PPT_TMLP_RB 2
#endif
#ifndef PPT_TMLP_D1
#define PPT_TMLP_D1 4
#endif
#ifndef PPT_TMLP_D2
#define PPT_TMLP_D2 4
#endif
constexpr int AP = 2 * D + 32, UP = 2 * SL + 32;                   // LDS pitches (bytes): = 32 mod 256
constexpr int K1 = D / 32, K2 = SL / 32;                           // k-steps of the two products (16 / 8)

template <int FORM> struct MlpForm {                               // the 16-bit forms (tools/build_variant.sh sets RB / D1 / D2 for A/B)
    using T = typename std::conditional<FORM == PPT_BF16, bf16_t, f16_t>::type;
    using Pre = T;                                                 // the saved pre-activation
    static constexpr bool SPLIT = false;
    static constexpr int PARTS = 1;                                // KiB pieces of a weight fragment = LDS images of A and of U
    static constexpr int RB = PPT_TMLP_RB;                         // row blocks of 16 per workgroup
    static constexpr int D1 = PPT_TMLP_D1, D2 = PPT_TMLP_D2;       // ring depths in k-steps (must divide 16 / 8)
};
template <> struct MlpForm<PPT_F32> {
    using T = f16_t;
    using Pre = float;
    static constexpr bool SPLIT = true;
    static constexpr int PARTS = 2;
    static constexpr int RB = 2;
    static constexpr int D1 = 4, D2 = 2;
};
template <typename F> struct MlpShape {
    static constexpr int R = 16 * F::RB;                           // rows per workgroup
    static constexpr int A_BYTES = R * AP, U_BYTES = R * UP;       // ONE image (hi or lo, or the 16-bit one)
    static constexpr int LDS_BYTES = F::PARTS * (A_BYTES + U_BYTES);
    static constexpr int WAVE_SLICE = F::PARTS * 32 * 1024;        // bytes of one wave's fragments per slice (either weight)
    static constexpr int W_BYTES = F::PARTS * HID * D * 2;
    static_assert(!F::SPLIT || F::RB == 2, "two hi + lo image pairs at RB = 4 do not fit the 160 KB LDS");
};

// a value on its way into an LDS image: split16 multiplies it by 2^a_pow2 and saturates it to half's range (counted)
template <typename F>
__device__ __forceinline__ float prep(float v, float sa, uint32_t &over)
{
    if constexpr (F::SPLIT) return split_saturate(v * sa, over);
    else return v;
}
// four prepared values of a row -> their 8 bytes of the image (16-bit forms: rounded) / of the hi and of the lo image (split16)
template <typename F>
__device__ __forceinline__ void put4(unsigned char *hi, unsigned char *lo, const float (&x)[4])
{
    if constexpr (F::SPLIT) {
        uint2 H, L;
        split4(x, H, L);
        *reinterpret_cast<uint2 *>(hi) = H;
        *reinterpret_cast<uint2 *>(lo) = L;
    } else {
        *reinterpret_cast<uint2 *>(hi) = make_uint2(h16<typename F::T>::pack2(x[0], x[1]), h16<typename F::T>::pack2(x[2], x[3]));
    }
}

// one product of the pair over KS k-steps: acc[rb][nb] += (this wave's weight fragments, ring g refilled by next()) . rows^T (transposed
// product: a lane holds four columns of a row).  `img` is this lane's place in the LDS image of the rows (pitch PITCH, the lo image
// LO_OFF further), read one k-step ahead.  split16: three MFMAs per fragment pair, a fragment's hi KiB then its lo KiB in the ring.
template <typename F, int NB, int KS, int DEPTH, int PITCH, int LO_OFF, typename Next>
__device__ __forceinline__ void product(ppt_f32x4 (&acc)[F::RB][NB], const unsigned char *img, uint4 (&g)[DEPTH][NB * F::PARTS], Next next)
{
    using T = typename F::T;
    constexpr int RB = F::RB;
    uint4 fh[2][RB], fl[2][RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        fh[0][rb] = *reinterpret_cast<const uint4 *>(img + rb * 16 * PITCH);
        if constexpr (F::SPLIT) fl[0][rb] = *reinterpret_cast<const uint4 *>(img + LO_OFF + rb * 16 * PITCH);
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if (ks + 1 < KS) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                fh[(ks + 1) & 1][rb] = *reinterpret_cast<const uint4 *>(img + rb * 16 * PITCH + 64 * (ks + 1));
                if constexpr (F::SPLIT) fl[(ks + 1) & 1][rb] = *reinterpret_cast<const uint4 *>(img + LO_OFF + rb * 16 * PITCH + 64 * (ks + 1));
            }
        }
        if constexpr (F::SPLIT) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const uint4 wh = g[ks % DEPTH][2 * nb], wl = g[ks % DEPTH][2 * nb + 1];
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    acc[rb][nb] = h16<T>::mfma16(wh, fl[ks & 1][rb], acc[rb][nb]);
                    acc[rb][nb] = h16<T>::mfma16(wl, fh[ks & 1][rb], acc[rb][nb]);
                    acc[rb][nb] = h16<T>::mfma16(wh, fh[ks & 1][rb], acc[rb][nb]);
                }
            }
        } else {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[rb][nb] = h16<T>::mfma16(g[ks % DEPTH][nb], fh[ks & 1][rb], acc[rb][nb]);
        }
        if (ks + DEPTH < KS) next(g[ks % DEPTH]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// LN (forward only): A is the fp32 residual stream x_mid and ln_2 (ULIP_models.py:21-27, 50: LayerNorm computed in fp32) is applied
// while the block's rows are staged -- 16 threads per row, two-pass statistics over DPP adds as in rowgemm.hip -- so the LayerNorm
// launch in front of this kernel goes too; the eight slices' workgroups of a row block recompute it (64 KB of rows each, L2-warm),
// slice 0 writes the statistics the LayerNorm backward needs.
template <int FORM, int MODE, bool LN>
__global__ __launch_bounds__(512, 2) void text_mlp_kernel(const ppt_text_mlp_params p)
{
    using F = MlpForm<FORM>;
    using T = typename F::T;
    using S = MlpShape<F>;
    using Pre = typename F::Pre;
    using Pre4 = typename std::conditional<F::SPLIT, float4, uint2>::type;      // this lane's four of a row
    constexpr int RB = F::RB, R = S::R, A_BYTES = S::A_BYTES, U_BYTES = S::U_BYTES, D1 = F::D1, D2 = F::D2;
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char *ai = smem, *ui = smem + F::PARTS * A_BYTES;       // split16: hi image, lo image at + A_BYTES / + U_BYTES
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, kg = lane >> 4, lo16 = lane * 16;
    PPT_PRIO(p.wave_prio);
    const int s = blockIdx.x % NS, row0 = (blockIdx.x / NS) * R;
    const int nrow = min(R, p.M - row0);
    const float sa = F::SPLIT ? pow2f(p.split_a_pow2) : 1.0f, inv = F::SPLIT ? pow2f(-(p.split_a_pow2 + p.split_b_pow2)) : 1.0f;
    uint32_t over = 0;

    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.W1), 0, S::W_BYTES, 0x00020000);
    const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.W2), 0, S::W_BYTES, 0x00020000);
    int o1 = (s * 8 + w) * S::WAVE_SLICE, o2 = o1;
    // one k-step of W1: [h < 2] x 1 KiB, of W2: [nb < 4] x 1 KiB (split16: x [hi, lo])
    auto next1 = [&](uint4 (&f)[2 * F::PARTS]) {
#pragma unroll
        for (int i = 0; i < 2 * F::PARTS; ++i) f[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r1, lo16 + 1024 * i, o1, 0));
        o1 += 2048 * F::PARTS;
    };
    auto next2 = [&](uint4 (&f)[4 * F::PARTS]) {
#pragma unroll
        for (int i = 0; i < 4 * F::PARTS; ++i) f[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r2, lo16 + 1024 * i, o2, 0));
        o2 += 4096 * F::PARTS;
    };
    // the first k-steps of W1 are requested before anything else: they do not depend on the rows
    uint4 g1[D1][2 * F::PARTS];
#pragma unroll
    for (int i = 0; i < D1; ++i) next1(g1[i]);

    // ---- the block's rows of A -> LDS image(s) (rows past M: zeros)
    if constexpr (LN) {
        static_assert(R == 32 && D == 512, "16 threads per row x 32 rows = the workgroup");
        const int r = threadIdx.x >> 4, j = threadIdx.x & 15;
        const float *src = (const float *)p.A + (size_t)(row0 + min(r, nrow - 1)) * p.lda;
        float4 xf[D / 64];
#pragma unroll
        for (int i = 0; i < D / 64; ++i) xf[i] = *reinterpret_cast<const float4 *>(src + 4 * (j + 16 * i));
        float sm = 0.f;
#pragma unroll
        for (int i = 0; i < D / 64; ++i) sm += (xf[i].x + xf[i].y) + (xf[i].z + xf[i].w);
        const float mean = row16_sum(sm) * (1.0f / (float)D);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < D / 64; ++i) {
            const float d0 = xf[i].x - mean, d1 = xf[i].y - mean, d2 = xf[i].z - mean, d3 = xf[i].w - mean;
            q = fmaf(d0, d0, q); q = fmaf(d1, d1, q); q = fmaf(d2, d2, q); q = fmaf(d3, d3, q);
        }
        const float rstd = 1.0f / sqrtf(row16_sum(q) * (1.0f / (float)D) + p.ln_eps);
        if (p.ln_mean && s == 0 && j == 0 && r < nrow) { p.ln_mean[row0 + r] = mean; p.ln_rstd[row0 + r] = rstd; }
#pragma unroll
        for (int i = 0; i < D / 64; ++i) {
            const int c = 4 * (j + 16 * i);
            const float4 g = *reinterpret_cast<const float4 *>(p.ln_w + c), b = *reinterpret_cast<const float4 *>(p.ln_b + c);
            float x[4] = {0.f, 0.f, 0.f, 0.f};
            if (r < nrow) {
                x[0] = prep<F>((xf[i].x - mean) * rstd * g.x + b.x, sa, over); x[1] = prep<F>((xf[i].y - mean) * rstd * g.y + b.y, sa, over);
                x[2] = prep<F>((xf[i].z - mean) * rstd * g.z + b.z, sa, over); x[3] = prep<F>((xf[i].w - mean) * rstd * g.w + b.w, sa, over);
            }
            put4<F>(ai + r * AP + 2 * c, ai + A_BYTES + r * AP + 2 * c, x);
        }
    } else if constexpr (F::SPLIT) {
        const float *A = (const float *)p.A;
        constexpr int PIECES = R * (D / 4);                          // float4 pieces of the block (4096)
        float4 v[PIECES / 512];
#pragma unroll
        for (int it = 0; it < PIECES / 512; ++it) {
            const int i = threadIdx.x + 512 * it, lr = i / (D / 4), c4 = i % (D / 4);
            v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (lr < nrow) v[it] = *reinterpret_cast<const float4 *>(A + (size_t)(row0 + lr) * p.lda + 4 * c4);
        }
#pragma unroll
        for (int it = 0; it < PIECES / 512; ++it) {
            const int i = threadIdx.x + 512 * it, lr = i / (D / 4), c4 = i % (D / 4);
            const float x[4] = {prep<F>(v[it].x, sa, over), prep<F>(v[it].y, sa, over), prep<F>(v[it].z, sa, over), prep<F>(v[it].w, sa, over)};
            put4<F>(ai + lr * AP + 8 * c4, ai + A_BYTES + lr * AP + 8 * c4, x);
        }
    } else {
        const T *A = (const T *)p.A;
#pragma unroll
        for (int it = 0; it < R * (D / 8) / 512; ++it) {
            const int i = threadIdx.x + 512 * it, lr = i / (D / 8), c8 = i % (D / 8);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (lr < nrow) v = *reinterpret_cast<const uint4 *>(A + (size_t)(row0 + lr) * p.lda + 8 * c8);
            *reinterpret_cast<uint4 *>(ai + lr * AP + 16 * c8) = v;
        }
    }
    // the saved pre-activation (backward) and the bias (forward) of this lane's hidden units: requested now
    Pre4 prev[RB][2];
    float4 bv[2];
    const int hcol = SL * s + 32 * w + 4 * kg;                       // + 16 h: this lane's four hidden units of half h
    if (MODE == 1) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int m = row0 + min(16 * rb + l15, nrow - 1);
                prev[rb][h] = *reinterpret_cast<const Pre4 *>((const Pre *)p.pre + (size_t)m * HID + hcol + 16 * h);
            }
    } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) bv[h] = p.b1 ? *reinterpret_cast<const float4 *>(p.b1 + hcol + 16 * h) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    lds_barrier();

    // ---- product 1: a1[rb][h] = W1[slice, this wave's 32 units] . A^T; the 16-bit forms' accumulator starts from the bias
    ppt_f32x4 a1[RB][2];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int h = 0; h < 2; ++h)
            a1[rb][h] = (MODE == 0 && !F::SPLIT) ? ppt_f32x4{bv[h].x, bv[h].y, bv[h].z, bv[h].w} : ppt_f32x4{0.f, 0.f, 0.f, 0.f};
    product<F, 2, K1, D1, AP, A_BYTES>(a1, ai + l15 * AP + 16 * kg, g1, next1);
    // the first k-steps of W2 fly under the activation
    uint4 g2[D2][4 * F::PARTS];
#pragma unroll
    for (int i = 0; i < D2; ++i) next2(g2[i]);
    // ---- (split16: un-scale, bias,) activation -> the U image(s); forward: the pre-activation is saved for the backward
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float v[4] = {a1[rb][h][0], a1[rb][h][1], a1[rb][h][2], a1[rb][h][3]};
            if constexpr (F::SPLIT) {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] *= inv;
            }
            const int lr = 16 * rb + l15;
            if (MODE == 0) {
                if constexpr (F::SPLIT) { v[0] += bv[h].x; v[1] += bv[h].y; v[2] += bv[h].z; v[3] += bv[h].w; }
                if (p.pre && lr < nrow) {
                    Pre4 *dst = reinterpret_cast<Pre4 *>((Pre *)p.pre + (size_t)(row0 + lr) * HID + hcol + 16 * h);
                    if constexpr (F::SPLIT) *dst = make_float4(v[0], v[1], v[2], v[3]);
                    else *dst = make_uint2(h16<T>::pack2(v[0], v[1]), h16<T>::pack2(v[2], v[3]));
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = v[i] / (1.0f + __expf(-1.702f * v[i]));                 // QuickGELU (ULIP_models.py:30-32)
            } else {
                float x[4];
                if constexpr (F::SPLIT) { x[0] = prev[rb][h].x; x[1] = prev[rb][h].y; x[2] = prev[rb][h].z; x[3] = prev[rb][h].w; }
                else { x[0] = h16<T>::lo(prev[rb][h].x); x[1] = h16<T>::hi(prev[rb][h].x); x[2] = h16<T>::lo(prev[rb][h].y); x[3] = h16<T>::hi(prev[rb][h].y); }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float sg = 1.0f / (1.0f + __expf(-1.702f * x[i]));
                    v[i] *= sg * (1.0f + 1.702f * x[i] * (1.0f - sg));
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = prep<F>(v[i], sa, over);
            // (both addresses spelled out from `ui`: given `dst` and `dst + U_BYTES` the compiler pairs the hi / lo stores differently)
            put4<F>(ui + lr * UP + (32 * w + 16 * h + 4 * kg) * 2, ui + U_BYTES + lr * UP + (32 * w + 16 * h + 4 * kg) * 2, v);
        }
    lds_barrier();

    // ---- product 2: acc[rb][nb] = W2[this wave's 64 columns, slice] . U^T
    ppt_f32x4 acc[RB][4];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[rb][nb] = ppt_f32x4{0.f, 0.f, 0.f, 0.f};
    product<F, 4, K2, D2, UP, U_BYTES>(acc, ui + l15 * UP + 16 * kg, g2, next2);
    // ---- the slice's partial product: parts[s][row][64 w + 16 nb + 4 kg ..]
    float *out = p.parts + (size_t)s * p.M * D;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int lr = 16 * rb + l15;
        if (lr < nrow) {
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                float v[4] = {acc[rb][nb][0], acc[rb][nb][1], acc[rb][nb][2], acc[rb][nb][3]};
                if constexpr (F::SPLIT) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] *= inv;
                }
                *reinterpret_cast<float4 *>(out + (size_t)(row0 + lr) * D + 64 * w + 16 * nb + 4 * kg) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    }
    if constexpr (F::SPLIT) split_report(over, p.split_overflow);
}

// fragment order (see next1 / next2): thread -> one 16-byte piece of 8 consecutive k of each weight
//   W1t[s][w][ks < 16][h < 2][lane][8] = W1[256 s + 32 w + 16 h + l15][32 ks + 8 kg ..)      W1 [2048, 512] row-major
//   W2t[s][w][ks < 8][nb < 4][lane][8] = W2[64 w + 16 nb + l15][256 s + 32 ks + 8 kg ..)       W2 [512, 2048] row-major
// SPLIT: the weights are fp32, multiplied by 2^b_pow2, and a fragment becomes its hi KiB followed by its lo KiB ([..][hi, lo][lane][8]).
// (They are fitted into half's range by the caller, ULIP_WITH_IMAGE._fit_split16_range: saturated, not counted.)
__device__ __forceinline__ void split8(const float *src, float sb, unsigned char *dst)
{
    uint32_t over = 0;
    const float4 a = *reinterpret_cast<const float4 *>(src), b = *reinterpret_cast<const float4 *>(src + 4);
    const float x0[4] = {split_saturate(a.x * sb, over), split_saturate(a.y * sb, over), split_saturate(a.z * sb, over), split_saturate(a.w * sb, over)};
    const float x1[4] = {split_saturate(b.x * sb, over), split_saturate(b.y * sb, over), split_saturate(b.z * sb, over), split_saturate(b.w * sb, over)};
    uint2 h0, l0, h1, l1;
    split4(x0, h0, l0);
    split4(x1, h1, l1);
    *reinterpret_cast<uint4 *>(dst) = make_uint4(h0.x, h0.y, h1.x, h1.y);
    *reinterpret_cast<uint4 *>(dst + 1024) = make_uint4(l0.x, l0.y, l1.x, l1.y);
}

template <bool SPLIT>
__global__ __launch_bounds__(256) void text_mlp_retile_kernel(const void *__restrict__ W1, const void *__restrict__ W2,
                                                              unsigned char *__restrict__ W1t, unsigned char *__restrict__ W2t, int b_pow2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;                        // over NS * 8 * 32 * 64 pieces (both weights)
    if (i >= NS * 8 * 32 * 64) return;
    const int lane = i & 63, f = (i >> 6) & 31, w = (i >> 11) & 7, s = i >> 14;      // f = 2 ks + h (W1) = 4 ks + nb (W2)
    const int l15 = lane & 15, kg = lane >> 4;
    const size_t e1 = (size_t)(SL * s + 32 * w + 16 * (f & 1) + l15) * D + 32 * (f >> 1) + 8 * kg;
    const size_t e2 = (size_t)(64 * w + 16 * (f & 3) + l15) * HID + SL * s + 32 * (f >> 2) + 8 * kg;
    const size_t dst = (size_t)(i >> 6) * (SPLIT ? 2048 : 1024) + lane * 16;
    if constexpr (SPLIT) {
        const float sb = pow2f(b_pow2);
        split8((const float *)W1 + e1, sb, W1t + dst);
        split8((const float *)W2 + e2, sb, W2t + dst);
    } else {
        *reinterpret_cast<uint4 *>(W1t + dst) = *reinterpret_cast<const uint4 *>((const uint16_t *)W1 + e1);
        *reinterpret_cast<uint4 *>(W2t + dst) = *reinterpret_cast<const uint4 *>((const uint16_t *)W2 + e2);
    }
}

template <bool SPLIT>
int retile(const void *W1, const void *W2, void *W1t, void *W2t, int b_pow2, void *stream)
{
    if (!W1 || !W2 || !W1t || !W2t || (((uintptr_t)W1 | (uintptr_t)W2 | (uintptr_t)W1t | (uintptr_t)W2t) & 15) || abs(b_pow2) > 24) return PPT_EINVAL;
    hipLaunchKernelGGL(text_mlp_retile_kernel<SPLIT>, dim3((NS * 8 * 32 * 64 + 255) / 256), dim3(256), 0, ppt_stream(stream), W1, W2,
                       (unsigned char *)W1t, (unsigned char *)W2t, b_pow2);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

template <int FORM>
int launch(const ppt_text_mlp_params &p, void *stream)
{
    using S = MlpShape<MlpForm<FORM>>;
    constexpr bool LN_OK = S::R == 32;                                   // the LayerNorm prologue: 16 threads per row x 32 rows
    const bool ln = p.ln_w != nullptr;
    if (ln && !LN_OK) return PPT_EINVAL;
    PPT_RAISE_LDS_ONCE(S::LDS_BYTES, (const void *)text_mlp_kernel<FORM, 0, false>, (const void *)text_mlp_kernel<FORM, 1, false>,
                       (const void *)text_mlp_kernel<FORM, 0, LN_OK>);
    const dim3 grid(NS * ((p.M + S::R - 1) / S::R)), block(512);
    hipStream_t st = ppt_stream(stream);
    if (ln) hipLaunchKernelGGL((text_mlp_kernel<FORM, 0, LN_OK>), grid, block, S::LDS_BYTES, st, p);
    else if (p.mode == 0) hipLaunchKernelGGL((text_mlp_kernel<FORM, 0, false>), grid, block, S::LDS_BYTES, st, p);
    else hipLaunchKernelGGL((text_mlp_kernel<FORM, 1, false>), grid, block, S::LDS_BYTES, st, p);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

}  // namespace

extern "C" int ppt_text_mlp_retile(const void *W1, const void *W2, void *W1t, void *W2t, void *stream)
{
    return retile<false>(W1, W2, W1t, W2t, 0, stream);
}

extern "C" int ppt_text_mlp_retile_split(const float *W1, const float *W2, void *W1t, void *W2t, int b_pow2, void *stream)
{
    return retile<true>(W1, W2, W1t, W2t, b_pow2, stream);
}

extern "C" int ppt_text_mlp_pair(const ppt_text_mlp_params *pp, void *stream)
{
    if (!pp) return PPT_EINVAL;
    ppt_text_mlp_params p = *pp;
    if (!p.A || !p.W1 || !p.W2 || !p.parts || p.M <= 0 || p.lda < D) return PPT_EINVAL;
    if (p.D != D || p.hidden != HID) return PPT_EUNSUPPORTED;
    if (p.dtype != PPT_BF16 && p.dtype != PPT_F16 && p.dtype != PPT_F32) return PPT_EINVAL;
    if (p.mode != 0 && p.mode != 1) return PPT_EINVAL;
    if (p.mode == 1 && !p.pre) return PPT_EINVAL;
    if (((uintptr_t)p.A | (uintptr_t)p.W1 | (uintptr_t)p.W2 | (uintptr_t)p.parts | (uintptr_t)p.pre | (uintptr_t)p.b1) & 15) return PPT_EINVAL;
    const bool split = p.dtype == PPT_F32, ln = p.ln_w != nullptr;
    if (p.lda % (split || ln ? 4 : 8)) return PPT_EINVAL;                     // rows are read as 16-byte pieces: fp32 (split16, LN) or 16-bit
    if (split && (abs(p.split_a_pow2) > 24 || abs(p.split_b_pow2) > 24)) return PPT_EINVAL;
    if (ln && (p.mode != 0 || !p.ln_b || (((uintptr_t)p.ln_w | (uintptr_t)p.ln_b) & 15))) return PPT_EINVAL;
    if (p.wave_prio == 0) p.wave_prio = ppt_get_wave_priority();
    if (split) return launch<PPT_F32>(p, stream);                            // fp32 operands as hi + lo half pairs
    return p.dtype == PPT_F16 ? launch<PPT_F16>(p, stream) : launch<PPT_BF16>(p, stream);
}
