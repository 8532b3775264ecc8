// text_lin.hip -- ONE linear of the CLIP text tower's attention half, rows stationary and the weight streamed -- the first
// product of csrc/text_mlp.hip as a launch of its own.  On the prompt chain (817 rows with the shared
// prefix) these are in_proj (512 -> 1536), out_proj (512 -> 512, + bias + residual) and their two input-gradient products
// (512 -> 512; 1536 -> 512 as three K chunks whose partial products the LayerNorm backward adds up, as it did for the split-K tile
// GEMM): 48 of the chain's tile GEMMs per step -- 64 x 64 tiles whose K loop pays a global round trip and a barrier per 32 k.
//
// Two operand forms of one kernel template (FORM):
//   * PPT_F32 (round 6, split16): fp32 operands multiplied as hi + lo IEEE-half pairs (gemm_common.h), three MFMAs per fragment pair;
//   * PPT_F16 / PPT_BF16 (round 7): the 16-bit operands of the mixed mode as they are, one MFMA per fragment.
// A workgroup = a 32-row block x a slice of SLN output columns x one 512-wide K chunk:
//   * the block's rows of A (columns [512 c, 512 c + 512)) are staged ONCE into LDS: split16 multiplies them by 2^a_pow2, saturates
//     to half's range (counted) and keeps a hi and a lo image (68 KB); the 16-bit forms copy them into a single image (34 KB);
//   * the slice of W (re-tiled once per weight version by ppt_text_lin_retile_split / ppt_text_lin_retile16, fragment order; split16:
//     x 2^b_pow2, hi KiB then lo KiB) streams through a register ring; a wave owns SLN / 8 columns; fp32 accumulation;
//   * epilogue: (split16: x 2^-(a_pow2 + b_pow2)) (+ bias) (+ residual) -> fp32 C[M, N] or (16-bit forms) a 16-bit C rounded as
//     ppt_gemm rounds (h16<T>::pack2: beyond the format's range is +-inf), or the K chunk's fp32 partial product parts[c][M][N].
// SLN = 256 for N >= 1024 (in_proj: 26 x 6 = 156 workgroups), 128 below (N = 512: 26 x 4 (x 3 chunks) = 104 / 312 workgroups).
#include "ppt_common.h"
#include "gemm_common.h"

namespace {

constexpr int KC = 512;                                            // K chunk
constexpr int RB = 2, R = 16 * RB;
constexpr int AP = 2 * KC + 32;                                    // LDS pitch (bytes): = 32 mod 256
constexpr int A_BYTES = R * AP;                                    // ONE image (hi or lo, or the 16-bit one)
constexpr int K1 = KC / 32;                                        // k-steps (16)

// what both public entry points hand the kernel
struct LinArgs {
    const void *A; int64_t lda;                                    // FORM's operand type (split16: fp32) [M, K]
    const void *W;
    const float *bias;
    const float *residual; int64_t ld_res;
    void *C; int64_t ldc;                                          // fp32, or (c16) FORM's 16-bit type
    int M, N, K;
    int c16;
    int split_a_pow2, split_b_pow2; unsigned int *split_overflow;
    int wave_prio;
};

template <int FORM> struct LinForm {                               // the 16-bit forms: one image, one MFMA per fragment
    using T = typename std::conditional<FORM == PPT_BF16, bf16_t, f16_t>::type;
    static constexpr bool SPLIT = false;
    static constexpr int PARTS = 1;                                // KiB of W fragment per (16 columns x 32 k)
    static constexpr int D1 = 8;                                   // ring depth in k-steps (the split form's bytes in flight)
};
template <> struct LinForm<PPT_F32> {
    using T = f16_t;
    static constexpr bool SPLIT = true;
    static constexpr int PARTS = 2;
    static constexpr int D1 = 4;
};

// NH = column halves of 16 a wave owns: 2 (SLN = 256) or 1 (SLN = 128)
template <int NH, int FORM>
__global__ __launch_bounds__(512, 2) void text_lin_kernel(const LinArgs p)
{
    using F = LinForm<FORM>;
    using T = typename F::T;
    constexpr int SLN = 128 * NH, NP = F::PARTS * NH, D1 = F::D1;
    constexpr int WAVE_SLICE = K1 * NP * 1024;                     // bytes of one wave's fragments per (slice, K chunk)
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char *ai = smem;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, kg = lane >> 4, lo16 = lane * 16;
    PPT_PRIO(p.wave_prio);
    const int nsl = p.N / SLN, nck = p.K / KC;
    const int sc = blockIdx.x % (nsl * nck), s = sc % nsl, c = sc / nsl;          // ids that agree modulo (slices x chunks) share a weight slice
    const int row0 = (blockIdx.x / (nsl * nck)) * R;
    const int nrow = min(R, p.M - row0);
    uint32_t over = 0;

    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.W), 0, (int)((size_t)p.N * p.K * 2 * F::PARTS), 0x00020000);
    int o1 = ((c * nsl + s) * 8 + w) * WAVE_SLICE;
    auto next1 = [&](uint4 (&f)[NP]) {
#pragma unroll
        for (int i = 0; i < NP; ++i) f[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r1, lo16 + 1024 * i, o1, 0));
        o1 += 1024 * NP;
    };
    // 16-bit forms: the block's rows of A (this K chunk) are requested BEFORE the weight ring, so that waiting for them does not
    // wait for the ring as well (loads return in order); rows past M: zeros
    constexpr int PIECES16 = R * (KC / 8);
    uint4 v16[F::SPLIT ? 1 : PIECES16 / 512];
    if constexpr (!F::SPLIT) {
        const uint16_t *A = (const uint16_t *)p.A + (size_t)c * KC;
#pragma unroll
        for (int it = 0; it < PIECES16 / 512; ++it) {
            const int i = threadIdx.x + 512 * it, lr = i / (KC / 8), c8 = i % (KC / 8);
            v16[it] = make_uint4(0, 0, 0, 0);
            if (lr < nrow) v16[it] = *reinterpret_cast<const uint4 *>(A + (size_t)(row0 + lr) * p.lda + 8 * c8);
        }
    }
    uint4 g1[D1][NP];
#pragma unroll
    for (int i = 0; i < D1; ++i) next1(g1[i]);

    if constexpr (F::SPLIT) {
        // ---- the block's rows of A (fp32, this K chunk) -> scaled, saturated, split -> the hi and lo images (rows past M: zeros)
        const float sa = pow2f(p.split_a_pow2);
        const float *A = (const float *)p.A + (size_t)c * KC;
        constexpr int PIECES = R * (KC / 4);
        float4 v[PIECES / 512];
#pragma unroll
        for (int it = 0; it < PIECES / 512; ++it) {
            const int i = threadIdx.x + 512 * it, lr = i / (KC / 4), c4 = i % (KC / 4);
            v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (lr < nrow) v[it] = *reinterpret_cast<const float4 *>(A + (size_t)(row0 + lr) * p.lda + 4 * c4);
        }
#pragma unroll
        for (int it = 0; it < PIECES / 512; ++it) {
            const int i = threadIdx.x + 512 * it, lr = i / (KC / 4), c4 = i % (KC / 4);
            const float x[4] = {split_saturate(v[it].x * sa, over), split_saturate(v[it].y * sa, over),
                                split_saturate(v[it].z * sa, over), split_saturate(v[it].w * sa, over)};
            uint2 H, L;
            split4(x, H, L);
            *reinterpret_cast<uint2 *>(ai + lr * AP + 8 * c4) = H;
            *reinterpret_cast<uint2 *>(ai + A_BYTES + lr * AP + 8 * c4) = L;
        }
    } else {
        // ---- ... and copied into the one image as they are
#pragma unroll
        for (int it = 0; it < PIECES16 / 512; ++it) {
            const int i = threadIdx.x + 512 * it, lr = i / (KC / 8), c8 = i % (KC / 8);
            *reinterpret_cast<uint4 *>(ai + lr * AP + 16 * c8) = v16[it];
        }
    }
    // bias and residual of this lane's output columns: requested now
    const int ncol = SLN * s + 16 * NH * w + 4 * kg;                 // + 16 h
    float4 bv[NH], rv[RB][NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        bv[h] = p.bias ? *reinterpret_cast<const float4 *>(p.bias + ncol + 16 * h) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const int m = row0 + min(16 * rb + l15, nrow - 1);
            rv[rb][h] = p.residual ? *reinterpret_cast<const float4 *>(p.residual + (size_t)m * p.ld_res + ncol + 16 * h) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    lds_barrier();

    ppt_f32x4 a1[RB][NH];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int h = 0; h < NH; ++h) a1[rb][h] = ppt_f32x4{0.f, 0.f, 0.f, 0.f};
    {
        const unsigned char *ha = ai + l15 * AP + 16 * kg;
        uint4 fh[2][RB], fl[2][RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            fh[0][rb] = *reinterpret_cast<const uint4 *>(ha + rb * 16 * AP);
            if constexpr (F::SPLIT) fl[0][rb] = *reinterpret_cast<const uint4 *>(ha + A_BYTES + rb * 16 * AP);
        }
#pragma unroll
        for (int ks = 0; ks < K1; ++ks) {
            if (ks + 1 < K1) {
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    fh[(ks + 1) & 1][rb] = *reinterpret_cast<const uint4 *>(ha + rb * 16 * AP + 64 * (ks + 1));
                    if constexpr (F::SPLIT) fl[(ks + 1) & 1][rb] = *reinterpret_cast<const uint4 *>(ha + A_BYTES + rb * 16 * AP + 64 * (ks + 1));
                }
            }
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                if constexpr (F::SPLIT) {
                    const uint4 wh = g1[ks % D1][2 * h], wl = g1[ks % D1][2 * h + 1];
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) {
                        a1[rb][h] = h16<f16_t>::mfma16(wh, fl[ks & 1][rb], a1[rb][h]);
                        a1[rb][h] = h16<f16_t>::mfma16(wl, fh[ks & 1][rb], a1[rb][h]);
                        a1[rb][h] = h16<f16_t>::mfma16(wh, fh[ks & 1][rb], a1[rb][h]);
                    }
                } else {
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) a1[rb][h] = h16<T>::mfma16(g1[ks % D1][h], fh[ks & 1][rb], a1[rb][h]);
                }
            }
            if (ks + D1 < K1) next1(g1[ks % D1]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // ---- epilogue: a lane holds four consecutive output columns of a row
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int lr = 16 * rb + l15;
        if (lr < nrow) {
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                if constexpr (F::SPLIT) {
                    const float inv = pow2f(-(p.split_a_pow2 + p.split_b_pow2));
                    float *C = (float *)p.C + (size_t)c * p.M * p.ldc;              // (K chunks > 1: parts[c][M][N], ldc == N)
                    *reinterpret_cast<float4 *>(C + (size_t)(row0 + lr) * p.ldc + ncol + 16 * h) =
                        make_float4(a1[rb][h][0] * inv + bv[h].x + rv[rb][h].x, a1[rb][h][1] * inv + bv[h].y + rv[rb][h].y,
                                    a1[rb][h][2] * inv + bv[h].z + rv[rb][h].z, a1[rb][h][3] * inv + bv[h].w + rv[rb][h].w);
                } else {
                    // ((acc + bias) + residual): ppt_gemm's epilogue order
                    const float4 v = make_float4(a1[rb][h][0] + bv[h].x + rv[rb][h].x, a1[rb][h][1] + bv[h].y + rv[rb][h].y,
                                                 a1[rb][h][2] + bv[h].z + rv[rb][h].z, a1[rb][h][3] + bv[h].w + rv[rb][h].w);
                    const size_t off = (size_t)c * p.M * p.ldc + (size_t)(row0 + lr) * p.ldc + ncol + 16 * h;
                    if (p.c16) *reinterpret_cast<uint2 *>((uint16_t *)p.C + off) = make_uint2(h16<T>::pack2(v.x, v.y), h16<T>::pack2(v.z, v.w));
                    else *reinterpret_cast<float4 *>((float *)p.C + off) = v;
                }
            }
        }
    }
    if constexpr (F::SPLIT) split_report(over, p.split_overflow);
}

// fragment order: Wt[c][s][w][ks < 16][h < NH][hi, lo][lane][8] <- W[SLN s + 16 NH w + 16 h + l15][512 c + 32 ks + 8 kg ..) * 2^b_pow2      W [N, K] f32
template <int NH>
__global__ __launch_bounds__(256) void text_lin_retile_split_kernel(const float *__restrict__ W, unsigned char *__restrict__ Wt, int N, int K, int b_pow2)
{
    constexpr int SLN = 128 * NH;
    const int nsl = N / SLN, nck = K / KC;
    const int i = blockIdx.x * 256 + threadIdx.x;                        // over nck * nsl * 8 * 16 * NH * 64 pieces
    if (i >= nck * nsl * 8 * K1 * NH * 64) return;
    const int lane = i & 63, f = (i >> 6) % (K1 * NH), w = (i / (64 * K1 * NH)) & 7, sc = i / (64 * K1 * NH * 8);
    const int s = sc % nsl, c = sc / nsl, ks = f / NH, h = f % NH;
    const int l15 = lane & 15, kg = lane >> 4;
    const float sb = pow2f(b_pow2);
    const float *src = W + (size_t)(SLN * s + 16 * NH * w + 16 * h + l15) * K + KC * c + 32 * ks + 8 * kg;
    uint32_t over = 0;       // (weights are fitted into half's range by the caller: saturated, not counted)
    const float4 a = *reinterpret_cast<const float4 *>(src), b = *reinterpret_cast<const float4 *>(src + 4);
    const float x0[4] = {split_saturate(a.x * sb, over), split_saturate(a.y * sb, over), split_saturate(a.z * sb, over), split_saturate(a.w * sb, over)};
    const float x1[4] = {split_saturate(b.x * sb, over), split_saturate(b.y * sb, over), split_saturate(b.z * sb, over), split_saturate(b.w * sb, over)};
    uint2 h0, l0, h1, l1;
    split4(x0, h0, l0);
    split4(x1, h1, l1);
    unsigned char *dst = Wt + (size_t)(sc * 8 + w) * (K1 * NH * 2048) + (size_t)f * 2048 + lane * 16;
    *reinterpret_cast<uint4 *>(dst) = make_uint4(h0.x, h0.y, h1.x, h1.y);
    *reinterpret_cast<uint4 *>(dst + 1024) = make_uint4(l0.x, l0.y, l1.x, l1.y);
}

// the 16-bit forms' order: Wt[c][s][w][ks < 16][h < NH][lane][8] <- W[SLN s + 16 NH w + 16 h + l15][512 c + 32 ks + 8 kg ..)   W [N, K] 16-bit
template <int NH>
__global__ __launch_bounds__(256) void text_lin_retile16_kernel(const uint16_t *__restrict__ W, unsigned char *__restrict__ Wt, int N, int K)
{
    constexpr int SLN = 128 * NH;
    const int nsl = N / SLN, nck = K / KC;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nck * nsl * 8 * K1 * NH * 64) return;
    const int lane = i & 63, f = (i >> 6) % (K1 * NH), w = (i / (64 * K1 * NH)) & 7, sc = i / (64 * K1 * NH * 8);
    const int s = sc % nsl, c = sc / nsl, ks = f / NH, h = f % NH;
    const int l15 = lane & 15, kg = lane >> 4;
    const uint16_t *src = W + (size_t)(SLN * s + 16 * NH * w + 16 * h + l15) * K + KC * c + 32 * ks + 8 * kg;
    *reinterpret_cast<uint4 *>(Wt + (size_t)i * 16) = *reinterpret_cast<const uint4 *>(src);
}

__host__ int slice_halves(int N) { return N >= 1024 ? 2 : 1; }

template <int NH, int FORM>
void launch(const LinArgs &p, hipStream_t st)
{
    constexpr int LDS_BYTES = LinForm<FORM>::PARTS * A_BYTES;
    PPT_RAISE_LDS_ONCE(LDS_BYTES, (const void *)text_lin_kernel<NH, FORM>);
    const int grid = (p.N / (128 * NH)) * (p.K / KC) * ((p.M + R - 1) / R);
    hipLaunchKernelGGL((text_lin_kernel<NH, FORM>), dim3(grid), dim3(512), LDS_BYTES, st, p);
}

template <int FORM>
void launch_form(const LinArgs &p, hipStream_t st)
{
    if (slice_halves(p.N) == 2) launch<2, FORM>(p, st);
    else launch<1, FORM>(p, st);
}

}  // namespace

extern "C" int ppt_text_lin_retile_split(const float *W, void *Wt, int N, int K, int b_pow2, void *stream)
{
    if (!W || !Wt || (((uintptr_t)W | (uintptr_t)Wt) & 15) || abs(b_pow2) > 24) return PPT_EINVAL;
    if (N <= 0 || K <= 0 || K % KC || N % 256) return PPT_EUNSUPPORTED;
    const int pieces = N * (K / 8);
    if (slice_halves(N) == 2)
        hipLaunchKernelGGL(text_lin_retile_split_kernel<2>, dim3((pieces + 255) / 256), dim3(256), 0, ppt_stream(stream), W, (unsigned char *)Wt, N, K, b_pow2);
    else
        hipLaunchKernelGGL(text_lin_retile_split_kernel<1>, dim3((pieces + 255) / 256), dim3(256), 0, ppt_stream(stream), W, (unsigned char *)Wt, N, K, b_pow2);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" int ppt_text_lin_split(const ppt_text_lin_params *pp, void *stream)
{
    if (!pp) return PPT_EINVAL;
    const ppt_text_lin_params &q = *pp;
    if (!q.A || !q.W || !q.C || q.M <= 0 || q.N <= 0 || q.K <= 0) return PPT_EINVAL;
    if (q.K % KC || q.N % 256) return PPT_EUNSUPPORTED;
    if (q.lda < q.K || (q.lda % 4) || q.ldc < q.N || (q.ldc % 4) || abs(q.split_a_pow2) > 24 || abs(q.split_b_pow2) > 24) return PPT_EINVAL;
    if (((uintptr_t)q.A | (uintptr_t)q.W | (uintptr_t)q.C | (uintptr_t)q.bias | (uintptr_t)q.residual) & 15) return PPT_EINVAL;
    if (q.residual && (q.ld_res < q.N || (q.ld_res % 4))) return PPT_EINVAL;
    if (q.K > KC && (q.bias || q.residual || q.ldc != q.N)) return PPT_EINVAL;          // K chunks leave as plain partial products
    const LinArgs p = {q.A, q.lda, q.W, q.bias, q.residual, q.ld_res, q.C, q.ldc, q.M, q.N, q.K, 0,
                       q.split_a_pow2, q.split_b_pow2, q.split_overflow, q.wave_prio ? q.wave_prio : ppt_get_wave_priority()};
    launch_form<PPT_F32>(p, ppt_stream(stream));
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" int ppt_text_lin_retile16(const void *W, void *Wt, int N, int K, void *stream)
{
    if (!W || !Wt || (((uintptr_t)W | (uintptr_t)Wt) & 15)) return PPT_EINVAL;
    if (N <= 0 || K <= 0 || K % KC || N % 256) return PPT_EUNSUPPORTED;
    const int pieces = N * (K / 8);
    if (slice_halves(N) == 2)
        hipLaunchKernelGGL(text_lin_retile16_kernel<2>, dim3((pieces + 255) / 256), dim3(256), 0, ppt_stream(stream), (const uint16_t *)W, (unsigned char *)Wt, N, K);
    else
        hipLaunchKernelGGL(text_lin_retile16_kernel<1>, dim3((pieces + 255) / 256), dim3(256), 0, ppt_stream(stream), (const uint16_t *)W, (unsigned char *)Wt, N, K);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" int ppt_text_lin16(const ppt_text_lin16_params *pp, void *stream)
{
    if (!pp) return PPT_EINVAL;
    const ppt_text_lin16_params &q = *pp;
    if (!q.A || !q.W || !q.C || q.M <= 0 || q.N <= 0 || q.K <= 0) return PPT_EINVAL;
    if (q.dtype != PPT_F16 && q.dtype != PPT_BF16) return PPT_EINVAL;
    if (q.c_dtype != PPT_F32 && q.c_dtype != q.dtype) return PPT_EINVAL;
    if (q.K % KC || q.N % 256) return PPT_EUNSUPPORTED;
    if (q.lda < q.K || (q.lda % 8) || q.ldc < q.N || (q.ldc % 4)) return PPT_EINVAL;
    if (((uintptr_t)q.A | (uintptr_t)q.W | (uintptr_t)q.bias | (uintptr_t)q.residual) & 15) return PPT_EINVAL;
    if (((uintptr_t)q.C) & (q.c_dtype == PPT_F32 ? 15 : 7)) return PPT_EINVAL;
    if (q.residual && (q.ld_res < q.N || (q.ld_res % 4))) return PPT_EINVAL;
    if (q.K > KC && (q.bias || q.residual || q.ldc != q.N || q.c_dtype != PPT_F32)) return PPT_EINVAL;   // K chunks: fp32 partial products
    const LinArgs p = {q.A, q.lda, q.W, q.bias, q.residual, q.ld_res, q.C, q.ldc, q.M, q.N, q.K, q.c_dtype != PPT_F32,
                       0, 0, nullptr, q.wave_prio ? q.wave_prio : ppt_get_wave_priority()};
    if (q.dtype == PPT_F16) launch_form<PPT_F16>(p, ppt_stream(stream));
    else launch_form<PPT_BF16>(p, ppt_stream(stream));
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}
