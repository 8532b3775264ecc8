// norm.hip -- LayerNorm forward / backward (point_encoder.py:65,69,152; ULIP_models.py:21-27).
// One wave per token row (D <= 1024): the row lives in registers, mean and variance are the
// two-pass forms the reference computes, reductions are wave-wide shuffles -- no LDS, no barrier.
// The forward optionally fuses the `x + pos` of TransformerEncoder.forward (point_encoder.py:103)
// and of encode_text (ULIP_models.py:210), writing the updated residual stream back.
#include "ppt_common.h"

namespace {

constexpr int MAX_EPL = 16;   // elements per lane -> D <= 1024

// ---- the 8-columns-per-lane row (D % 8 == 0, D <= 512): a lane's eight consecutive fp32 values travel as two float4 (v0, v1) ------
// Macros, because the two backward kernels keep their register allocation with nothing else: a function for any one of these
// (float4 pair by reference, a two-float4 struct by value or by reference) changed ln_bwd_dx8_kernel and ln_bwd_w8_kernel; the
// forward kernels took the struct-by-value form unchanged, but one vocabulary for the three kernels is worth more.  LOAD8 and
// STORE8 name p twice and ADD8 binds it once, again because that is what leaves every kernel as it was (a bound pointer in LOAD8
// or STORE8 changed the backward kernels, p twice in ADD8 the forward ones): pass them a pointer that is cheap to spell twice.
#define LOAD8(p, v0, v1)                                                                                    \
    do {                                                                                                     \
        v0 = *reinterpret_cast<const float4 *>(p); v1 = *reinterpret_cast<const float4 *>((p) + 4);          \
    } while (0)
#define ADD8(p, v0, v1)                                                                                      \
    do {                                                                                                     \
        const float *p__ = (p);                                                                              \
        const float4 a0__ = *reinterpret_cast<const float4 *>(p__), a1__ = *reinterpret_cast<const float4 *>(p__ + 4);                    \
        v0.x += a0__.x; v0.y += a0__.y; v0.z += a0__.z; v0.w += a0__.w; v1.x += a1__.x; v1.y += a1__.y; v1.z += a1__.z; v1.w += a1__.w;   \
    } while (0)
#define UNPACK8(v0, v1) {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w}          // the initialiser of a float[8]
#define STORE8(p, v)                                                                                         \
    do {                                                                                                     \
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);                                \
        *reinterpret_cast<float4 *>((p) + 4) = make_float4(v[4], v[5], v[6], v[7]);                          \
    } while (0)

template <typename TY>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float *__restrict__ x, const float *__restrict__ add,
                                                     int add_rows, float *__restrict__ xs,
                                                     const float *__restrict__ w, const float *__restrict__ b,
                                                     TY *__restrict__ y, float *__restrict__ mean_out,
                                                     float *__restrict__ rstd_out, int M, int D, float eps)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float *xr = x + (size_t)row * D;
    const float *ar = add ? add + (size_t)(add_rows > 0 ? row % add_rows : row) * D : nullptr;
    float v[MAX_EPL];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < MAX_EPL; ++j) {
        const int e = lane + 64 * j;
        float t = 0.f;
        if (e < D) { t = xr[e]; if (ar) t += ar[e]; }
        v[j] = t; s += t;
    }
    const float mean = wave_reduce_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < MAX_EPL; ++j) {
        const int e = lane + 64 * j;
        const float d = e < D ? v[j] - mean : 0.f;
        q += d * d;
    }
    const float rstd = 1.0f / sqrtf(wave_reduce_sum(q) / (float)D + eps);
#pragma unroll
    for (int j = 0; j < MAX_EPL; ++j) {
        const int e = lane + 64 * j;
        if (e < D) {
            if (xs) xs[(size_t)row * D + e] = v[j];
            dt<TY>::store(y + (size_t)row * D + e, (v[j] - mean) * rstd * w[e] + b[e]);
        }
    }
    if (lane == 0) {
        if (mean_out) mean_out[row] = mean;
        if (rstd_out) rstd_out[row] = rstd;
    }
}

// D % 8 == 0 and D <= 512 (both towers: 384, 512): lane c owns columns 8c .. 8c+7, so a row is two 16-byte loads
// (+ two for the fused add) and ONE 16-byte bf16 store per lane instead of six 4-byte loads and six 2-byte stores;
// gamma / beta stay in registers while the wave walks its rows (rows strided by the number of waves in the grid).
// Same arithmetic as ln_fwd_kernel (two-pass mean / variance), summed in a different lane order.
// SUM (round 5): the row is x + bias + parts[0] + ... + parts[S-1] (added in that order) -- the consumer side of a split-K GEMM
// whose S partial products were written as plain fp32 slices [S, M, D]: the reduction costs no launch of its own, no atomics, and
// the summation order is fixed (the prompt chain's K = 2048 linears: engine.text_tower_forward).
template <typename TY, bool SUM = false>
__global__ __launch_bounds__(256) void ln_fwd_vec8_kernel(const float *__restrict__ x, const float *__restrict__ add,
                                                          int add_rows, float *__restrict__ xs,
                                                          const float *__restrict__ w, const float *__restrict__ b,
                                                          TY *__restrict__ y, float *__restrict__ mean_out,
                                                          float *__restrict__ rstd_out, int M, int D, float eps, int prio,
                                                          const float *__restrict__ sum_bias = nullptr,
                                                          const float *__restrict__ parts = nullptr, int S = 0)
{
    PPT_PRIO(prio);
    const int lane = threadIdx.x & 63;
    const int nw = gridDim.x * 4;
    const bool on = lane * 8 < D;
    const int c = on ? lane * 8 : 0;
    float4 g0, g1, b0, b1;
    LOAD8(w + c, g0, g1);
    LOAD8(b + c, b0, b1);
    const float g[8] = UNPACK8(g0, g1), be[8] = UNPACK8(b0, b1);
    const float inv_d = 1.0f / (float)D;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < M; row += nw) {
        float4 v0, v1;
        LOAD8(x + (size_t)row * D + c, v0, v1);
        if (add) ADD8(add + (size_t)(add_rows > 0 ? row % add_rows : row) * D + c, v0, v1);
        if constexpr (SUM) {
            if (sum_bias) ADD8(sum_bias + c, v0, v1);
            for (int z = 0; z < S; ++z) ADD8(parts + ((size_t)z * M + row) * D + c, v0, v1);
        }
        const float v[8] = UNPACK8(v0, v1);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
        const float mean = wave_reduce_sum(on ? s : 0.f) * inv_d;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = v[j] - mean; q = fmaf(d, d, q); }
        const float rstd = 1.0f / sqrtf(wave_reduce_sum(on ? q : 0.f) * inv_d + eps);
        if (on) {
            if (xs) STORE8(xs + (size_t)row * D + c, v);
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (v[j] - mean) * rstd * g[j] + be[j];
            if constexpr (sizeof(TY) == 2) {
                *reinterpret_cast<uint4 *>(y + (size_t)row * D + c) =
                    make_uint4(h16<TY>::pack2(o[0], o[1]), h16<TY>::pack2(o[2], o[3]), h16<TY>::pack2(o[4], o[5]), h16<TY>::pack2(o[6], o[7]));
            } else {
                STORE8(y + (size_t)row * D + c, o);
            }
        }
        if (lane == 0) {
            if (mean_out) mean_out[row] = mean;
            if (rstd_out) rstd_out[row] = rstd;
        }
    }
}

// wave g handles rows [g*rpw, (g+1)*rpw); dw/db partial row g.
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ xs,
                                                     const float *__restrict__ w, const float *__restrict__ mean,
                                                     const float *__restrict__ rstd, float *__restrict__ dx,
                                                     int accumulate, void *__restrict__ dx_copy, int copy_dtype,
                                                     float *__restrict__ dw_part,
                                                     float *__restrict__ db_part, int rpw, int M, int D, int prio)
{
    PPT_PRIO(prio);
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int r0 = g * rpw, r1 = min(M, r0 + rpw);
    if (r0 >= M) return;
    float wv[MAX_EPL], dwa[MAX_EPL], dba[MAX_EPL];
#pragma unroll
    for (int j = 0; j < MAX_EPL; ++j) {
        const int e = lane + 64 * j;
        wv[j] = e < D ? w[e] : 0.f;
        dwa[j] = 0.f; dba[j] = 0.f;
    }
    for (int row = r0; row < r1; ++row) {
        const float mu = mean[row], rs = rstd[row];
        float gv[MAX_EPL], xh[MAX_EPL];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < MAX_EPL; ++j) {
            const int e = lane + 64 * j;
            float d = 0.f, xhat = 0.f;
            if (e < D) { d = dy[(size_t)row * D + e]; xhat = (xs[(size_t)row * D + e] - mu) * rs; }
            dwa[j] += d * xhat; dba[j] += d;
            gv[j] = d * wv[j]; xh[j] = xhat;
            s1 += gv[j]; s2 += gv[j] * xhat;
        }
        s1 = wave_reduce_sum(s1) / (float)D;
        s2 = wave_reduce_sum(s2) / (float)D;
#pragma unroll
        for (int j = 0; j < MAX_EPL; ++j) {
            const int e = lane + 64 * j;
            if (e < D) {
                const float r = rs * (gv[j] - s1 - xh[j] * s2);
                float *o = dx + (size_t)row * D + e;
                const float t = accumulate ? *o + r : r;
                *o = t;
                if (dx_copy) {
                    if (copy_dtype != PPT_F32) ((uint16_t *)dx_copy)[(size_t)row * D + e] = from_f32_dt(copy_dtype, t);
                    else ((float *)dx_copy)[(size_t)row * D + e] = t;
                }
            }
        }
    }
    if (dw_part) {
#pragma unroll
        for (int j = 0; j < MAX_EPL; ++j) {
            const int e = lane + 64 * j;
            if (e < D) { dw_part[(size_t)g * D + e] = dwa[j]; db_part[(size_t)g * D + e] = dba[j]; }
        }
    }
}

// ---- the two pieces ln_bwd_dx8_kernel and ln_bwd_w8_kernel share, as macros in the kernel's scope for the reason given at LOAD8 ----
// One row's arithmetic.  Reads dv, xv, wv (the lane's eight dy, x, gamma), mu, rs, act, D; declares gv, xh and the row means s1
// (of g = dy * gamma) and s2 (of g * xhat).  PER_COLUMN runs for each j once xh[j] is known: ln_bwd_w8_kernel's dw / db sums.
#define LN_BWD8_ROW(PER_COLUMN)                                                           \
    float gv[8], xh[8], s1 = 0.f, s2 = 0.f;                                               \
    _Pragma("unroll")                                                                     \
    for (int j = 0; j < 8; ++j) {                                                         \
        xh[j] = act ? (xv[j] - mu) * rs : 0.f;                                            \
        PER_COLUMN;                                                                       \
        gv[j] = dv[j] * wv[j];                                                            \
        s1 += gv[j]; s2 += gv[j] * xh[j];                                                 \
    }                                                                                     \
    s1 = wave_reduce_sum(s1) / (float)D;                                                  \
    s2 = wave_reduce_sum(s2) / (float)D
// The lane's eight dx at element offset `off` (added to av, the row of dx loaded before: zeros unless accumulate) and their fp32 or
// 16-bit operand copy: one 16-byte store per lane for the latter.  Reads av, rs, gv, xh, s1, s2, dx, dx_copy, copy_dtype.
#define LN_BWD8_STORE_DX(off)                                                                                                     \
    do {                                                                                                                          \
        float t[8];                                                                                                               \
        _Pragma("unroll")                                                                                                         \
        for (int j = 0; j < 8; ++j) t[j] = av[j] + rs * (gv[j] - s1 - xh[j] * s2);                                                \
        STORE8(dx + (off), t);                                                                                                    \
        if (dx_copy) {                                                                                                            \
            if (copy_dtype != PPT_F32) {                                                                                          \
                *reinterpret_cast<uint4 *>((uint16_t *)dx_copy + (off)) = make_uint4(pack2_dt(copy_dtype, t[0], t[1]), pack2_dt(copy_dtype, t[2], t[3]), \
                                                                                   pack2_dt(copy_dtype, t[4], t[5]), pack2_dt(copy_dtype, t[6], t[7])); \
            } else {                                                                                                              \
                STORE8((float *)dx_copy + (off), t);                                                                              \
            }                                                                                                                     \
        }                                                                                                                         \
    } while (0)

// The input-gradient-only backward (no dw / db: the text tower's LayerNorms are frozen) for D % 8 == 0, D <= 512: one wave per
// row, a lane owns EIGHT consecutive columns -- two 16-byte loads per tensor, and the row of dx that the result is added to is
// requested together with dy and xs instead of after the reduction (the scalar kernel's third dependent round trip); the bf16
// operand copy leaves as one 16-byte store per lane.  8.5 -> ~5 us for 817 x 512 (24 launches per step of the prompt chain).
// S > 0 (round 5): dy is the sum of S fp32 slices [S, M, D] (a split-K dX GEMM's partial products), added in slice order.
__global__ __launch_bounds__(256) void ln_bwd_dx8_kernel(const float *__restrict__ dy, const float *__restrict__ xs,
                                                         const float *__restrict__ w, const float *__restrict__ mean,
                                                         const float *__restrict__ rstd, float *__restrict__ dx, int accumulate,
                                                         void *__restrict__ dx_copy, int copy_dtype, int M, int D, int prio, int S = 0)
{
    PPT_PRIO(prio);
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const bool act = lane * 8 < D;
    const size_t off = (size_t)row * D + lane * 8;
    float4 d0 = make_float4(0.f, 0.f, 0.f, 0.f), d1 = d0, x0 = d0, x1 = d0, a0 = d0, a1 = d0, w0 = d0, w1 = d0;
    if (act) {
        LOAD8(dy + off, d0, d1);
        for (int z = 1; z < S; ++z) ADD8(dy + (size_t)z * M * D + off, d0, d1);
        LOAD8(xs + off, x0, x1);
        LOAD8(w + lane * 8, w0, w1);
        if (accumulate) LOAD8(dx + off, a0, a1);
    }
    const float mu = mean[row], rs = rstd[row];
    const float dv[8] = UNPACK8(d0, d1), xv[8] = UNPACK8(x0, x1), wv[8] = UNPACK8(w0, w1), av[8] = UNPACK8(a0, a1);
    LN_BWD8_ROW((void)0);
    if (!act) return;
    LN_BWD8_STORE_DX(off);
}

// The backward WITH weight / bias gradients (trainable LayerNorms: the un-frozen last PointBERT block, point_encoder.py:70-79) in
// the 16-byte form: wave g walks rows [g * rpw, (g + 1) * rpw), a lane owns EIGHT consecutive columns (two float4 per tensor and
// row), the NEXT row's dy / xs / dx are requested before this row's two wave reductions (ln_bwd_kernel: one 4-byte element per
// lane and load, three dependent round trips per row -- 92 us for 32 832 x 384 at C3, 0.55 TB/s), and dw / db accumulate per
// column in the lane's registers in row order -- the partial rows ln_bwd_kernel writes, bit for bit; dx sums its two row
// statistics in ln_bwd_dx8_kernel's order.
__global__ __launch_bounds__(256) void ln_bwd_w8_kernel(const float *__restrict__ dy, const float *__restrict__ xs,
                                                        const float *__restrict__ w, const float *__restrict__ mean,
                                                        const float *__restrict__ rstd, float *__restrict__ dx, int accumulate,
                                                        void *__restrict__ dx_copy, int copy_dtype, float *__restrict__ dw_part,
                                                        float *__restrict__ db_part, int rpw, int M, int D, int prio)
{
    PPT_PRIO(prio);
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int r0 = g * rpw, r1 = min(M, r0 + rpw);
    if (r0 >= M) return;
    const bool act = lane * 8 < D;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 w0 = z4, w1 = z4;
    if (act) LOAD8(w + lane * 8, w0, w1);
    const float wv[8] = UNPACK8(w0, w1);
    float dwa[8], dba[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { dwa[j] = 0.f; dba[j] = 0.f; }
    float4 d0 = z4, d1 = z4, x0 = z4, x1 = z4, a0 = z4, a1 = z4;
    auto fetch = [&](int row, float4 &D0, float4 &D1, float4 &X0, float4 &X1, float4 &A0, float4 &A1) {
        if (act) {
            const size_t off = (size_t)row * D + lane * 8;
            LOAD8(dy + off, D0, D1);
            LOAD8(xs + off, X0, X1);
            if (accumulate) LOAD8(dx + off, A0, A1);
        }
    };
    fetch(r0, d0, d1, x0, x1, a0, a1);
    for (int row = r0; row < r1; ++row) {
        float4 nd0 = z4, nd1 = z4, nx0 = z4, nx1 = z4, na0 = z4, na1 = z4;
        if (row + 1 < r1) fetch(row + 1, nd0, nd1, nx0, nx1, na0, na1);       // in flight during this row's reductions
        const float mu = mean[row], rs = rstd[row];
        const float dv[8] = UNPACK8(d0, d1), xv[8] = UNPACK8(x0, x1), av[8] = UNPACK8(a0, a1);
        LN_BWD8_ROW(dwa[j] += dv[j] * xh[j]; dba[j] += dv[j]);
        if (act) {
            const size_t off = (size_t)row * D + lane * 8;
            LN_BWD8_STORE_DX(off);
        }
        d0 = nd0; d1 = nd1; x0 = nx0; x1 = nx1; a0 = na0; a1 = na1;
    }
    if (act) {
        float *pw = dw_part + (size_t)g * D + lane * 8, *pb = db_part + (size_t)g * D + lane * 8;
        STORE8(pw, dwa);
        STORE8(pb, dba);
    }
}

// The 8-wide kernels apply: D % 8 == 0, D <= 512 and every operand (absent ones are null) on a 16-byte boundary.
bool ln_wide8(int D, std::initializer_list<const void *> operands)
{
    uintptr_t bits = 0;
    for (const void *p : operands) bits |= (uintptr_t)p;
    return D % 8 == 0 && D <= 512 && (bits & 15) == 0;
}

// ln_fwd_vec8_kernel; S > 0: its split-K consumer form.  false: y_dtype is none of the three formats.
bool launch_fwd_vec8(const float *x, const float *add, int add_rows, float *xs, const float *w, const float *b, void *y, int y_dtype,
                     float *mean, float *rstd, int M, int D, float eps, const float *sum_bias, const float *parts, int S, void *stream)
{
    dim3 vgrid(min((M + 3) / 4, 256 * 8));         // 8 workgroups per CU; each wave walks rows with that stride
    return ppt_launch3(y_dtype, [&](auto t) {
        using TY = decltype(t);
        const auto k = S > 0 ? ln_fwd_vec8_kernel<TY, true> : ln_fwd_vec8_kernel<TY, false>;
        hipLaunchKernelGGL(k, vgrid, dim3(256), 0, ppt_stream(stream), x, add, add_rows, xs, w, b, (TY *)y, mean, rstd, M, D, eps,
                           ppt_get_wave_priority(), sum_bias, parts, S);
    });
}

// ln_bwd_dx8_kernel; S > 0: dy is S slices
void launch_bwd_dx8(const float *dy, int S, const float *xs, const float *w, const float *mean, const float *rstd, float *dx,
                    int accumulate_dx, void *dx_copy, int dx_copy_dtype, int M, int D, void *stream)
{
    hipLaunchKernelGGL(ln_bwd_dx8_kernel, dim3((M + 3) / 4), dim3(256), 0, ppt_stream(stream), dy, xs, w, mean, rstd, dx, accumulate_dx,
                       dx_copy, dx_copy_dtype, M, D, ppt_get_wave_priority(), S);
}

}  // namespace

extern "C" int ppt_layernorm_fwd(const float *x, const float *add, int add_rows, float *xs, const float *w,
                                 const float *b, void *y, int y_dtype, float *mean, float *rstd, int M, int D,
                                 float eps, void *stream)
{
    if (!x || !w || !b || !y || M <= 0 || D <= 0 || D > 64 * MAX_EPL) return PPT_EINVAL;
    if (y_dtype != PPT_BF16 && y_dtype != PPT_F32 && y_dtype != PPT_F16) return PPT_EINVAL;
    if (ln_wide8(D, {x, w, b, y, add, xs}))
        (void)launch_fwd_vec8(x, add, add_rows, xs, w, b, y, y_dtype, mean, rstd, M, D, eps, nullptr, nullptr, 0, stream);
    else
        (void)ppt_launch3(y_dtype, [&](auto t) {
            using TY = decltype(t);
            hipLaunchKernelGGL(ln_fwd_kernel<TY>, dim3((M + 3) / 4), dim3(256), 0, ppt_stream(stream), x, add, add_rows, xs, w, b, (TY *)y,
                               mean, rstd, M, D, eps);
        });
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" int ppt_layernorm_bwd(const float *dy, const float *xs, const float *w, const float *mean,
                                 const float *rstd, float *dx, int accumulate_dx, void *dx_copy, int dx_copy_dtype,
                                 float *dw_partial, float *db_partial, int partial_rows, int M, int D, void *stream)
{
    if (!dy || !xs || !w || !mean || !rstd || !dx || M <= 0 || D <= 0 || D > 64 * MAX_EPL) return PPT_EINVAL;
    if ((dw_partial == nullptr) != (db_partial == nullptr)) return PPT_EINVAL;
    if (dw_partial && partial_rows <= 0) return PPT_EINVAL;
    const bool wide8 = ln_wide8(D, {dy, xs, w, dx, dx_copy, dw_partial, db_partial});
    if (!dw_partial && wide8) {
        launch_bwd_dx8(dy, 0, xs, w, mean, rstd, dx, accumulate_dx, dx_copy, dx_copy_dtype, M, D, stream);
        PPT_CHECK_LAUNCH();
        return PPT_OK;
    }
    const int waves = dw_partial ? partial_rows : M;
    const int rpw = (M + waves - 1) / waves;
    // every partial row must be written (rows past the data get zeros from an empty range): the
    // kernel returns early for empty ranges, so clear the tail partial rows here.
    const int used = (M + rpw - 1) / rpw;
    if (dw_partial && used < partial_rows) {
        (void)hipMemsetAsync(dw_partial + (size_t)used * D, 0, sizeof(float) * (size_t)(partial_rows - used) * D, ppt_stream(stream));
        (void)hipMemsetAsync(db_partial + (size_t)used * D, 0, sizeof(float) * (size_t)(partial_rows - used) * D, ppt_stream(stream));
    }
    // the 16-byte form where it applies (it needs dw / db partials); ln_bwd_kernel for every other shape and alignment
    const auto k = dw_partial && wide8 ? ln_bwd_w8_kernel : ln_bwd_kernel;
    hipLaunchKernelGGL(k, dim3((used + 3) / 4), dim3(256), 0, ppt_stream(stream), dy, xs, w, mean, rstd, dx, accumulate_dx, dx_copy,
                       dx_copy_dtype, dw_partial, db_partial, rpw, M, D, ppt_get_wave_priority());
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

// LayerNorm of x + bias + parts[0] + ... + parts[S-1] (split-K consumer, see ln_fwd_vec8_kernel<.., true>); xs (required) receives
// the summed row.  D % 8 == 0, D <= 512, 16-byte aligned operands.
extern "C" int ppt_layernorm_fwd_sum(const float *x, const float *bias, const float *parts, int S, float *xs, const float *w, const float *b,
                                     void *y, int y_dtype, float *mean, float *rstd, int M, int D, float eps, void *stream)
{
    if (!x || !parts || !xs || !w || !b || !y || S <= 0 || S > 8 || M <= 0 || D <= 0) return PPT_EINVAL;
    if ((D % 8) != 0 || D > 512) return PPT_EUNSUPPORTED;
    if (!ln_wide8(D, {x, w, b, y, parts, xs, bias})) return PPT_EINVAL;
    if (!launch_fwd_vec8(x, nullptr, 0, xs, w, b, y, y_dtype, mean, rstd, M, D, eps, bias, parts, S, stream)) return PPT_EINVAL;
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

// ppt_layernorm_bwd's input-gradient form with dy = dy_parts[0] + ... + dy_parts[S-1] ([S, M, D] fp32, summed in that order).
extern "C" int ppt_layernorm_bwd_sum(const float *dy_parts, int S, const float *xs, const float *w, const float *mean, const float *rstd,
                                     float *dx, int accumulate_dx, void *dx_copy, int dx_copy_dtype, int M, int D, void *stream)
{
    if (!dy_parts || !xs || !w || !mean || !rstd || !dx || S <= 0 || S > 8 || M <= 0 || D <= 0) return PPT_EINVAL;
    if ((D % 8) != 0 || D > 512) return PPT_EUNSUPPORTED;
    if (!ln_wide8(D, {dy_parts, xs, w, dx, dx_copy})) return PPT_EINVAL;
    launch_bwd_dx8(dy_parts, S, xs, w, mean, rstd, dx, accumulate_dx, dx_copy, dx_copy_dtype, M, D, stream);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}
