// zeroshot.hip -- the small kernels around the ragged text tower (attention_ragged.hip) for zero-shot classification:
//
//   * sentence_rows: x0[off[s] + p] = token_embedding[ids[s, p]] + positional_embedding[p] for p < off[s + 1] - off[s]
//     (ULIP_models.py:102 token_embedding(tokenized) + :209 the positional add), all sentences in one launch, rows behind
//     off[S] (the padding of the row kernels) zero.  One fp32 add per element: bit-equal to the torch expression.
//   * template_ensemble: W[c] = normalize(mean_t normalize(feat[t])) over class c's sentences t in [goff[c], goff[c + 1])
//     -- ULIP's zero-shot rule (normalise each template's feature, average, normalise) -- one workgroup per class, sentences
//     taken in ascending order, every reduction a fixed tree: the same bits on every call.
//   * cosine_head: logits[b, c] = exp(logit_scale) * <f_b / |f_b|, W[c]> -- the CLIP / ULIP rule.  PPT's own forward
//     (ULIP_models.py:279-281) does NOT normalise the point feature; this head does.
// All fp32.
#include "ppt_common.h"

namespace {

// sum over the 256 threads of a workgroup, the same value (and bits) in every thread: wave sums by DPP, the four folded in wave order
__device__ __forceinline__ float block256_sum(float v, float *scr)
{
    const float ws = wave_reduce_sum(v);
    __syncthreads();                                           // scr may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) scr[threadIdx.x >> 6] = ws;
    __syncthreads();
    return ((scr[0] + scr[1]) + scr[2]) + scr[3];
}

__global__ __launch_bounds__(256) void sentence_rows_kernel(const float *__restrict__ table, int vocab, const float *__restrict__ pos,
                                                            const int *__restrict__ ids, int ctx, const int *__restrict__ offsets, int S,
                                                            int W4, float4 *__restrict__ out, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int row = (int)(i / W4), c4 = (int)(i % W4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < offsets[S]) {
        int lo = 0, hi = S - 1;                                // the sentence with off[s] <= row < off[s + 1]
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (offsets[mid] <= row) lo = mid; else hi = mid - 1;
        }
        const int p = row - offsets[lo];
        const int id = p < ctx ? ids[(int64_t)lo * ctx + p] : -1;
        if (id >= 0 && id < vocab) {
            const float4 a = reinterpret_cast<const float4 *>(table)[(int64_t)id * W4 + c4];
            const float4 b = reinterpret_cast<const float4 *>(pos)[(int64_t)p * W4 + c4];
            v = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
        }
    }
    out[i] = v;
}

constexpr int ENS_MAXE = 2048;                                 // columns a thread keeps: ENS_MAXE / 256

__global__ __launch_bounds__(256) void template_ensemble_kernel(const float *__restrict__ feat, const int *__restrict__ goff, int S, int E,
                                                                float *__restrict__ Wout)
{
    __shared__ float scr[4];
    const int c = blockIdx.x;
    const int t0 = max(goff[c], 0), t1 = min(goff[c + 1], S);           // (a malformed range reads nothing outside feat)
    if (t1 <= t0) {                                                       // an empty class: a zero row, not 0 / 0 (workgroup-uniform)
        for (int col = threadIdx.x; col < E; col += 256) Wout[(int64_t)c * E + col] = 0.f;
        return;
    }
    float acc[ENS_MAXE / 256];
#pragma unroll
    for (int k = 0; k < ENS_MAXE / 256; ++k) acc[k] = 0.f;
    for (int t = t0; t < t1; ++t) {
        const float *f = feat + (int64_t)t * E;
        float x[ENS_MAXE / 256], ss = 0.f;
#pragma unroll
        for (int k = 0; k < ENS_MAXE / 256; ++k) {
            const int col = threadIdx.x + 256 * k;
            x[k] = col < E ? f[col] : 0.f;
            ss = fmaf(x[k], x[k], ss);
        }
        const float inv = 1.0f / sqrtf(block256_sum(ss, scr));
#pragma unroll
        for (int k = 0; k < ENS_MAXE / 256; ++k) acc[k] = fmaf(x[k], inv, acc[k]);
    }
    const float invn = 1.0f / (float)(t1 - t0);
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < ENS_MAXE / 256; ++k) {
        acc[k] *= invn;
        ss = fmaf(acc[k], acc[k], ss);
    }
    const float inv = 1.0f / sqrtf(block256_sum(ss, scr));
#pragma unroll
    for (int k = 0; k < ENS_MAXE / 256; ++k) {
        const int col = threadIdx.x + 256 * k;
        if (col < E) Wout[(int64_t)c * E + col] = acc[k] * inv;
    }
}

constexpr int COS_MAXE = 4096;

// one workgroup per point feature: the row and its norm once, then wave w takes classes w, w + 4, ...
__global__ __launch_bounds__(256) void cosine_head_kernel(const float *__restrict__ f, const float *__restrict__ Wt, const float *__restrict__ logit_scale,
                                                          int C, int E, float *__restrict__ logits)
{
    __shared__ float row[COS_MAXE];
    __shared__ float scr[4];
    const int b = blockIdx.x;
    float ss = 0.f;
    for (int col = threadIdx.x; col < E; col += 256) {
        const float v = f[(int64_t)b * E + col];
        row[col] = v;
        ss = fmaf(v, v, ss);
    }
    const float k = expf(logit_scale[0]) / sqrtf(block256_sum(ss, scr));      // (the barriers inside publish `row` too)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = w; c < C; c += 4) {
        const float *wc = Wt + (int64_t)c * E;
        float dot = 0.f;
        for (int col = lane; col < E; col += 64) dot = fmaf(row[col], wc[col], dot);
        dot = wave_reduce_sum(dot);
        if (lane == 0) logits[(int64_t)b * C + c] = k * dot;
    }
}

}  // namespace

extern "C" int ppt_sentence_rows(const float *table, int vocab, const float *pos, const int *ids, int ctx, const int *offsets, int S, int W,
                                 float *out, int rows, void *stream)
{
    if (!table || !pos || !ids || !offsets || !out || vocab <= 0 || ctx <= 0 || S <= 0 || W <= 0 || (W & 3) || rows <= 0) return PPT_EINVAL;
    if (((uintptr_t)table & 15) || ((uintptr_t)pos & 15) || ((uintptr_t)out & 15)) return PPT_EINVAL;
    const int64_t total = (int64_t)rows * (W / 4);
    hipLaunchKernelGGL(sentence_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ppt_stream(stream), table, vocab, pos, ids,
                       ctx, offsets, S, W / 4, reinterpret_cast<float4 *>(out), total);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" int ppt_template_ensemble(const float *feat, const int *group_offsets, int S, int C, int E, float *W, void *stream)
{
    if (!feat || !group_offsets || !W || S <= 0 || C <= 0 || E <= 0) return PPT_EINVAL;
    if (E > ENS_MAXE) return PPT_EUNSUPPORTED;
    hipLaunchKernelGGL(template_ensemble_kernel, dim3(C), dim3(256), 0, ppt_stream(stream), feat, group_offsets, S, E, W);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" int ppt_cosine_head(const float *f, const float *W, const float *logit_scale, int B, int C, int E, float *logits, void *stream)
{
    if (!f || !W || !logit_scale || !logits || B <= 0 || C <= 0 || E <= 0) return PPT_EINVAL;
    if (E > COS_MAXE) return PPT_EUNSUPPORTED;
    hipLaunchKernelGGL(cosine_head_kernel, dim3(B), dim3(256), 0, ppt_stream(stream), f, W, logit_scale, C, E, logits);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}
