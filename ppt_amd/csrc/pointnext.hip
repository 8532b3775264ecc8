// pointnext.hip -- the three kernels the PointNeXt-S encoder (models/pointnext/PointNeXt/openpoints) needs beyond the
// PointNet++ set: the strict direct-form ball query of openpoints' compiled extension, the end of a residual set-abstraction
// level, and the `use_height` column of the input pipeline.  Built with -ffp-contract=off: every product and sum below is rounded
// where it is written.
#include "ppt_common.h"

namespace {

// Ball query of openpoints/cpp/pointnet2_batch/src/ball_query_gpu.cu:15-51: first K indices in ascending order with
// d2 = (dx*dx + dy*dy) + dz*dz < r2 (strict, direct form, fp32), the list padded with its first hit; all zeros when nothing hits.
// Staging as in knn_group.hip: workgroup = (cloud, tile of centres), the cloud once into LDS, one wave per centre, 64 candidates
// per step.  A hit writes its index and its centred coordinates at once; the pad comes from the first hit, kept in a register.
template <int W>
__global__ __launch_bounds__(W * 64) void ball_query_lt_kernel(const float *__restrict__ xyz, const float *__restrict__ center, int N,
                                                               int S, float r2, int K, int cpb, int64_t *__restrict__ idx,
                                                               float *__restrict__ gxyz)
{
    extern __shared__ __align__(16) unsigned char smem[];
    float4 *cloud = reinterpret_cast<float4 *>(smem);
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    const float *p = xyz + (size_t)b * N * 3;
    for (int i = threadIdx.x; i < N; i += blockDim.x) cloud[i] = make_float4(p[i * 3 + 0], p[i * 3 + 1], p[i * 3 + 2], 0.f);
    __syncthreads();
    const int c_end = min(S, (int)(blockIdx.x + 1) * cpb);
    for (int c = blockIdx.x * cpb + w; c < c_end; c += W) {
        const float *q = center + ((size_t)b * S + c) * 3;
        const float qx = q[0], qy = q[1], qz = q[2];
        int64_t *o = idx + ((size_t)b * S + c) * K;
        float *g = gxyz ? gxyz + ((size_t)b * S + c) * K * 3 : nullptr;
        int cnt = 0;
        int first = 0;   // the extension's zero-filled index list when nothing is inside the ball
        for (int base = 0; base < N && cnt < K; base += 64) {
            const int i = base + lane;
            bool hit = false;
            float4 pt = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < N) {
                pt = cloud[i];
                const float dx = __fsub_rn(qx, pt.x), dy = __fsub_rn(qy, pt.y), dz = __fsub_rn(qz, pt.z);
                hit = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)) < r2;
            }
            const unsigned long long mask = __ballot(hit);
            if (mask) {
                if (cnt == 0) first = base + (int)__builtin_ctzll(mask);
                if (hit) {
                    const int pos = cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
                    if (pos < K) {
                        o[pos] = (int64_t)i;
                        if (g) { g[pos * 3 + 0] = __fsub_rn(pt.x, qx); g[pos * 3 + 1] = __fsub_rn(pt.y, qy); g[pos * 3 + 2] = __fsub_rn(pt.z, qz); }
                    }
                }
                cnt += __popcll(mask);
            }
        }
        const float4 pf = cloud[first];                  // (first < N always: 0 or a hit)
        for (int j = min(cnt, K) + lane; j < K; j += 64) {
            o[j] = (int64_t)first;
            if (g) { g[j * 3 + 0] = __fsub_rn(pf.x, qx); g[j * 3 + 1] = __fsub_rn(pf.y, qy); g[j * 3 + 2] = __fsub_rn(pf.z, qz); }
        }
    }
}

// out[g, c] = relu((scale[c] * (scale[c] >= 0 ? max : min)[g, c] + shift[c]) + identity[g, c]), max / min folded over `fold`
// pooled rows: max_k of an affine with no activation behind it, the skip branch added, then the activation
// (SetAbstraction.forward with use_res, backbone/pointnext.py:166-168).  identity may be NULL (nothing added).
template <typename TO>
__global__ __launch_bounds__(256) void pool_res_finish_kernel(const float *__restrict__ pmax, const float *__restrict__ pmin, int G, int fold,
                                                              int C, const float *__restrict__ scale, const float *__restrict__ shift,
                                                              const float *__restrict__ identity, TO *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)G * C) return;
    const int64_t g = i / C;
    const int c = (int)(i % C);
    float mx = -INFINITY, mn = INFINITY;
    for (int f = 0; f < fold; ++f) {
        mx = fmaxf(mx, pmax[(size_t)(g * fold + f) * C + c]);
        mn = fminf(mn, pmin[(size_t)(g * fold + f) * C + c]);
    }
    const float sc = scale[c];
    float v = __fadd_rn(__fmul_rn(sc, sc >= 0.f ? mx : mn), shift[c]);
    if (identity) v = __fadd_rn(v, identity[i]);
    dt<TO>::store(out + i, fmaxf(v, 0.f));
}

// data/dataset_3d.py:311-314 (use_height): out[b, n] = (x, y, z, y - min_n y).  One workgroup per cloud: the minimum through LDS
// (a minimum is the same in every order), then the rows.
__global__ __launch_bounds__(256) void cloud_height_kernel(const float *__restrict__ pc, int N, float *__restrict__ out)
{
    __shared__ float red[256];
    const float *p = pc + (size_t)blockIdx.x * N * 3;
    float *o = out + (size_t)blockIdx.x * N * 4;
    float m = INFINITY;
    for (int i = threadIdx.x; i < N; i += 256) m = fminf(m, p[i * 3 + 1]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] = fminf(red[threadIdx.x], red[threadIdx.x + off]);
        __syncthreads();
    }
    m = red[0];
    for (int i = threadIdx.x; i < N; i += 256) {
        const float x = p[i * 3 + 0], y = p[i * 3 + 1], z = p[i * 3 + 2];
        *reinterpret_cast<float4 *>(o + (size_t)i * 4) = make_float4(x, y, z, __fsub_rn(y, m));
    }
}

}  // namespace

extern "C" int ppt_ball_query_lt_f32(const float *xyz, const float *center, int B, int N, int S, float radius_sq, int K, int64_t *idx,
                                     float *grouped_xyz, void *stream)
{
    if (!xyz || !center || !idx || B <= 0 || N <= 0 || S <= 0 || K <= 0 || K > 64 || N > 8192 || B > 65535) return PPT_EINVAL;
    constexpr int W = 8;
    const size_t lds = (size_t)N * 16;
    static const hipError_t optin = hipFuncSetAttribute((const void *)ball_query_lt_kernel<W>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                         8192 * 16);
    if (lds > 64 * 1024 && optin != hipSuccess) return PPT_ELAUNCH;
    const int cpb = 32;
    dim3 grid((S + cpb - 1) / cpb, B);
    hipLaunchKernelGGL((ball_query_lt_kernel<W>), grid, dim3(W * 64), lds, ppt_stream(stream), xyz, center, N, S, radius_sq, K, cpb, idx,
                       grouped_xyz);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" int ppt_pool_res_finish(const float *pmax, const float *pmin, int G, int fold, int C, const float *scale, const float *shift,
                                   const float *identity, void *out, int out_dtype, void *stream)
{
    if (!pmax || !pmin || !scale || !shift || !out || G <= 0 || fold <= 0 || C <= 0) return PPT_EINVAL;
    const int64_t n = (int64_t)G * C;
    dim3 grid((unsigned)((n + 255) / 256));
    if (!ppt_launch3(out_dtype, [&](auto t) {
            using TO = decltype(t);
            hipLaunchKernelGGL(pool_res_finish_kernel<TO>, grid, dim3(256), 0, ppt_stream(stream), pmax, pmin, G, fold, C, scale, shift,
                               identity, (TO *)out);
        }))
        return PPT_EINVAL;
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" int ppt_cloud_height_f32(const float *pc, int B, int N, float *out, void *stream)
{
    if (!pc || !out || B <= 0 || N <= 0 || ((uintptr_t)out & 15)) return PPT_EINVAL;
    hipLaunchKernelGGL(cloud_height_kernel, dim3(B), dim3(256), 0, ppt_stream(stream), pc, N, out);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}
