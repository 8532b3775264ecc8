// tsne.hip -- the "Feature Distribution" figure of notebook/visualize.ipynb on the device (ppt_amd/tsne.py): exact t-SNE in two
// dimensions over the logits that save_recog_feats writes.  The statement of every quantity is in include/ppt_hip.h; the file is
// built with -ffp-contract=off, so each `*` and `+` below is one IEEE fp32 (or double) operation.
//
//   tsne_cond_kernel     one workgroup per row i: the N squared distances of the row go to LDS once (x is streamed from L2) and
//                        stay there for the <= 100 evaluations of the perplexity search; the conditional row is written into P.
//   tsne_sym_kernel      one workgroup per pair of mirrored 32 x 32 tiles: P = (C + C^T) / 2N in place (no tile is touched by two
//                        workgroups), plus the tile pair's sums of P and P log P in double.
//   tsne_pstats_kernel   one workgroup folds the tile sums in tile order.
//   tsne_pair_kernel     per iteration: one wave per row i, Y in LDS, P read once with 16 bytes per lane along j; the lane sums
//                        are folded by a shuffle butterfly and the row's attraction, repulsion, sum of w (and, on check
//                        iterations, sum of P log(1 + d^2)) go to the workspace.  Symmetry is not exploited: nothing is scattered.
//   tsne_update_kernel   per iteration: every workgroup re-reduces the N row sums of w to Z in double (the same order, so the
//                        same bits, in every workgroup -- no third launch, no grid-wide synchronisation), then one thread per
//                        point forms the gradient and takes sklearn's step; on check iterations workgroup 0 also writes KL, ||g||.
// No atomics anywhere; all reductions have a fixed shape: two runs write identical bytes.
#include <math.h>
#include "ppt_common.h"

#define TS_THREADS 256
#define TS_WAVES (TS_THREADS / PPT_WAVE)
#define TS_MAX_N 16384
#define TS_MAX_D 4096
#define TS_TILE 32
#define TS_PAIR_SMALL 4096                 // up to this N the pair pass runs 256-thread workgroups (several per CU), 1024 above
#define TS_SEARCH_STEPS 100
#define TS_SEARCH_TOL 1e-5

// sum over the workgroup's 256 threads, the same bits in every thread: butterfly inside the wave, the four wave sums in order
__device__ __forceinline__ double ts_block_sum(double v, double *red)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(TS_THREADS) void tsne_cond_kernel(const float *__restrict__ x, int64_t ld, int N, int D, int vec,
                                                               double log_perplexity, float *__restrict__ P, int64_t ldp,
                                                               float *__restrict__ beta_out)
{
    extern __shared__ float ts_lds[];
    __shared__ double red[TS_WAVES];
    __shared__ float red_min[TS_WAVES];
    float *d = ts_lds;                                     // [N] the row's distances, then e_ij = d_ij - m_i
    float *xi = ts_lds + ((N + 3) & ~3);                   // [D]
    const int i = blockIdx.x, tid = threadIdx.x;
    for (int c = tid; c < D; c += TS_THREADS) xi[c] = x[(size_t)i * ld + c];
    __syncthreads();

    float m = INFINITY;
    for (int j = tid; j < N; j += TS_THREADS) {
        const float *xj = x + (size_t)j * ld;
        float acc = 0.0f;
        int c = 0;
        if (vec) {                                         // 16-byte loads, the columns still in ascending order: the same bits
            for (; c + 3 < D; c += 4) {
                const float4 v = *reinterpret_cast<const float4 *>(xj + c);
                const float t0 = xi[c] - v.x, t1 = xi[c + 1] - v.y, t2 = xi[c + 2] - v.z, t3 = xi[c + 3] - v.w;
                acc += t0 * t0; acc += t1 * t1; acc += t2 * t2; acc += t3 * t3;
            }
        }
        for (; c < D; c++) {
            const float t = xi[c] - xj[c];
            acc += t * t;
        }
        d[j] = acc;
        if (j != i) m = fminf(m, acc);
    }
    for (int o = 32; o; o >>= 1) m = fminf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) red_min[tid >> 6] = m;
    __syncthreads();
    m = fminf(fminf(red_min[0], red_min[1]), fminf(red_min[2], red_min[3]));
    for (int j = tid; j < N; j += TS_THREADS) d[j] -= m;    // (each thread its own entries: no barrier needed)

    float beta = 1.0f, lo = -INFINITY, hi = INFINITY;
    double S = 1.0;
    for (int step = 0; step < TS_SEARCH_STEPS; step++) {
        float s = 0.0f, a = 0.0f;
        for (int j = tid; j < N; j += TS_THREADS) {
            if (j != i) {
                const float e = d[j];
                const float q = expf(-(beta * e));
                s += q;
                a += e * q;
            }
        }
        S = ts_block_sum((double)s, red);
        const double A = ts_block_sum((double)a, red);
        const double diff = (log(S) + (double)beta * A / S) - log_perplexity;
        if (fabs(diff) <= TS_SEARCH_TOL || step == TS_SEARCH_STEPS - 1) break;      // (the same decision in every thread)
        if (diff > 0.0) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.0f : (beta + hi) * 0.5f;
        } else {
            hi = beta;
            beta = lo == -INFINITY ? beta * 0.5f : (beta + lo) * 0.5f;
        }
    }
    const float Sf = (float)S;
    for (int j = tid; j < N; j += TS_THREADS) P[(size_t)i * ldp + j] = j == i ? 0.0f : expf(-(beta * d[j])) / Sf;
    if (tid == 0) beta_out[i] = beta;
}

__global__ __launch_bounds__(TS_THREADS) void tsne_sym_kernel(float *__restrict__ P, int64_t ldp, int N, int T, double *__restrict__ partial)
{
    __shared__ float ta[TS_TILE][TS_TILE + 1], tb[TS_TILE][TS_TILE + 1];
    __shared__ double red[TS_WAVES];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;                                   // the pair (bi, bj), (bj, bi) belongs to the workgroup with bi <= bj
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    for (int r = r0; r < TS_TILE; r += TS_THREADS / TS_TILE) {
        const int ia = bi * TS_TILE + r, ja = bj * TS_TILE + c, ib = bj * TS_TILE + r, jb = bi * TS_TILE + c;
        ta[r][c] = ia < N && ja < N ? P[(size_t)ia * ldp + ja] : 0.0f;
        tb[r][c] = ib < N && jb < N ? P[(size_t)ib * ldp + jb] : 0.0f;
    }
    __syncthreads();
    const float two_n = (float)(2 * N);
    double sp = 0.0, spl = 0.0;
    for (int r = r0; r < TS_TILE; r += TS_THREADS / TS_TILE) {
        const int ia = bi * TS_TILE + r, ja = bj * TS_TILE + c, ib = bj * TS_TILE + r, jb = bi * TS_TILE + c;
        if (ia < N && ja < N) {
            const float v = (ta[r][c] + tb[c][r]) / two_n;
            P[(size_t)ia * ldp + ja] = v;
            sp += (double)v;
            if (v > 0.0f) spl += (double)(v * logf(v));
        }
        if (bi != bj && ib < N && jb < N) {
            const float v = (tb[r][c] + ta[c][r]) / two_n;
            P[(size_t)ib * ldp + jb] = v;
            sp += (double)v;
            if (v > 0.0f) spl += (double)(v * logf(v));
        }
    }
    sp = ts_block_sum(sp, red);
    spl = ts_block_sum(spl, red);
    if (threadIdx.x == 0) {
        partial[2 * ((size_t)bi * T + bj)] = sp;
        partial[2 * ((size_t)bi * T + bj) + 1] = spl;
    }
}

__global__ __launch_bounds__(TS_THREADS) void tsne_pstats_kernel(const double *__restrict__ partial, int T, double *__restrict__ pstats)
{
    __shared__ double red[TS_WAVES];
    double sp = 0.0, spl = 0.0;
    for (int k = threadIdx.x; k < T * T; k += TS_THREADS) {
        if (k / T <= k % T) { sp += partial[2 * (size_t)k]; spl += partial[2 * (size_t)k + 1]; }
    }
    sp = ts_block_sum(sp, red);
    spl = ts_block_sum(spl, red);
    if (threadIdx.x == 0) { pstats[0] = sp; pstats[1] = spl; }
}

// one term of row i: lane sums of (P w)(dx, dy), (w w)(dx, dy), w and P log(1 + d^2)
template <bool CHECK>
__device__ __forceinline__ void ts_pair(float p, float yj0, float yj1, bool valid, float yi0, float yi1, float &ax, float &ay,
                                        float &rx, float &ry, float &z, float &l)
{
    const float dx = yi0 - yj0, dy = yi1 - yj1;
    const float dd = (dx * dx + dy * dy) + 1.0f;
    const float w = valid ? __builtin_amdgcn_rcpf(dd) : 0.0f;
    const float pw = p * w, ww = w * w;
    ax += pw * dx; ay += pw * dy;
    rx += ww * dx; ry += ww * dy;
    z += w;
    if (CHECK) l += p * logf(dd);
}

// workspace rows: ar [N] float4 = (a_i, r_i), z [N], l [N]
template <bool CHECK>
__global__ __launch_bounds__(1024) void tsne_pair_kernel(const float *__restrict__ P, int64_t ldp, int N, const float *__restrict__ y,
                                                         float4 *__restrict__ ar, float *__restrict__ zrow, float *__restrict__ lrow)
{
    extern __shared__ float ts_lds[];
    float2 *Y = reinterpret_cast<float2 *>(ts_lds);        // [(N + 3) & ~3], the padding zero
    const int npad = (N + 3) & ~3;
    for (int j = threadIdx.x; j < npad; j += blockDim.x)
        Y[j] = j < N ? reinterpret_cast<const float2 *>(y)[j] : make_float2(0.0f, 0.0f);
    __syncthreads();
    const int lane = threadIdx.x & 63, waves = blockDim.x >> 6;
    for (int i = blockIdx.x * waves + (threadIdx.x >> 6); i < N; i += gridDim.x * waves) {
        const float *row = P + (size_t)i * ldp;
        const float2 yi = Y[i];
        float ax = 0.0f, ay = 0.0f, rx = 0.0f, ry = 0.0f, z = 0.0f, l = 0.0f;
        for (int j0 = 4 * lane; j0 < N; j0 += 4 * PPT_WAVE) {
            float4 p;
            if (j0 + 3 < N) {
                p = *reinterpret_cast<const float4 *>(row + j0);
            } else {                                       // the row's last, partial group: the padding of P is never read
                p.x = row[j0];
                p.y = j0 + 1 < N ? row[j0 + 1] : 0.0f;
                p.z = j0 + 2 < N ? row[j0 + 2] : 0.0f;
                p.w = 0.0f;
            }
            const float4 y01 = *reinterpret_cast<const float4 *>(&Y[j0]), y23 = *reinterpret_cast<const float4 *>(&Y[j0 + 2]);
            ts_pair<CHECK>(p.x, y01.x, y01.y, j0 != i, yi.x, yi.y, ax, ay, rx, ry, z, l);
            ts_pair<CHECK>(p.y, y01.z, y01.w, j0 + 1 != i && j0 + 1 < N, yi.x, yi.y, ax, ay, rx, ry, z, l);
            ts_pair<CHECK>(p.z, y23.x, y23.y, j0 + 2 != i && j0 + 2 < N, yi.x, yi.y, ax, ay, rx, ry, z, l);
            ts_pair<CHECK>(p.w, y23.z, y23.w, j0 + 3 != i && j0 + 3 < N, yi.x, yi.y, ax, ay, rx, ry, z, l);
        }
        for (int o = 32; o; o >>= 1) {
            ax += __shfl_xor(ax, o); ay += __shfl_xor(ay, o);
            rx += __shfl_xor(rx, o); ry += __shfl_xor(ry, o);
            z += __shfl_xor(z, o);
            if (CHECK) l += __shfl_xor(l, o);
        }
        if (lane == 0) {
            ar[i] = make_float4(ax, ay, rx, ry);
            zrow[i] = z;
            if (CHECK) lrow[i] = l;
        }
    }
}

__device__ __forceinline__ float ts_grad(float alpha, float a, float r, float inv_z) { return 4.0f * (alpha * a - r * inv_z); }

__device__ __forceinline__ void ts_step(float g, float mu, float lr, float &gain, float &upd, float &yv)
{
    const bool inc = upd * g < 0.0f;
    gain = inc ? gain + 0.2f : gain * 0.8f;
    gain = fmaxf(gain, 0.01f);
    upd = mu * upd - lr * (g * gain);
    yv += upd;
}

template <bool CHECK>
__global__ __launch_bounds__(TS_THREADS) void tsne_update_kernel(const float4 *__restrict__ ar, const float *__restrict__ zrow,
                                                                 const float *__restrict__ lrow, const double *__restrict__ pstats, int N,
                                                                 float alpha, float mu, float lr, float *__restrict__ y,
                                                                 float *__restrict__ update, float *__restrict__ gains,
                                                                 float *__restrict__ grad, float *__restrict__ stats)
{
    __shared__ double red[TS_WAVES];
    double zs = 0.0;
    for (int j = threadIdx.x; j < N; j += TS_THREADS) zs += (double)zrow[j];
    const double Z = ts_block_sum(zs, red);
    const float inv_z = (float)(1.0 / Z);
    const int i = blockIdx.x * TS_THREADS + threadIdx.x;
    if (i < N) {
        const float4 v = ar[i];
        const float gx = ts_grad(alpha, v.x, v.z, inv_z), gy = ts_grad(alpha, v.y, v.w, inv_z);
        float2 yv = reinterpret_cast<float2 *>(y)[i], uv = reinterpret_cast<float2 *>(update)[i], gv = reinterpret_cast<float2 *>(gains)[i];
        ts_step(gx, mu, lr, gv.x, uv.x, yv.x);
        ts_step(gy, mu, lr, gv.y, uv.y, yv.y);
        reinterpret_cast<float2 *>(y)[i] = yv;
        reinterpret_cast<float2 *>(update)[i] = uv;
        reinterpret_cast<float2 *>(gains)[i] = gv;
        if (grad) reinterpret_cast<float2 *>(grad)[i] = make_float2(gx, gy);
    }
    if (CHECK && blockIdx.x == 0) {                        // (ar, zrow, lrow are read-only here: workgroup 0 sees what all others see)
        double gs = 0.0, ls = 0.0;
        for (int j = threadIdx.x; j < N; j += TS_THREADS) {
            const float4 v = ar[j];
            const float gx = ts_grad(alpha, v.x, v.z, inv_z), gy = ts_grad(alpha, v.y, v.w, inv_z);
            gs += (double)gx * (double)gx + (double)gy * (double)gy;
            ls += (double)lrow[j];
        }
        gs = ts_block_sum(gs, red);
        ls = ts_block_sum(ls, red);
        if (threadIdx.x == 0) {
            stats[0] = (float)((double)alpha * (pstats[1] + pstats[0] * (log((double)alpha) + log(Z)) + ls));
            stats[1] = (float)sqrt(gs);
        }
    }
}

static inline bool ts_supported(int N, int D) { return N >= 2 && N <= TS_MAX_N && D >= 1 && D <= TS_MAX_D; }
static inline size_t ts_align(size_t b) { return (b + 255) & ~(size_t)255; }
static inline int ts_tiles(int N) { return (N + TS_TILE - 1) / TS_TILE; }

extern "C" size_t ppt_tsne_affinities_workspace_bytes(int N, int D)
{
    if (!ts_supported(N, D)) return 0;
    return ts_align((size_t)ts_tiles(N) * ts_tiles(N) * 2 * sizeof(double));           // the tile sums of P and P log P
}

extern "C" int ppt_tsne_affinities(const float *x, int64_t ld, int N, int D, float perplexity, float *P, int64_t ldp, float *beta,
                                   double *pstats, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!x || !P || !beta || !pstats || !workspace || N <= 0 || D <= 0 || ld < D || ldp < N) return PPT_EINVAL;
    if (!(perplexity > 0.0f) || !isfinite(perplexity)) return PPT_EINVAL;
    if (((uintptr_t)x & 3) || ((uintptr_t)P & 15) || (ldp & 3) || ((uintptr_t)beta & 3) || ((uintptr_t)pstats & 7) ||
        ((uintptr_t)workspace & 255))
        return PPT_EINVAL;
    if (!ts_supported(N, D)) return PPT_EUNSUPPORTED;
    if (workspace_bytes < ppt_tsne_affinities_workspace_bytes(N, D)) return PPT_EINVAL;
    const size_t lds = ((size_t)((N + 3) & ~3) + (size_t)D) * sizeof(float);            // <= 80 KiB
    PPT_RAISE_LDS_ONCE((int)((TS_MAX_N + TS_MAX_D) * sizeof(float)), reinterpret_cast<const void *>(tsne_cond_kernel));
    const int vec = !((uintptr_t)x & 15) && !(ld & 3);
    const int T = ts_tiles(N);
    double *partial = reinterpret_cast<double *>(workspace);
    hipStream_t s = ppt_stream(stream);
    hipLaunchKernelGGL(tsne_cond_kernel, dim3((unsigned)N), dim3(TS_THREADS), lds, s, x, ld, N, D, vec, log((double)perplexity), P, ldp,
                       beta);
    PPT_CHECK_LAUNCH();
    hipLaunchKernelGGL(tsne_sym_kernel, dim3((unsigned)T, (unsigned)T), dim3(TS_THREADS), 0, s, P, ldp, N, T, partial);
    PPT_CHECK_LAUNCH();
    hipLaunchKernelGGL(tsne_pstats_kernel, dim3(1), dim3(TS_THREADS), 0, s, partial, T, pstats);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" size_t ppt_tsne_steps_workspace_bytes(int N)
{
    if (!ts_supported(N, 1)) return 0;
    return ts_align((size_t)N * sizeof(float4)) + 2 * ts_align((size_t)N * sizeof(float));
}

extern "C" int ppt_tsne_steps(const float *P, int64_t ldp, const double *pstats, int N, float *y, float *update, float *gains, int t0,
                              int n, int t_switch, float early_exaggeration, float lr, int check_every, float *stats, int stats_rows,
                              float *grad, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!P || !pstats || !y || !update || !gains || !workspace || N <= 0 || ldp < N || t0 < 0 || n < 1 || check_every < 0) return PPT_EINVAL;
    if (t0 > 0x7fffffff - n) return PPT_EINVAL;
    if (!(lr > 0.0f) || !isfinite(lr) || !(early_exaggeration > 0.0f) || !isfinite(early_exaggeration)) return PPT_EINVAL;
    if (((uintptr_t)P & 15) || (ldp & 3) || ((uintptr_t)pstats & 7) || ((uintptr_t)y & 7) || ((uintptr_t)update & 7) ||
        ((uintptr_t)gains & 7) || ((uintptr_t)grad & 7) || ((uintptr_t)stats & 3) || ((uintptr_t)workspace & 255))
        return PPT_EINVAL;
    if (!ts_supported(N, 1)) return PPT_EUNSUPPORTED;
    if (workspace_bytes < ppt_tsne_steps_workspace_bytes(N)) return PPT_EINVAL;
    const int checks = check_every ? (t0 + n) / check_every - t0 / check_every : 0;    // iterations t with (t + 1) % check_every == 0
    if (checks > 0 && (!stats || stats_rows < checks)) return PPT_EINVAL;

    char *ws = reinterpret_cast<char *>(workspace);
    float4 *ar = reinterpret_cast<float4 *>(ws);
    float *zrow = reinterpret_cast<float *>(ws + ts_align((size_t)N * sizeof(float4)));
    float *lrow = reinterpret_cast<float *>(ws + ts_align((size_t)N * sizeof(float4)) + ts_align((size_t)N * sizeof(float)));
    hipStream_t s = ppt_stream(stream);
    const int threads = N <= TS_PAIR_SMALL ? TS_THREADS : 1024, waves = threads / PPT_WAVE;
    const size_t lds = (size_t)((N + 3) & ~3) * sizeof(float2);                         // <= 128 KiB
    PPT_RAISE_LDS_ONCE((int)(TS_MAX_N * sizeof(float2)), reinterpret_cast<const void *>(tsne_pair_kernel<false>),
                       reinterpret_cast<const void *>(tsne_pair_kernel<true>));
    const int cus = ppt_cu_count(s);
    const int want = (N + waves - 1) / waves, cap = threads == TS_THREADS ? 2 * cus : cus;
    const unsigned grid_pair = (unsigned)(want < cap ? want : cap), grid_upd = (unsigned)((N + TS_THREADS - 1) / TS_THREADS);
    int row = 0;
    for (int t = t0; t < t0 + n; t++) {
        const float alpha = t < t_switch ? early_exaggeration : 1.0f, mu = t < t_switch ? 0.5f : 0.8f;
        const bool check = check_every && (t + 1) % check_every == 0;
        float *g = t == t0 + n - 1 ? grad : nullptr;
        if (check) {
            hipLaunchKernelGGL(tsne_pair_kernel<true>, dim3(grid_pair), dim3(threads), lds, s, P, ldp, N, y, ar, zrow, lrow);
            PPT_CHECK_LAUNCH();
            hipLaunchKernelGGL(tsne_update_kernel<true>, dim3(grid_upd), dim3(TS_THREADS), 0, s, ar, zrow, lrow, pstats, N, alpha, mu, lr, y,
                               update, gains, g, stats + 2 * (size_t)row++);
        } else {
            hipLaunchKernelGGL(tsne_pair_kernel<false>, dim3(grid_pair), dim3(threads), lds, s, P, ldp, N, y, ar, zrow, lrow);
            PPT_CHECK_LAUNCH();
            hipLaunchKernelGGL(tsne_update_kernel<false>, dim3(grid_upd), dim3(TS_THREADS), 0, s, ar, zrow, lrow, pstats, N, alpha, mu, lr, y,
                               update, gains, g, (float *)nullptr);
        }
        PPT_CHECK_LAUNCH();
    }
    return PPT_OK;
}
