// logreg.hip -- the few-shot linear probe's solver for gfx950: F independent L2-regularised multinomial logistic regressions
// in one launch, and the batched arg-max prediction that scores them.
//
// Replaces the sklearn.LogisticRegression(solver="lbfgs").fit / .predict calls of the reference's linear_probe.py:55-57,68-74,92
// (1 150 CPU fits per dataset with its defaults).  The fits are small (n <= 16 K rows, d = 768, K = 40 or 15) and independent, so
// the shape is fps.hip's: ONE persistent workgroup of 1024 threads per fit, the whole optimiser loop inside the kernel, no word
// exchanged between workgroups, no atomics.  Every reduction has a fixed order (DPP tree inside a wave, the 16 wave partials
// summed in wave order by every thread), so two runs write identical bytes and a fit does not see its neighbours.
//
//   minimise  F(W, b) = sum_i ( logsumexp_k z_ik - z_{i, y_i} ) + ||W||^2 / (2 C),   z_i = W x_i + b        (all fp32)
//
// L-BFGS, 10 pairs, Armijo backtracking.  Per iteration the features are read twice:
//   logits of the direction   ZD = X D^T     16 lanes per row, each lane a 1/16 slice of d, the direction in LDS when it fits
//                                            (K = 40, d = 768: 123 KB), row16_sum folds the slices;
//   gradient                  G = P^T X      4 columns of X by 8 classes per thread, P = softmax(Z) - onehot read 16 bytes at a time.
// Both walk the classes in chunks of 8 with 8 and 4 x 8 accumulators in VGPRs (compile-time indices: no scratch, and no per-class address
// in SGPRs); the class dimension is padded to a multiple of 8 (K8) in every vector and padded entries stay exactly zero.
// Parameter vectors are stored class-fastest, [d][K8] then the intercept [K8], so a chunk is two 16-byte loads.
// A line-search trial is Z + alpha ZD (one thread per row) and ||W + alpha D||^2 from three dot products: no pass over X.
// After every accepted step the intercept takes its exact iterative-scaling step (intercept_step below), again without X.
#include <cmath>
#include <type_traits>

#include "ppt_common.h"

namespace {

constexpr int LR_T = 1024;                 // threads per fit
constexpr int LR_R = 1024 / LR_T;          // rows of the fit per thread (n <= 1024)
constexpr int LR_WAVES = LR_T / 64;
constexpr int LR_M = 10;                   // (s, y) pairs
constexpr int LR_CHUNK = 128;              // fits per launch: their C values travel by value in the kernel arguments
constexpr int LR_LS_MAX = 30;              // halvings of a line search
constexpr float LR_C1 = 1e-4f;
constexpr float LR_EPS = 1.1920929e-7f;
constexpr int LR_LDS_FIXED = 4096 + 256 + 128 + 4096 + 512;        // s_row, red, s_rho + s_al, s_part, s_nk + s_delta (bytes)
constexpr int LR_LDS_MAX = 160 * 1024;

struct lr_cvals { float c[LR_CHUNK]; };

struct lr_dims {
    int K8, np;
    size_t P, Pp, per_fit;                 // floats
};

__host__ __device__ inline lr_dims lr_layout(int n, int d, int K)
{
    lr_dims L;
    L.K8 = (K + 7) & ~7;
    L.np = (n + 63) & ~63;
    L.P = (size_t)L.K8 * (d + 1);
    L.Pp = (L.P + 63) & ~(size_t)63;
    L.per_fit = (3 + 2 * LR_M) * L.Pp + 3 * (size_t)L.K8 * L.np;          // x, g, dir, S, Y | Z, ZD, P
    return L;
}

struct lr_ctx {
    const float *feat;
    int64_t ld;
    int n, d, K, K8;
    float *x, *g, *dir, *Z, *ZD, *Pb;          // parameters [d][K8] + [K8]; logits and P [n][K8]
    int32_t *s_row;
    float *red, *s_rho, *s_al, *s_part, *s_nk, *s_delta;          // s_nk: rows per class; s_delta: the intercept step
};

// sums of N values over the workgroup, returned to every thread with the same bits
template <int N>
__device__ __forceinline__ void block_sum(float (&v)[N], float *red)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = wave_reduce_sum(v[e]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < N; ++e) red[e * LR_WAVES + w] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < N; ++e) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < LR_WAVES; ++k) s += red[e * LR_WAVES + k];
        v[e] = s;
    }
}

__device__ __forceinline__ float block_max(float v, float *red)         // v >= 0
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = wave_reduce_max(v);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < LR_WAVES; ++k) m = fmaxf(m, red[k]);
    return m;
}

// The thread index behind a compiler barrier.  The optimiser loop below is one long loop around a dozen phases; whatever a phase
// derives from the thread index (row and column addresses, lane predicates) is invariant in that loop, and hoisted out of it all
// those values together do not fit the 128 VGPRs of a 1024-thread workgroup.  Each phase starts from an opaque copy instead.
__device__ __forceinline__ int phase_tid()
{
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

__device__ __forceinline__ void fma8(float (&acc)[8], const float4 a, const float4 b, float x)
{
    acc[0] = fmaf(a.x, x, acc[0]); acc[1] = fmaf(a.y, x, acc[1]); acc[2] = fmaf(a.z, x, acc[2]); acc[3] = fmaf(a.w, x, acc[3]);
    acc[4] = fmaf(b.x, x, acc[4]); acc[5] = fmaf(b.y, x, acc[5]); acc[6] = fmaf(b.z, x, acc[6]); acc[7] = fmaf(b.w, x, acc[7]);
}

// row i's loss at Z + alpha ZD, in three passes over its K logits (max, sum of exponentials, and with COMMIT the stores of the
// new logits and of P = softmax - onehot); padded classes count as -inf and are stored as zero
template <bool COMMIT>
__device__ __forceinline__ float row_loss(const lr_ctx &c, int i, int y, float alpha)
{
    float *zr = c.Z + i * c.K8, *pr = c.Pb + i * c.K8;
    const float *dr = c.ZD + i * c.K8;
    float m = -INFINITY;
    for (int k = 0; k < c.K; ++k) m = fmaxf(m, fmaf(alpha, dr[k], zr[k]));
    float s = 0.0f;
    for (int k = 0; k < c.K; ++k) s += expf(fmaf(alpha, dr[k], zr[k]) - m);
    const float zy = fmaf(alpha, dr[y], zr[y]);
    if constexpr (COMMIT) {
        const float inv = 1.0f / s;
        for (int k = 0; k < c.K; ++k) {
            const float z = fmaf(alpha, dr[k], zr[k]);
            zr[k] = z;
            pr[k] = expf(z - m) * inv - (k == y ? 1.0f : 0.0f);
        }
    }
    return (m + logf(s)) - zy;
}

// row i after the intercept moved by s_delta: its logits shifted, P and the loss at the new point
__device__ __forceinline__ float row_shift(const lr_ctx &c, int i, int y)
{
    float *zr = c.Z + i * c.K8;
    for (int k = 0; k < c.K; ++k) zr[k] += c.s_delta[k];
    return row_loss<true>(c, i, y, 0.0f);
}

// ZD = X dir_W^T + dir_b: 64 rows per pass, 16 lanes per row (lane l takes the columns l, l + 16, ...), 8 classes at a time
__device__ __forceinline__ void direction_logits(const lr_ctx &c)
{
    const int t = phase_tid(), grp = t >> 4, l16 = t & 15;
    const float *db = c.dir + c.K8 * c.d;
    for (int i0 = 0; i0 < c.n; i0 += LR_T / 16) {
        const int i = i0 + grp;
        const bool valid = i < c.n;
        const float *xr = c.feat + (size_t)c.s_row[valid ? i : 0] * c.ld;
        for (int k0 = 0; k0 < c.K8; k0 += 8) {
            float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            for (int j = l16; j < c.d; j += 16) {
                const float4 *dp = reinterpret_cast<const float4 *>(c.dir + j * c.K8 + k0);
                fma8(acc, dp[0], dp[1], xr[j]);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {                      // (all 64 lanes are back here: the DPP row sums see every slice)
                const float sum = row16_sum(acc[e]);
                if (valid && l16 == e) c.ZD[i * c.K8 + k0 + e] = sum + db[k0 + e];
            }
        }
    }
}

// out[k] = sum_i P[i, k] for k < K8: wave w sums rows w, w + 16, ... of column `lane`, the 16 partials are added in wave order.
// Ends with a barrier: `out` (global or LDS) is visible to the workgroup.
__device__ __forceinline__ void column_sums(const lr_ctx &c, float *out)
{
    const int t = phase_tid(), lane = t & 63, w = t >> 6;
    float s = 0.0f;
    if (lane < c.K8)
        for (int i = w; i < c.n; i += LR_WAVES) s += c.Pb[i * c.K8 + lane];
    c.s_part[w * 64 + lane] = s;
    __syncthreads();
    if (t < c.K8) {
        float a = 0.0f;
#pragma unroll
        for (int k = 0; k < LR_WAVES; ++k) a += c.s_part[k * 64 + t];
        out[t] = a;
    }
    __syncthreads();
}

// g = P^T X + W / C and g_b = column sums of P.  A work item is 4 columns of X (j, j + ceil(d / 4), ...: consecutive lanes read
// consecutive columns) by 8 classes, 32 accumulators: per row 6 loads feed 32 FMAs (one column by 8 classes is 3 loads for 8,
// and the loads bound it).  K = 40, d = 768: 960 items, one per thread.  A sum runs over the rows in order.
__device__ __forceinline__ void gradient(const lr_ctx &c, float invC)
{
    const int t = phase_tid();
    const int ncg = (c.d + 3) >> 2;
    for (int item = t; item < ncg * (c.K8 >> 3); item += LR_T) {
        const int k0 = (item / ncg) * 8, j0 = item % ncg;
        float acc[4][8];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[q][e] = 0.0f;
#pragma unroll 2
        for (int i = 0; i < c.n; ++i) {
            const float4 *pr = reinterpret_cast<const float4 *>(c.Pb + i * c.K8 + k0);
            const float *fr = c.feat + (size_t)c.s_row[i] * c.ld;
            const float4 a = pr[0], b = pr[1];
#pragma unroll
            for (int q = 0; q < 4; ++q) fma8(acc[q], a, b, j0 + q * ncg < c.d ? fr[j0 + q * ncg] : 0.0f);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = j0 + q * ncg;
            if (j < c.d) {
                const float4 *xp = reinterpret_cast<const float4 *>(c.x + j * c.K8 + k0);
                float4 *gp = reinterpret_cast<float4 *>(c.g + j * c.K8 + k0);
                const float4 xa = xp[0], xb = xp[1];
                gp[0] = make_float4(fmaf(xa.x, invC, acc[q][0]), fmaf(xa.y, invC, acc[q][1]), fmaf(xa.z, invC, acc[q][2]), fmaf(xa.w, invC, acc[q][3]));
                gp[1] = make_float4(fmaf(xb.x, invC, acc[q][4]), fmaf(xb.y, invC, acc[q][5]), fmaf(xb.z, invC, acc[q][6]), fmaf(xb.w, invC, acc[q][7]));
            }
        }
    }
    column_sums(c, c.g + c.K8 * c.d);
}

__global__ __launch_bounds__(LR_T) void logreg_fit_kernel(const float *__restrict__ feat, int64_t ld, int Nbank,
                                                          const int64_t *__restrict__ labels, const int32_t *__restrict__ rows,
                                                          int f0, int n, int d, int K, lr_cvals cv, float tol, int max_iter,
                                                          float *__restrict__ Wout, float *__restrict__ bout,
                                                          int32_t *__restrict__ info, float *__restrict__ ws, int dir_in_lds)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int t = threadIdx.x;
    const int f = f0 + blockIdx.x;
    const lr_dims L = lr_layout(n, d, K);

    lr_ctx c;
    c.feat = feat; c.ld = ld; c.n = n; c.d = d; c.K = K; c.K8 = L.K8;
    c.s_row = reinterpret_cast<int32_t *>(smem);
    c.red = reinterpret_cast<float *>(smem + 4096);
    c.s_rho = c.red + 64;
    c.s_al = c.s_rho + 16;
    c.s_part = c.s_al + 16;
    float *wsf = ws + (size_t)f * L.per_fit;
    c.x = wsf; c.g = c.x + L.Pp;
    c.s_nk = c.s_part + 1024;
    c.s_delta = c.s_nk + 64;
    c.dir = dir_in_lds ? c.s_delta + 64 : c.g + L.Pp;
    float *const S = c.g + 2 * L.Pp, *const Y = S + LR_M * L.Pp;
    c.Z = Y + LR_M * L.Pp; c.ZD = c.Z + (size_t)L.K8 * L.np; c.Pb = c.ZD + (size_t)L.K8 * L.np;
    const int P = (int)L.P, PW = L.K8 * d, Pp = (int)L.Pp;          // all parameters; the penalised ones (W) come first
    const float invC = 1.0f / cv.c[blockIdx.x];

    // the fit's rows and labels, checked before anything is read through them
    int bad = 0, y[LR_R];
#pragma unroll
    for (int r = 0; r < LR_R; ++r) {
        const int i = t + r * LR_T;
        y[r] = 0;
        if (i < n) {
            int row = rows[(size_t)f * n + i];
            if (row < 0 || row >= Nbank) { bad = 1; row = 0; }
            c.s_row[i] = row;
            const int64_t l = labels[row];
            if (l < 0 || l >= K) bad = 1; else y[r] = (int)l;
        }
    }
    {   // any thread's verdict, through the dynamic LDS (no static LDS in this kernel: the whole 160 KB can be requested)
        float v[1] = {(float)bad};
        block_sum<1>(v, c.red);
        bad = v[0] != 0.0f;
    }
    if (bad) {
        for (int e = t; e < K * d; e += LR_T) Wout[(size_t)f * K * d + e] = 0.0f;
        if (t < K) bout[(size_t)f * K + t] = 0.0f;
        if (t < PPT_LOGREG_INFO) info[(size_t)f * PPT_LOGREG_INFO + t] = t == 2 ? PPT_LOGREG_BADINPUT : 0;
        return;
    }

    if (t < L.K8) {                           // rows per class (the barrier of the check above published s_row)
        int cnt = 0;
        for (int i = 0; i < n; ++i) cnt += labels[c.s_row[i]] == t;
        c.s_nk[t] = (float)cnt;
    }
    for (int e = t; e < P; e += LR_T) { c.x[e] = 0.0f; c.dir[e] = 0.0f; }
    for (int e = t; e < 3 * L.K8 * L.np; e += LR_T) c.Z[e] = 0.0f;          // Z, ZD and P (their padding stays zero)
    __syncthreads();

    // the loss at Z + alpha ZD over this thread's rows
    auto loss_rows = [&](float alpha, auto commit) {
        float v = 0.0f;
        const int tt = phase_tid();
#pragma unroll
        for (int r = 0; r < LR_R; ++r) {
            const int i = tt + r * LR_T;
            if (i < n) v += row_loss<decltype(commit)::value>(c, i, y[r], alpha);
        }
        return v;
    };
    // The exact intercept step.  Given W, F is minimised over b where every class's probabilities sum to its number of rows;
    // b_k += log(n_k / sum_i softmax(z_i)_k) is the iterative-scaling step towards that point (monotone in F; exact when the
    // probabilities are near uniform) and needs no pass over X: the logits shift with b.  Taken at the start and after every
    // accepted step it keeps grad_b F at round-off, so where ||W x|| is tiny (C <= 1e-4) and the intercept alone decides the
    // arg-max, the point the stopping rule accepts has the optimum's intercept.  P must be current; it is current afterwards.
    // `Ss`: the step vector the move is added to (NULL at the start).  -> the loss sum at the new point.
    auto intercept_step = [&](float *Ss) {
        column_sums(c, c.s_delta);
        const int tt = phase_tid();
        if (tt < L.K8) {
            const float nk = c.s_nk[tt];
            const float dl = tt < K && nk > 0.0f ? logf(nk / (c.s_delta[tt] + nk)) : 0.0f;          // (P = softmax - onehot: + n_k)
            c.s_delta[tt] = dl;
            c.x[PW + tt] += dl;
            if (Ss) Ss[PW + tt] += dl;
        }
        __syncthreads();
        float v[1] = {0.0f};
#pragma unroll
        for (int r = 0; r < LR_R; ++r) {
            const int i = tt + r * LR_T;
            if (i < n) v[0] += row_shift(c, i, y[r]);
        }
        block_sum<1>(v, c.red);
        return v[0];
    };
    float fcur, gmax, gg;          // F, max |g| / n and g.g (a NaN anywhere in g shows in g.g)

    // F and its gradient at the start
    {
        float v[1] = {loss_rows(0.0f, std::true_type{})};
        block_sum<1>(v, c.red);
        fcur = intercept_step(nullptr);                      // (W = 0: no penalty term yet)
        gradient(c, invC);
        float gm = 0.0f, s[1] = {0.0f};
        for (int e = t; e < P; e += LR_T) { const float ge = c.g[e]; gm = fmaxf(gm, fabsf(ge)); s[0] = fmaf(ge, ge, s[0]); }
        block_sum<1>(s, c.red);
        gg = s[0];
        gm = block_max(gm, c.red);
        gmax = gg < INFINITY ? gm / (float)n : NAN;
    }

    int it = 0, nfev = 2, status, head = 0, cnt = 0;
    float gamma = 1.0f;
    while (true) {
        if (gmax <= tol) { status = PPT_LOGREG_CONVERGED; break; }
        if (it >= max_iter) { status = PPT_LOGREG_MAXITER; break; }
        const int t = phase_tid();

        // two-loop recursion: dir = -H g.  Every vector pass maps element e to thread e % 1024, so passes need no barrier
        // between them; the dot products bring their own (which also order the s_al hand-over between the two loops).
        for (int e = t; e < P; e += LR_T) c.dir[e] = c.g[e];
        for (int i = 0; i < cnt; ++i) {
            const int sl = (head + LR_M - 1 - i) % LR_M;
            const float *Ss = S + sl * Pp, *Ys = Y + sl * Pp;
            float v[1] = {0.0f};
            for (int e = t; e < P; e += LR_T) v[0] = fmaf(Ss[e], c.dir[e], v[0]);
            block_sum<1>(v, c.red);
            const float al = c.s_rho[sl] * v[0];
            if (t == 0) c.s_al[i] = al;
            for (int e = t; e < P; e += LR_T) c.dir[e] = fmaf(-al, Ys[e], c.dir[e]);
        }
        if (cnt > 0)
            for (int e = t; e < P; e += LR_T) c.dir[e] *= gamma;
        for (int i = cnt - 1; i >= 0; --i) {
            const int sl = (head + LR_M - 1 - i) % LR_M;
            const float *Ss = S + sl * Pp, *Ys = Y + sl * Pp;
            float v[1] = {0.0f};
            for (int e = t; e < P; e += LR_T) v[0] = fmaf(Ys[e], c.dir[e], v[0]);
            block_sum<1>(v, c.red);
            const float coef = c.s_al[i] - c.s_rho[sl] * v[0];
            for (int e = t; e < P; e += LR_T) c.dir[e] = fmaf(coef, Ss[e], c.dir[e]);
        }
        // dir = -q; the slope g.dir and the three products that give ||W + alpha D||^2
        float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int e = t; e < P; e += LR_T) {
            const float de = -c.dir[e], xe = c.x[e];
            c.dir[e] = de;
            q[0] = fmaf(c.g[e], de, q[0]);
            if (e < PW) { q[1] = fmaf(xe, xe, q[1]); q[2] = fmaf(xe, de, q[2]); q[3] = fmaf(de, de, q[3]); }
        }
        block_sum<4>(q, c.red);                               // (its barriers also publish dir to the whole workgroup)
        const float dg = q[0], ww = q[1], wd = q[2], dd = q[3];
        if (!(dg < 0.0f)) {                                   // not a descent direction (round-off in the history, or NaN)
            if (cnt > 0) { cnt = 0; continue; }
            status = PPT_LOGREG_LINESEARCH; break;
        }

        direction_logits(c);
        __syncthreads();

        // Armijo backtracking on phi(alpha) = loss(Z + alpha ZD) + (ww + 2 alpha wd + alpha^2 dd) / (2 C).  The slack of 4 ulp of F
        // is the resolution of an fp32 sum: without it the search fails next to the optimum, where the true decrease is below it.
        float alpha = cnt == 0 ? 1.0f / sqrtf(gg) : 1.0f;
        bool ok = false;
        for (int ls = 0; ls < LR_LS_MAX; ++ls) {
            float v[1] = {loss_rows(alpha, std::false_type{})};
            block_sum<1>(v, c.red);
            ++nfev;
            const float fnew = fmaf(0.5f * invC, fmaf(alpha, fmaf(alpha, dd, 2.0f * wd), ww), v[0]);
            if (fnew <= fcur + LR_C1 * alpha * dg + 4.0f * LR_EPS * fabsf(fcur)) { ok = true; break; }
            alpha *= 0.5f;
        }
        if (!ok) {
            ++it;
            if (cnt > 0) { cnt = 0; continue; }              // drop the history and try the gradient itself
            status = PPT_LOGREG_LINESEARCH; break;
        }

        // accept: x += alpha dir, s = alpha dir, y = -g_old for now
        float *Ss = S + head * Pp, *Ys = Y + head * Pp;
        float v2[2] = {0.0f, loss_rows(alpha, std::true_type{})};
        for (int e = t; e < P; e += LR_T) {
            const float se = alpha * c.dir[e], xe = c.x[e] + se;
            Ss[e] = se; Ys[e] = -c.g[e]; c.x[e] = xe;
            if (e < PW) v2[0] = fmaf(xe, xe, v2[0]);
        }
        block_sum<2>(v2, c.red);                              // (publishes x and P for the gradient)
        fcur = fmaf(0.5f * invC, v2[0], intercept_step(Ss));
        ++nfev;
        gradient(c, invC);
        float gm = 0.0f, r[3] = {0.0f, 0.0f, 0.0f};
        for (int e = t; e < P; e += LR_T) {
            const float ge = c.g[e], ye = Ys[e] + ge;
            Ys[e] = ye;
            r[0] = fmaf(Ss[e], ye, r[0]); r[1] = fmaf(ye, ye, r[1]); r[2] = fmaf(ge, ge, r[2]);
            gm = fmaxf(gm, fabsf(ge));
        }
        block_sum<3>(r, c.red);
        gg = r[2];
        gm = block_max(gm, c.red);
        gmax = gg < INFINITY ? gm / (float)n : NAN;
        if (r[0] > LR_EPS * r[1]) {                           // curvature safely positive: keep the pair
            if (t == 0) c.s_rho[head] = 1.0f / r[0];
            gamma = r[0] / r[1];
            head = (head + 1) % LR_M;
            cnt = cnt < LR_M ? cnt + 1 : LR_M;
        }
        __syncthreads();
        ++it;
    }

    for (int e = t; e < K * d; e += LR_T) Wout[(size_t)f * K * d + e] = c.x[(e % d) * L.K8 + e / d];          // [d][K8] -> [K][d]
    if (t < K) bout[(size_t)f * K + t] = c.x[PW + t];
    if (t == 0) {
        int32_t *o = info + (size_t)f * PPT_LOGREG_INFO;
        o[0] = it; o[1] = nfev; o[2] = status;
        o[3] = (int32_t)__float_as_uint(gmax); o[4] = (int32_t)__float_as_uint(fcur / (float)n);
        o[5] = 0; o[6] = 0; o[7] = 0;
    }
}

// 16 lanes per row, 4 rows per lane group, 64 rows per workgroup; blockIdx.y = fit; 8 classes at a time (the classes of the last
// chunk beyond K repeat class K - 1: read in bounds, never a new maximum)
__global__ __launch_bounds__(256) void logreg_predict_kernel(const float *__restrict__ feat, int64_t ld, int Nbank,
                                                             const int32_t *__restrict__ rows, int n_eval,
                                                             const float *__restrict__ W, const float *__restrict__ b, int d, int K,
                                                             int32_t *__restrict__ pred)
{
    const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
    const int f = blockIdx.y;
    const float *Wf = W + (size_t)f * K * d, *bf = b + (size_t)f * K;
    for (int r = 0; r < 4; ++r) {
        const int i = blockIdx.x * 64 + r * 16 + grp;
        const bool in_list = i < n_eval;
        const int row = in_list ? (rows ? rows[i] : i) : 0;
        const bool valid = in_list && row >= 0 && row < Nbank;
        const float *xr = feat + (valid ? (size_t)row * ld : 0);
        float bv = -INFINITY;
        int bi = 0;
        for (int k0 = 0; k0 < K; k0 += 8) {
            float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            for (int j = l16; j < d; j += 16) {
                const float x = xr[j];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = k0 + e < K ? k0 + e : K - 1;
                    acc[e] = fmaf(x, Wf[(size_t)k * d + j], acc[e]);
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = k0 + e < K ? k0 + e : K - 1;
                const float v = row16_sum(acc[e]) + bf[k];
                const bool take = v > bv;                     // strict: the first maximum wins (np.argmax)
                bv = take ? v : bv; bi = take ? k : bi;
            }
        }
        if (in_list && l16 == 0) pred[(size_t)f * n_eval + i] = valid ? bi : -1;
    }
}

bool lr_supported(int n, int d, int K) { return K >= 2 && K <= 64 && d >= 1 && d <= 1024 && n >= K && n <= 1024; }

int launch_fit(const float *feat, int64_t ld, int Nbank, const int64_t *labels, const int32_t *rows, int F, int n, int d, int K,
               const float *C, float tol, int max_iter, float *W, float *b, int32_t *info, float *ws, hipStream_t s)
{
    const lr_dims L = lr_layout(n, d, K);
    const size_t with_dir = LR_LDS_FIXED + L.Pp * sizeof(float);
    const int dir_in_lds = with_dir <= (size_t)LR_LDS_MAX;
    const size_t lds = dir_in_lds ? with_dir : LR_LDS_FIXED;
    PPT_RAISE_LDS_ONCE(LR_LDS_MAX, (const void *)logreg_fit_kernel);
    for (int f0 = 0; f0 < F; f0 += LR_CHUNK) {
        const int nf = F - f0 < LR_CHUNK ? F - f0 : LR_CHUNK;
        lr_cvals cv;
        for (int k = 0; k < LR_CHUNK; ++k) cv.c[k] = k < nf ? C[f0 + k] : 1.0f;
        hipLaunchKernelGGL(logreg_fit_kernel, dim3(nf), dim3(LR_T), lds, s, feat, ld, Nbank, labels, rows, f0, n, d, K, cv,
                           tol, max_iter, W, b, info, ws, dir_in_lds);
        PPT_CHECK_LAUNCH();
    }
    return PPT_OK;
}

}  // namespace

extern "C" size_t ppt_logreg_workspace_bytes(int F, int n, int d, int K)
{
    if (F <= 0 || !lr_supported(n, d, K)) return 0;
    return (size_t)F * lr_layout(n, d, K).per_fit * sizeof(float);
}

extern "C" int ppt_logreg_fit_f32(const float *feat, int64_t ld, int Nbank, const int64_t *labels, const int32_t *rows, int F, int n,
                                  int d, int K, const float *C, float tol, int max_iter, float *W, float *b, int32_t *info,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    if (!feat || !labels || !rows || !C || !W || !b || !info || !workspace) return PPT_EINVAL;
    if (F <= 0 || n <= 0 || d <= 0 || K <= 0 || Nbank <= 0 || ld < d || max_iter < 0 || !(tol >= 0.0f)) return PPT_EINVAL;
    for (int f = 0; f < F; ++f)
        if (!(C[f] > 0.0f) || !std::isfinite(C[f])) return PPT_EINVAL;
    if (!lr_supported(n, d, K)) return PPT_EUNSUPPORTED;
    if (workspace_bytes < ppt_logreg_workspace_bytes(F, n, d, K) || ((uintptr_t)workspace & 255)) return PPT_EINVAL;
    hipStream_t s = ppt_stream(stream);
    float *ws = static_cast<float *>(workspace);
    return launch_fit(feat, ld, Nbank, labels, rows, F, n, d, K, C, tol, max_iter, W, b, info, ws, s);
}

extern "C" int ppt_logreg_predict_f32(const float *feat, int64_t ld, int Nbank, const int32_t *rows, int n_eval, const float *W,
                                      const float *b, int F, int d, int K, int32_t *pred, void *stream)
{
    if (!feat || !W || !b || !pred || F <= 0 || n_eval <= 0 || d <= 0 || K <= 0 || Nbank <= 0 || ld < d) return PPT_EINVAL;
    if (!rows && n_eval > Nbank) return PPT_EINVAL;
    if (K < 2 || K > 64 || d > 1024 || F > 65535) return PPT_EUNSUPPORTED;
    hipStream_t s = ppt_stream(stream);
    const dim3 grid((n_eval + 63) / 64, F);
    hipLaunchKernelGGL(logreg_predict_kernel, grid, dim3(256), 0, s, feat, ld, Nbank, rows, n_eval, W, b, d, K, pred);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}
