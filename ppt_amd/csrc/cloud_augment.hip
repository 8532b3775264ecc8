// cloud_augment.hip -- the reference's point-cloud augmentations (data/dataset_3d.py:63-153) on a finished device batch, and the
// Philox draws that drive them (ppt_amd/data/augment.py, ppt_amd/data/device_loader.py).
//
//   ppt_cloud_augment_f32   an ordered list of at most 8 stages applied to pc [B, n, 3] f32 (what ppt_cloud_prep_f32 returns).  One
//                           workgroup per cloud; the cloud (n <= 8192 rows x 12 B) sits in LDS, every stage is one pass over that
//                           copy with a barrier behind it, and the result is stored once: [B, n, 3], or [B, n, 4] when the height
//                           stage closes the list.
//   ppt_cloud_draws_aug     the draws of those stages from Philox4x32-10 (cloud_rng.h), slots 4-10, one workgroup per sample.
//
// The arithmetic of a stage is numpy's (>= 2), operation by operation, so the output is bit-identical given the same parameters:
//   dropout   batch_pc[b, drop_idx, :] = batch_pc[b, 0, :]                       rows under the mask take row 0 as it is at this stage
//   scale     batch_data[b] *= np.float64 scalar                                (float)((double)v * s): the product in double, rounded once
//   shift     batch_data[b] += f64 [3]                                          (float)((double)v + t[c])
//   rotate    f32 array <- np.dot(pc, R), R f64 [3, 3]                          (float)(((double)x*R[0][c] + (double)y*R[1][c]) + (double)z*R[2][c])
//   jitter    clip(sigma * randn) += batch_data                                 (float)(noise + (double)v)   (the reference keeps float64)
//   affine    np.add(np.multiply(pc, s), t).astype('float32')                   translate_pointcloud, as cloud_prep.hip does it
//   height    y - min_i y in fp32, as ppt_cloud_height_f32 (csrc/pointnext.hip)
// Built with -ffp-contract=off (ppt_amd/build.py PER_FILE): no product is fused into a sum.  Two rotate stages stay two stages --
// the reference rounds to float32 between them.
#include "ppt_common.h"
#include "cloud_rng.h"

namespace {

constexpr int AUG_T = 256;             // threads per workgroup (4 waves)
constexpr int AUG_MAX_N = 8192;        // 96 KB of LDS for the cloud
constexpr int AUG_PAR = 9;             // doubles of per-cloud parameters a stage may have (a 3 x 3 matrix)
constexpr int AUG_HDR = PPT_AUG_MAX_STAGES * AUG_PAR * 8 + 32;      // parameters f64[8][9] @0, per-wave minima f32[4] @576; 608 B

struct aug_args {
    const float *pc; int n; int count;
    int kind[PPT_AUG_MAX_STAGES]; const void *a[PPT_AUG_MAX_STAGES]; const void *b[PPT_AUG_MAX_STAGES];
    float *out;
};

__global__ __launch_bounds__(AUG_T) void cloud_augment_kernel(aug_args g)
{
    extern __shared__ __align__(16) unsigned char smem[];
    double *par = reinterpret_cast<double *>(smem);                // [count][AUG_PAR]: read by the axis index (see cloud_prep.hip)
    float *red = reinterpret_cast<float *>(smem + PPT_AUG_MAX_STAGES * AUG_PAR * 8);
    float *p = reinterpret_cast<float *>(smem + AUG_HDR);          // [n][3]
    const int t = threadIdx.x, b = blockIdx.x, n = g.n, E = n * 3;
    const float *src = g.pc + (size_t)b * E;

    if (t < g.count * AUG_PAR) {                                   // count <= 8: 72 threads at the most
        const int s = t / AUG_PAR, j = t - s * AUG_PAR;
        const double *a = static_cast<const double *>(g.a[s]), *bb = static_cast<const double *>(g.b[s]);
        double v = 0.0;
        switch (g.kind[s]) {
        case PPT_AUG_SCALE:  if (j < 1) v = a[b]; break;
        case PPT_AUG_SHIFT:  if (j < 3) v = a[b * 3 + j]; break;
        case PPT_AUG_ROTATE: v = a[(size_t)b * 9 + j]; break;
        case PPT_AUG_AFFINE: if (j < 3) v = a[b * 3 + j]; else if (j < 6) v = bb[b * 3 + j - 3]; break;
        default: break;
        }
        par[t] = v;
    }
    if ((n & 3) == 0 && ((uintptr_t)g.pc & 15) == 0) {             // every cloud's 12 n bytes start 16-byte aligned
        for (int j = t; j < E / 4; j += AUG_T) reinterpret_cast<float4 *>(p)[j] = reinterpret_cast<const float4 *>(src)[j];
    } else {
        for (int e = t; e < E; e += AUG_T) p[e] = src[e];
    }
    __syncthreads();

    bool height = false;
    for (int s = 0; s < g.count; ++s) {                            // uniform over the workgroup: every thread meets every barrier
        const double *q = par + s * AUG_PAR;
        switch (g.kind[s]) {
        case PPT_AUG_DROPOUT: {
            const uint8_t *mask = static_cast<const uint8_t *>(g.a[s]) + (size_t)b * n;
            const float x0 = p[0], y0 = p[1], z0 = p[2];           // row 0 is never changed by this stage (it can only take itself)
            for (int i = t; i < n; i += AUG_T)
                if (mask[i]) { p[i * 3 + 0] = x0; p[i * 3 + 1] = y0; p[i * 3 + 2] = z0; }
            break;
        }
        case PPT_AUG_SCALE: {
            const double sc = q[0];
            for (int e = t; e < E; e += AUG_T) p[e] = (float)__dmul_rn((double)p[e], sc);
            break;
        }
        case PPT_AUG_SHIFT:
            for (int e = t; e < E; e += AUG_T) p[e] = (float)__dadd_rn((double)p[e], q[e % 3]);
            break;
        case PPT_AUG_ROTATE:
            for (int i = t; i < n; i += AUG_T) {
                const double x = (double)p[i * 3 + 0], y = (double)p[i * 3 + 1], z = (double)p[i * 3 + 2];
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    p[i * 3 + c] = (float)__dadd_rn(__dadd_rn(__dmul_rn(x, q[c]), __dmul_rn(y, q[3 + c])), __dmul_rn(z, q[6 + c]));
            }
            break;
        case PPT_AUG_JITTER: {
            const double *noise = static_cast<const double *>(g.a[s]) + (size_t)b * E;
            for (int e = t; e < E; e += AUG_T) p[e] = (float)__dadd_rn(noise[e], (double)p[e]);
            break;
        }
        case PPT_AUG_AFFINE:
            for (int e = t; e < E; e += AUG_T) {
                const int c = e % 3;
                p[e] = (float)__dadd_rn(__dmul_rn((double)p[e], q[c]), q[3 + c]);
            }
            break;
        default:                                                   // PPT_AUG_HEIGHT (the last stage; checked by the host)
            height = true;
            break;
        }
        __syncthreads();
    }

    if (height) {
        float m = -INFINITY;                                       // min y = -max(-y): exact, and the DPP max reduction is at hand
        for (int i = t; i < n; i += AUG_T) m = fmaxf(m, -p[i * 3 + 1]);
        m = wave_reduce_max(m);
        if ((t & 63) == 0) red[t >> 6] = m;
        __syncthreads();
        const float ymin = -fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        float *out = g.out + (size_t)b * n * 4;
        for (int i = t; i < n; i += AUG_T) {
            const float x = p[i * 3 + 0], y = p[i * 3 + 1], z = p[i * 3 + 2];
            *reinterpret_cast<float4 *>(out + (size_t)i * 4) = make_float4(x, y, z, __fsub_rn(y, ymin));
        }
        return;
    }
    float *out = g.out + (size_t)b * E;
    if ((n & 3) == 0) {
        for (int j = t; j < E / 4; j += AUG_T) reinterpret_cast<float4 *>(out)[j] = reinterpret_cast<const float4 *>(p)[j];
    } else {
        for (int e = t; e < E; e += AUG_T) out[e] = p[e];
    }
}

// ---- the draws ---------------------------------------------------------------------------------------------------------------------
struct aug_draws_args {
    const int64_t *index; int n; uint32_t epoch, k0, k1;
    double max_dropout, scale_low, scale_high, shift_range, angle_sigma, angle_clip, jitter_sigma, jitter_clip;
    double *ratio; uint8_t *mask; double *scale, *shift, *angles, *perturb, *angle, *rotate, *noise;
};

constexpr double TWO_PI = 6.283185307179586;                       // the double nearest 2 pi (= 2 * np.pi)

__device__ __forceinline__ double clipd(double v, double c)        // np.clip(v, -c, c) = min(max(v, -c), c)
{
    return fmin(fmax(v, -c), c);
}

// Box-Muller in fp64 on one Philox block: u1 = uniform53(w0, w1), u2 = uniform53(w2, w3), r = sqrt(-2 log(1 - u1)) (1 - u1 is in
// (0, 1]: the logarithm's argument is never 0), z0 = r cos(2 pi u2), z1 = r sin(2 pi u2).
__device__ __forceinline__ void box_muller(const philox_out &w, double &z0, double &z1)
{
    const double u1 = uniform53(w.w[0], w.w[1]), u2 = uniform53(w.w[2], w.w[3]);
    const double r = sqrt(__dmul_rn(-2.0, log(__dsub_rn(1.0, u1)))), th = __dmul_rn(TWO_PI, u2);
    z0 = __dmul_rn(r, cos(th));
    z1 = __dmul_rn(r, sin(th));
}

__device__ __forceinline__ void matmul3(const double *A, const double *B, double *C)      // row-major, each sum left to right, unfused
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            C[i * 3 + j] = __dadd_rn(__dadd_rn(__dmul_rn(A[i * 3], B[j]), __dmul_rn(A[i * 3 + 1], B[3 + j])), __dmul_rn(A[i * 3 + 2], B[6 + j]));
}

__global__ __launch_bounds__(AUG_T) void cloud_draws_aug_kernel(aug_draws_args a)
{
    const int t = threadIdx.x, b = blockIdx.x, n = a.n;
    const uint32_t idx = (uint32_t)a.index[b];

    if (a.mask) {                                                  // every thread derives the ratio: no hand-over through memory
        const philox_out r0 = philox4x32_10(idx, a.epoch, SLOT_DROP_RATIO, 0, a.k0, a.k1);
        const double ratio = __dmul_rn(uniform53(r0.w[0], r0.w[1]), a.max_dropout);
        if (t == 0 && a.ratio) a.ratio[b] = ratio;
        for (int j = t; j < (n + 1) / 2; j += AUG_T) {             // block j: words 0,1 -> row 2j, words 2,3 -> row 2j + 1
            const philox_out r = philox4x32_10(idx, a.epoch, SLOT_DROP_MASK, (uint32_t)j, a.k0, a.k1);
            a.mask[(size_t)b * n + 2 * j] = uniform53(r.w[0], r.w[1]) <= ratio;
            if (2 * j + 1 < n) a.mask[(size_t)b * n + 2 * j + 1] = uniform53(r.w[2], r.w[3]) <= ratio;
        }
    }
    if (a.scale && t == 0) {
        const philox_out r = philox4x32_10(idx, a.epoch, SLOT_SCALE, 0, a.k0, a.k1);
        a.scale[b] = __dadd_rn(a.scale_low, __dmul_rn(__dsub_rn(a.scale_high, a.scale_low), uniform53(r.w[0], r.w[1])));
    }
    if (a.shift && t < 3) {                                        // block c: words 0,1 -> axis c
        const philox_out r = philox4x32_10(idx, a.epoch, SLOT_SHIFT, (uint32_t)t, a.k0, a.k1);
        a.shift[b * 3 + t] = __dadd_rn(-a.shift_range, __dmul_rn(__dsub_rn(a.shift_range, -a.shift_range), uniform53(r.w[0], r.w[1])));
    }
    if (a.perturb && t == 0) {                                     // block 0: z0, z1 -> angles 0, 1; block 1: z0 -> angle 2
        double z[4];
        box_muller(philox4x32_10(idx, a.epoch, SLOT_PERTURB, 0, a.k0, a.k1), z[0], z[1]);
        box_muller(philox4x32_10(idx, a.epoch, SLOT_PERTURB, 1, a.k0, a.k1), z[2], z[3]);
        double ang[3], cs[3], sn[3];
        for (int c = 0; c < 3; ++c) {
            ang[c] = clipd(__dmul_rn(a.angle_sigma, z[c]), a.angle_clip);
            cs[c] = cos(ang[c]); sn[c] = sin(ang[c]);
            if (a.angles) a.angles[b * 3 + c] = ang[c];
        }
        const double Rx[9] = {1, 0, 0, 0, cs[0], -sn[0], 0, sn[0], cs[0]};
        const double Ry[9] = {cs[1], 0, sn[1], 0, 1, 0, -sn[1], 0, cs[1]};
        const double Rz[9] = {cs[2], -sn[2], 0, sn[2], cs[2], 0, 0, 0, 1};
        double M[9], R[9];
        matmul3(Ry, Rx, M);
        matmul3(Rz, M, R);                                         // R = Rz (Ry Rx), dataset_3d.py:150
        for (int j = 0; j < 9; ++j) a.perturb[(size_t)b * 9 + j] = R[j];
    }
    if (a.rotate && t == 0) {
        const philox_out r = philox4x32_10(idx, a.epoch, SLOT_ROTATE, 0, a.k0, a.k1);
        const double ang = __dmul_rn(uniform53(r.w[0], r.w[1]), TWO_PI), c = cos(ang), s = sin(ang);
        if (a.angle) a.angle[b] = ang;
        const double R[9] = {c, 0, s, 0, 1, 0, -s, 0, c};          // about y, dataset_3d.py:76-78
        for (int j = 0; j < 9; ++j) a.rotate[(size_t)b * 9 + j] = R[j];
    }
    if (a.noise) {                                                 // block j: z0 -> flat element 2j, z1 -> 2j + 1 of the cloud's [n*3]
        const int E = n * 3;
        double *noise = a.noise + (size_t)b * E;
        for (int j = t; j < (E + 1) / 2; j += AUG_T) {
            double z0, z1;
            box_muller(philox4x32_10(idx, a.epoch, SLOT_JITTER, (uint32_t)j, a.k0, a.k1), z0, z1);
            noise[2 * j] = clipd(__dmul_rn(a.jitter_sigma, z0), a.jitter_clip);
            if (2 * j + 1 < E) noise[2 * j + 1] = clipd(__dmul_rn(a.jitter_sigma, z1), a.jitter_clip);
        }
    }
}

}  // namespace

extern "C" int ppt_cloud_augment_f32(const float *pc, int B, int n, const ppt_aug_stage *stages, int count, float *out, void *stream)
{
    if (!pc || !out || B <= 0 || n <= 0 || !stages || count <= 0 || count > PPT_AUG_MAX_STAGES) return PPT_EINVAL;
    if (((uintptr_t)out & 15) != 0 || ((uintptr_t)pc & 3) != 0) return PPT_EINVAL;
    aug_args a{};
    a.pc = pc; a.n = n; a.count = count; a.out = out;
    for (int s = 0; s < count; ++s) {
        const ppt_aug_stage &st = stages[s];
        switch (st.kind) {
        case PPT_AUG_DROPOUT: case PPT_AUG_SCALE: case PPT_AUG_SHIFT: case PPT_AUG_ROTATE: case PPT_AUG_JITTER:
            if (!st.a) return PPT_EINVAL;
            break;
        case PPT_AUG_AFFINE:
            if (!st.a || !st.b) return PPT_EINVAL;
            break;
        case PPT_AUG_HEIGHT:
            if (s != count - 1) return PPT_EINVAL;
            break;
        default:
            return PPT_EINVAL;
        }
        if (st.kind != PPT_AUG_DROPOUT && st.kind != PPT_AUG_HEIGHT && ((uintptr_t)st.a & 7) != 0) return PPT_EINVAL;
        if (st.kind == PPT_AUG_AFFINE && ((uintptr_t)st.b & 7) != 0) return PPT_EINVAL;
        a.kind[s] = st.kind; a.a[s] = st.a; a.b[s] = st.b;
    }
    if (n > AUG_MAX_N) return PPT_EUNSUPPORTED;                    // a valid cloud, but larger than the LDS copy this kernel works on
    const size_t lds = AUG_HDR + (size_t)n * 12;
    static const hipError_t optin = hipFuncSetAttribute((const void *)cloud_augment_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                        AUG_HDR + AUG_MAX_N * 12);
    if (lds > 64 * 1024 && optin != hipSuccess) return PPT_ELAUNCH;
    hipLaunchKernelGGL(cloud_augment_kernel, dim3(B), dim3(AUG_T), lds, ppt_stream(stream), a);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" int ppt_cloud_draws_aug(const int64_t *index, int B, int n, uint64_t seed, uint32_t epoch, const double *magnitudes,
                                   double *ratio, uint8_t *mask, double *scale, double *shift, double *angles, double *perturb,
                                   double *angle, double *rotate, double *noise, void *stream)
{
    if (!index || B <= 0 || n <= 0) return PPT_EINVAL;
    if (!mask && !scale && !shift && !perturb && !rotate && !noise) return PPT_EINVAL;
    if ((ratio && !mask) || (angles && !perturb) || (angle && !rotate)) return PPT_EINVAL;      // a by-product without its draw
    if (n > AUG_MAX_N) return PPT_EUNSUPPORTED;
    static const double defaults[PPT_AUG_MAGNITUDES] = {0.875, 0.8, 1.25, 0.1, 0.06, 0.18, 0.01, 0.05};
    const double *m = magnitudes ? magnitudes : defaults;
    for (int i = 0; i < PPT_AUG_MAGNITUDES; ++i)
        if (!(m[i] == m[i]) || m[i] - m[i] != 0.0) return PPT_EINVAL;                            // NaN or infinite
    aug_draws_args a{index, n, epoch, (uint32_t)seed, (uint32_t)(seed >> 32), m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7],
                     ratio, mask, scale, shift, angles, perturb, angle, rotate, noise};
    hipLaunchKernelGGL(cloud_draws_aug_kernel, dim3(B), dim3(AUG_T), 0, ppt_stream(stream), a);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}
