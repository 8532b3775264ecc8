// cloud_prep.hip -- the device-resident input pipeline (ppt_amd/data/device_loader.py): everything the reference's datasets do
// to one sample after the row selection, and the random draws that drive it.
//
//   ppt_cloud_prep_f32   data/dataset_3d.py:33-38 pc_normalize, :155-160 translate_pointcloud, np.random.shuffle and the
//                        row gathers of ModelNet._get_item (:294-296), ScanObjectNN.__getitem__ (:407) and
//                        ShapeNetPart.__getitem__ (:752-755), for a whole batch in one launch.  One workgroup per output cloud;
//                        the gathered cloud (n <= 8192 rows x 12 B) sits in LDS and is read-only from then on.
//   ppt_cloud_draws      Philox4x32-10 draws for the same batch: FPS start, scale / shift, the shuffle permutation, the part-seg
//                        row choice.  One workgroup per sample.  (The generator itself is cloud_rng.h.)
// The reference's other augmentations -- rotation, dropout, scale, shift, jitter, ShapeNet's chain -- take a finished [B, n, 3] batch
// of this kernel as their input: cloud_augment.hip (ppt_cloud_augment_f32, ppt_cloud_draws_aug).
//
// The arithmetic of cloud_prep is the reference's, operation by operation, so the output is bit-identical to numpy's:
//   centroid   np.mean(pc, axis=0) of a C-contiguous [n,3] float32 array adds row after row (no pairwise tree along axis 0), then
//              divides by n: three lanes walk the rows in order.  The order is the contract; the sum is not parallelised.
//   radius     np.sqrt(np.sum(pc**2, axis=1)): (x*x + y*y) + z*z, each step rounded, then a correctly rounded sqrt.
//   scale      pc / m: a correctly rounded division, not a multiplication by 1/m.
//   translate  np.add(np.multiply(pc_f32, s_f64), t_f64).astype('float32'): product and sum in float64, ONE rounding to float32.
// Built with -ffp-contract=off and correctly rounded fp32 divide / sqrt (ppt_amd/build.py PER_FILE); sqrtf and `/` are used
// rather than __fsqrt_rn / __fdiv_rn because the HIP headers map __fsqrt_rn to the native (1 ulp) square root.
#include "ppt_common.h"
#include "cloud_rng.h"      // Philox4x32-10, the draw slots, uniform53, bounded

namespace {

constexpr int PREP_T = 256;            // threads per workgroup (4 waves)
constexpr int PREP_MAX_N = 8192;       // 96 KB of LDS for the gathered cloud
constexpr int PREP_HDR = 96;           // bytes of LDS in front of the cloud
constexpr int SUM_CHUNK = 16;          // rows fetched from LDS ahead of the dependent add chain

__device__ __forceinline__ int clampi(int64_t v, int hi)      // [0, hi - 1]: an index outside its range must not leave the buffer
{
    return v < 0 ? 0 : (v >= hi ? hi - 1 : (int)v);
}

struct prep_args {
    const float *src; int M, Nmax, C; const int32_t *lengths;
    const int64_t *item; const int64_t *sel; int n;
    int normalize, translate;
    const double *scale, *shift; const int32_t *perm;
    const int32_t *seg_src; int64_t *seg_out;
    float *out;
};

__global__ __launch_bounds__(PREP_T) void cloud_prep_kernel(prep_args a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    // header: centroid f32[3] @0, per-wave maxima f32[4] @16, scale f64[3] @32, shift f64[3] @56 -- per-axis values are read
    // from LDS by the axis index (written as selects over registers, the compiler builds a table in scratch memory instead)
    float *red = reinterpret_cast<float *>(smem);
    double *aff = reinterpret_cast<double *>(smem + 32);
    float *p = reinterpret_cast<float *>(smem + PREP_HDR);        // [n][3]
    const int t = threadIdx.x, b = blockIdx.x, n = a.n;
    const int it = clampi(a.item[b], a.M);
    const int len = a.lengths ? clampi((int64_t)a.lengths[it] - 1, a.Nmax) + 1 : a.Nmax;      // 1 .. Nmax
    const float *cloud = a.src + (size_t)it * a.Nmax * a.C;
    const int64_t *sel = a.sel ? a.sel + (size_t)b * n : nullptr;

    for (int i = t; i < n; i += PREP_T) {
        const int r = clampi(sel ? sel[i] : (int64_t)i, len);
        const float *q = cloud + (size_t)r * a.C;
        p[i * 3 + 0] = q[0]; p[i * 3 + 1] = q[1]; p[i * 3 + 2] = q[2];
    }
    __syncthreads();

    if (t < 3) {
        red[t] = 0.f;
        aff[t] = a.translate ? a.scale[b * 3 + t] : 1.0;
        aff[3 + t] = a.translate ? a.shift[b * 3 + t] : 0.0;
    }
    float m = 1.f;
    if (a.normalize) {
        if (t < 3) {
            float s = 0.f;
            int i = 0;
            for (; i + SUM_CHUNK <= n; i += SUM_CHUNK) {
                float v[SUM_CHUNK];
#pragma unroll
                for (int j = 0; j < SUM_CHUNK; ++j) v[j] = p[(i + j) * 3 + t];
#pragma unroll
                for (int j = 0; j < SUM_CHUNK; ++j) s = __fadd_rn(s, v[j]);
            }
            for (; i < n; ++i) s = __fadd_rn(s, p[i * 3 + t]);
            red[t] = s / (float)n;
        }
        __syncthreads();
        const float cx = red[0], cy = red[1], cz = red[2];
        float mx = 0.f;                                            // radii are >= +0
        for (int i = t; i < n; i += PREP_T) {
            const float x = __fsub_rn(p[i * 3 + 0], cx), y = __fsub_rn(p[i * 3 + 1], cy), z = __fsub_rn(p[i * 3 + 2], cz);
            const float r2 = __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
            mx = fmaxf(mx, sqrtf(r2));
        }
        mx = wave_reduce_max(mx);
        if ((t & 63) == 0) red[4 + (t >> 6)] = mx;
        __syncthreads();
        m = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    } else {
        __syncthreads();
    }
    const int32_t *perm = a.perm ? a.perm + (size_t)b * n : nullptr;
    const bool normalize = a.normalize != 0, translate = a.translate != 0;

    auto value = [=](int e) -> float {                             // element e of the flat [n*3] output
        const int row = e / 3, c = e - row * 3;
        const int r = perm ? clampi(perm[row], n) : row;
        float v = p[r * 3 + c];
        if (normalize) v = __fsub_rn(v, red[c]) / m;
        if (translate) v = (float)__dadd_rn(__dmul_rn((double)v, aff[c]), aff[3 + c]);
        return v;
    };
    float *out = a.out + (size_t)b * n * 3;
    if ((n & 3) == 0) {                                            // every cloud's 12 n bytes start 16-byte aligned
        for (int j = t; j < n * 3 / 4; j += PREP_T) {
            float4 v;
            v.x = value(4 * j); v.y = value(4 * j + 1); v.z = value(4 * j + 2); v.w = value(4 * j + 3);
            reinterpret_cast<float4 *>(out)[j] = v;
        }
    } else {
        for (int e = t; e < n * 3; e += PREP_T) out[e] = value(e);
    }
    if (a.seg_out) {
        const int32_t *seg = a.seg_src + (size_t)it * a.Nmax;
        for (int i = t; i < n; i += PREP_T) {
            const int row = perm ? clampi(perm[i], n) : i;
            a.seg_out[(size_t)b * n + i] = (int64_t)seg[clampi(sel ? sel[row] : (int64_t)row, len)];
        }
    }
}

struct draws_args {
    const int64_t *index; const int32_t *rows; int rows_all; int n;
    uint32_t epoch, k0, k1;
    int64_t *start; double *scale, *shift; int32_t *perm; int64_t *sel;
    int P;                                                         // n rounded up to a power of two (the sort's size)
};

constexpr int DRAW_T = 256;
constexpr int DRAW_MAX_N = 8192;       // 64 KB of (key, index) pairs

__global__ __launch_bounds__(DRAW_T) void cloud_draws_kernel(draws_args a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint64_t *kv = reinterpret_cast<uint64_t *>(smem);            // [P] (key << 32 | index): one compare orders both
    const int t = threadIdx.x, b = blockIdx.x, n = a.n;
    const uint32_t idx = (uint32_t)a.index[b];
    const int rows = a.rows ? a.rows[b] : a.rows_all;
    const uint32_t range = rows < 1 ? 1u : (uint32_t)rows;

    if (a.start && t == 0) a.start[b] = (int64_t)bounded(idx, a.epoch, SLOT_START, 0, a.k0, a.k1, range);
    if (a.scale && t < 3) {                                        // block c: words 0,1 -> the scale of axis c, words 2,3 -> its shift
        const philox_out r = philox4x32_10(idx, a.epoch, SLOT_AFFINE, (uint32_t)t, a.k0, a.k1);
        const double lo = 2.0 / 3.0, hi = 3.0 / 2.0;
        a.scale[b * 3 + t] = lo + (hi - lo) * uniform53(r.w[0], r.w[1]);     // np.random.uniform: low + (high - low) * u
        a.shift[b * 3 + t] = -0.2 + (0.2 - -0.2) * uniform53(r.w[2], r.w[3]);
    }
    if (a.sel)
        for (int i = t; i < n; i += DRAW_T)
            a.sel[(size_t)b * n + i] = (int64_t)bounded(idx, a.epoch, SLOT_SEL, (uint32_t)i, a.k0, a.k1, range);
    if (!a.perm) return;                                           // (uniform over the workgroup: no barrier is skipped by some)

    // the permutation: sort (32-bit key, index) pairs, ties by index -- a bitonic network over P >= n slots, padding sorts last
    const int P = a.P;
    for (int j = t; j < P / 4; j += DRAW_T) {
        const philox_out r = philox4x32_10(idx, a.epoch, SLOT_PERM, (uint32_t)j, a.k0, a.k1);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = 4 * j + q;
            kv[i] = i < n ? ((uint64_t)r.w[q] << 32) | (uint32_t)i : ~(uint64_t)0;
        }
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += DRAW_T) {
                const int l = i ^ j;
                if (l > i) {
                    const uint64_t x = kv[i], y = kv[l];
                    const bool up = (i & k) == 0;
                    if ((x > y) == up) { kv[i] = y; kv[l] = x; }
                }
            }
            __syncthreads();
        }
    for (int i = t; i < n; i += DRAW_T) a.perm[(size_t)b * n + i] = (int32_t)(uint32_t)kv[i];
}

__global__ void philox_raw_kernel(const uint32_t *ctr, int R, uint32_t k0, uint32_t k1, uint32_t *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R) return;
    const philox_out r = philox4x32_10(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], k0, k1);
    *reinterpret_cast<uint4 *>(out + 4 * i) = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]);
}

}  // namespace

extern "C" int ppt_cloud_prep_f32(const float *src, int M, int Nmax, int C, const int32_t *lengths, const int64_t *item, int B,
                                  const int64_t *sel, int n, int normalize, int translate, const double *scale,
                                  const double *shift, const int32_t *perm, const int32_t *seg_src, int64_t *seg_out, float *out,
                                  void *stream)
{
    if (!src || !item || !out || M <= 0 || Nmax <= 0 || Nmax > 16384 || C < 3 || B <= 0 || n <= 0 || n > PREP_MAX_N) return PPT_EINVAL;
    if (!sel && n > Nmax) return PPT_EINVAL;                       // rows 0 .. n-1 must exist
    if (translate && (!scale || !shift)) return PPT_EINVAL;
    if ((seg_src == nullptr) != (seg_out == nullptr)) return PPT_EINVAL;
    if (((uintptr_t)out & 15) != 0) return PPT_EINVAL;
    const size_t lds = PREP_HDR + (size_t)n * 12;
    static const hipError_t optin = hipFuncSetAttribute((const void *)cloud_prep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                        PREP_HDR + PREP_MAX_N * 12);
    if (lds > 64 * 1024 && optin != hipSuccess) return PPT_ELAUNCH;
    prep_args a{src, M, Nmax, C, lengths, item, sel, n, normalize, translate, scale, shift, perm, seg_src, seg_out, out};
    hipLaunchKernelGGL(cloud_prep_kernel, dim3(B), dim3(PREP_T), lds, ppt_stream(stream), a);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" int ppt_cloud_draws(const int64_t *index, int B, const int32_t *rows, int rows_all, int n, uint64_t seed, uint32_t epoch,
                               int64_t *start, double *scale, double *shift, int32_t *perm, int64_t *sel,
                               const uint32_t *raw_ctr, int raw_count, uint32_t *raw_out, void *stream)
{
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    hipStream_t s = ppt_stream(stream);
    const bool raw = raw_ctr || raw_out || raw_count;
    if (raw && (!raw_ctr || !raw_out || raw_count <= 0 || ((uintptr_t)raw_out & 15) != 0)) return PPT_EINVAL;
    const bool batch = index || B || start || scale || shift || perm || sel;
    if (!raw && !batch) return PPT_EINVAL;
    if (batch) {
        if (!index || B <= 0 || n <= 0 || n > DRAW_MAX_N) return PPT_EINVAL;
        if (!start && !scale && !perm && !sel) return PPT_EINVAL;
        if ((scale == nullptr) != (shift == nullptr)) return PPT_EINVAL;
        if ((start || sel) && !rows && (rows_all <= 0 || rows_all > 16384)) return PPT_EINVAL;
    }
    if (raw) {
        hipLaunchKernelGGL(philox_raw_kernel, dim3((raw_count + 255) / 256), dim3(256), 0, s, raw_ctr, raw_count, k0, k1, raw_out);
        PPT_CHECK_LAUNCH();
    }
    if (batch) {
        int P = 4;
        while (P < n) P <<= 1;
        draws_args a{index, rows, rows_all, n, epoch, k0, k1, start, scale, shift, perm, sel, P};
        hipLaunchKernelGGL(cloud_draws_kernel, dim3(B), dim3(DRAW_T), perm ? (size_t)P * 8 : 0, s, a);
        PPT_CHECK_LAUNCH();
    }
    return PPT_OK;
}
