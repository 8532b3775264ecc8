// meters.hip -- the training loops' per-step figures on the device (ppt_amd/recognition.py, ppt_amd/partseg.py): what
// main_cls.py:200-217 and main_partseg.py:218-243 take out of a step with `.item()` reads (the loss for the finite check, the
// accuracy, and in part segmentation one label per cloud) folded into ONE running record of PPT_METER_REC doubles per epoch, by one
// launch per step.  The host reads the record once, at the end of the epoch.
//
//   train_meter_cls_kernel      one workgroup: wave w takes rows w, w + 4, ...; inside a row the lanes share the classes and a
//                               butterfly picks the first maximum (the idiom of csrc/metrics.hip); thread 0 folds the step.
//   train_meter_partseg_kernel  one workgroup per MT_CHUNK points of one cloud, lane = point, the arg-max walks the category's part
//                               range only.  Workgroups add their integer counts with integer atomics into `scratch`; the last to
//                               arrive folds the step into the record and clears the scratch for the next call.
// The record's sums are AverageMeter.update's (utils/utils.py:333-337): sum += val * n in double, step after step, val the fp32
// figure widened to double (what .item() returns).  No floating-point atomics: the same calls write the same bytes.
#include "ppt_common.h"
#include <math.h>

#define MT_THREADS 256
#define MT_WAVES (MT_THREADS / PPT_WAVE)
#define MT_CHUNK MT_THREADS                // points of one cloud per workgroup

namespace {

__device__ __forceinline__ bool mt_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// (float)correct / (float)total as torch divides: both operands rounded to fp32, the quotient formed in double and rounded once
// (53 >= 2 * 24 + 2: the double quotient of two fp32 values rounds to the correctly rounded fp32 quotient)
__device__ __forceinline__ float mt_ratio(long long correct, long long total)
{
    return (float)((double)(float)correct / (double)(float)total);
}

// one step into the record; every product and sum is rounded on its own (the file is built without contraction)
__device__ __forceinline__ void mt_fold(double *__restrict__ rec, const float *__restrict__ loss, float acc, double weight, int metered,
                                        bool bad_label)
{
    const float lf = *loss;
    rec[3] += 1.0;
    if (mt_nonfinite(lf)) rec[4] += 1.0;                   // main_cls.py:205: the finite check sits in front of the `continue`
    if (bad_label) rec[7] += 1.0;
    if (!metered) return;
    const double l = (double)lf, a = (double)acc;
    rec[0] += l * weight;
    rec[1] += a * weight;
    rec[2] += weight;
    rec[5] = l;
    rec[6] = a;
}

__global__ __launch_bounds__(MT_THREADS) void train_meter_cls_kernel(const float *__restrict__ logits, const int64_t *__restrict__ labels,
                                                                     const float *__restrict__ loss, int B, int C, double weight,
                                                                     int metered, double *__restrict__ rec)
{
    __shared__ int wave_correct[MT_WAVES], wave_bad[MT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int correct = 0, bad = 0;                              // wave-uniform
    for (int row = wave; row < B; row += MT_WAVES) {
        const float *x = logits + (size_t)row * C;
        float best = -INFINITY;
        int idx = 0x7fffffff, nan = 0;
        for (int c = lane; c < C; c += PPT_WAVE) {         // ascending inside a lane: `>` keeps the first maximum
            const float v = x[c];
            nan |= v != v ? 1 : 0;
            if (v > best || idx == 0x7fffffff) { best = v; idx = c; }
        }
        for (int o = 32; o; o >>= 1) {
            const float ob = __shfl_xor(best, o);
            const int oi = __shfl_xor(idx, o);
            if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
        }
        const bool any_nan = __builtin_amdgcn_ballot_w64(nan != 0) != 0;
        const int64_t t = labels[row];
        const bool out = t < 0 || t >= (int64_t)C;
        bad |= out ? 1 : 0;
        correct += (!any_nan && !out && (int64_t)idx == t) ? 1 : 0;
    }
    if (lane == 0) { wave_correct[wave] = correct; wave_bad[wave] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0, b = 0;
        for (int w = 0; w < MT_WAVES; w++) { n += wave_correct[w]; b |= wave_bad[w]; }
        mt_fold(rec, loss, mt_ratio(n, B), weight, metered, b != 0);
    }
}

// RAGGED (ppt_train_meter_partseg_ragged): N is the slabs' row stride, cloud b its first lengths[b] rows; nothing behind them is
// read, a chunk wholly behind a cloud's end counts nothing and still draws its ticket, and the accuracy's denominator is the sum of
// the lengths.  A compile-time flag, lengths the last argument: the uniform instantiation is the kernel it was.
template <bool RAGGED>
__global__ __launch_bounds__(MT_THREADS) void train_meter_partseg_kernel(const float *__restrict__ logits, const int64_t *__restrict__ labels,
                                                                         const float *__restrict__ loss, int B, int N, int P, int chunks,
                                                                         const int32_t *__restrict__ part_start,
                                                                         const int32_t *__restrict__ part_count, double weight,
                                                                         int metered, double *__restrict__ rec, unsigned *scratch,
                                                                         const int32_t *__restrict__ lengths)
{
    __shared__ int wave_correct[MT_WAVES], wave_bad[MT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const int n = chunk * MT_CHUNK + tid;
    const int64_t *lab = labels + (size_t)b * N;

    // the cloud's category is the one point 0's label belongs to (main_partseg.py:222-225).  The tables are device memory the host
    // entry cannot look into: clamp what they say so that no index below can leave the row.
    const int64_t l0 = lab[0];
    const bool bad_cat = l0 < 0 || l0 >= (int64_t)P;
    int start = bad_cat ? 0 : part_start[l0];
    int count = bad_cat ? 0 : part_count[l0];
    start = max(0, min(start, P));
    count = max(0, min(count, P - start));

    int n_rows = N;
    if constexpr (RAGGED) n_rows = max(1, min((int)lengths[b], N));      // (clamped: a bad length must not leave the slab)
    bool hit = false, out = false;
    if (n < n_rows) {
        const int64_t t = lab[n];
        out = t < 0 || t >= (int64_t)P;
        if (count > 0) {
            const float *x = logits + ((size_t)b * N + n) * P + start;
            float best = x[0];
            int pred = 0;
            for (int j = 1; j < count; j++) {              // the first maximum wins (torch.argmax, :225)
                const float v = x[j];
                if (v > best) { best = v; pred = j; }
            }
            hit = (int64_t)(start + pred) == t;
        }
    }
    const int correct = __popcll(__builtin_amdgcn_ballot_w64(hit));
    const bool any_out = __builtin_amdgcn_ballot_w64(out) != 0;
    if (lane == 0) { wave_correct[wave] = correct; wave_bad[wave] = (any_out || bad_cat) ? 1 : 0; }
    __syncthreads();
    if (tid != 0) return;
    int c = 0, bd = 0;
    for (int w = 0; w < MT_WAVES; w++) { c += wave_correct[w]; bd |= wave_bad[w]; }
    if (c) atomicAdd(scratch + 0, (unsigned)c);
    if (bd) atomicOr(scratch + 2, 1u);
    // release: the two atomics above return nothing, so nothing waits for them by itself -- they must have been performed before
    // the ticket is drawn (the explicit wait stands behind the fence on purpose: the compiler may drop the fence's own)
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned ticket = atomicAdd(scratch + 1, 1u);
    if (ticket != gridDim.x - 1u) return;
    // ---- the last workgroup to get here: fold the step, leave the scratch as it was found (all zero) ---------------------------
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned total = __hip_atomic_load(scratch + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned flags = __hip_atomic_load(scratch + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    long long points = (long long)B * N;
    if constexpr (RAGGED) {
        points = 0;
        for (int i = 0; i < B; i++) points += max(1, min((int)lengths[i], N));
    }
    mt_fold(rec, loss, mt_ratio((long long)total, points), weight, metered, flags != 0);
    __hip_atomic_store(scratch + 0, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(scratch + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(scratch + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

extern "C" int ppt_train_meter_cls(const float *logits, const int64_t *labels, const float *loss, int B, int C, double weight,
                                   int metered, double *rec, void *stream)
{
    if (!logits || !labels || !loss || !rec || B <= 0 || C <= 0) return PPT_EINVAL;
    if (((uintptr_t)rec & 7) || ((uintptr_t)logits & 3) || ((uintptr_t)loss & 3) || ((uintptr_t)labels & 7)) return PPT_EINVAL;
    hipLaunchKernelGGL(train_meter_cls_kernel, dim3(1), dim3(MT_THREADS), 0, ppt_stream(stream), logits, labels, loss, B, C, weight,
                       metered ? 1 : 0, rec);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

static int train_meter_partseg_launch(const float *logits, const int64_t *labels, const int32_t *lengths, const float *loss, int B, int N,
                                      int P, const int32_t *part_start, const int32_t *part_count, double weight, int metered,
                                      double *rec, uint32_t *scratch, void *stream)
{
    if (!logits || !labels || !loss || !part_start || !part_count || !rec || !scratch || B <= 0 || N <= 0 || P <= 0) return PPT_EINVAL;
    if (((uintptr_t)rec & 7) || ((uintptr_t)logits & 3) || ((uintptr_t)loss & 3) || ((uintptr_t)labels & 7) || ((uintptr_t)scratch & 3))
        return PPT_EINVAL;
    if (P > 64) return PPT_EUNSUPPORTED;
    const int chunks = (N + MT_CHUNK - 1) / MT_CHUNK;
    if ((int64_t)B * chunks > 0x7fffffffLL || (int64_t)B * N > 0x7fffffffLL) return PPT_EINVAL;
    if (lengths)
        hipLaunchKernelGGL(train_meter_partseg_kernel<true>, dim3((unsigned)(B * chunks)), dim3(MT_THREADS), 0, ppt_stream(stream), logits,
                           labels, loss, B, N, P, chunks, part_start, part_count, weight, metered ? 1 : 0, rec, (unsigned *)scratch, lengths);
    else
        hipLaunchKernelGGL(train_meter_partseg_kernel<false>, dim3((unsigned)(B * chunks)), dim3(MT_THREADS), 0, ppt_stream(stream), logits,
                           labels, loss, B, N, P, chunks, part_start, part_count, weight, metered ? 1 : 0, rec, (unsigned *)scratch, lengths);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" int ppt_train_meter_partseg(const float *logits, const int64_t *labels, const float *loss, int B, int N, int P,
                                       const int32_t *part_start, const int32_t *part_count, double weight, int metered, double *rec,
                                       uint32_t *scratch, void *stream)
{
    return train_meter_partseg_launch(logits, labels, nullptr, loss, B, N, P, part_start, part_count, weight, metered, rec, scratch, stream);
}

extern "C" int ppt_train_meter_partseg_ragged(const float *logits, const int64_t *labels, const int32_t *lengths, const float *loss, int B,
                                              int Nmax, int P, const int32_t *part_start, const int32_t *part_count, double weight,
                                              int metered, double *rec, uint32_t *scratch, void *stream)
{
    if (!lengths) return PPT_EINVAL;
    return train_meter_partseg_launch(logits, labels, lengths, loss, B, Nmax, P, part_start, part_count, weight, metered, rec, scratch,
                                      stream);
}
