// metrics.hip -- validate()'s bookkeeping on the device (ppt_amd/evaluate.py): what main_cls.py:266-284 and main_partseg.py:295-344
// take out of a batch of logits with host loops and .item() calls, as ONE launch per batch that writes a small record per sample.
// The host reads the records once, at the end of the epoch, and repeats the reference's final arithmetic on the integers.
//
//   cls_metrics_kernel      one wave per row of logits [B, C]: a row of 40 classes is less than one wave-wide load, so the lanes
//                           share the row (coalesced dword loads), butterfly reductions, lane 0 writes the 16-byte record.
//   partseg_metrics_kernel  one workgroup per chunk of PS_CHUNK points of one cloud.  A row of P = 50 classes is 200 bytes: the
//                           workgroup stages PS_TILE rows at a time through LDS with 16-byte coalesced loads (the tile is one
//                           contiguous span of global memory) and an ODD row stride in LDS, then lane = point.  Histograms per wave
//                           with ballots and popcounts, waves combined in LDS, chunks combined with integer atomics (order-
//                           independent); the loss through one fp32 partial per chunk that the LAST workgroup of the cloud to
//                           arrive folds in chunk order -- every byte of the record is the same on every run.
// Sums run in double and are rounded to fp32 once: cheaper than arguing about the error of 2048 fp32 additions.
#include "ppt_common.h"
#include <math.h>

#define PS_TILE 128                        // rows staged per pass == threads per workgroup
#define PS_CHUNK 256                       // points of one cloud per workgroup
#define PS_WAVES (PS_TILE / PPT_WAVE)
#define PS_SLOTS (3 * PPT_PARTSEG_MAX_PARTS + 2)          // per-wave: 3 counts per part slot, correct points, flag bits

__device__ __forceinline__ bool met_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ double met_wave_sum(double v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;                                              // the butterfly adds mirror images: every lane holds the same bits
}
__device__ __forceinline__ float met_wave_max(float v)
{
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// (1 - s)(lse - x_t) + s (lse - mean_c x_c): nn.CrossEntropyLoss(label_smoothing = s) of one row, before the mean over rows
__device__ __forceinline__ double met_row_loss(float m, double sumexp, double sumx, float xt, int C, float smoothing)
{
    const double lse = (double)m + log(sumexp);
    const double s = (double)smoothing;
    return (1.0 - s) * (lse - (double)xt) + s * (lse - sumx / (double)C);
}

__global__ __launch_bounds__(256) void cls_metrics_kernel(const float *__restrict__ logits, const int64_t *__restrict__ labels,
                                                          float smoothing, int B, int C, int32_t *__restrict__ records)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;                                  // wave-uniform
    const float *x = logits + (size_t)row * C;
    const int64_t t64 = labels[row];
    const bool bad = t64 < 0 || t64 >= (int64_t)C;
    const int t = bad ? 0 : (int)t64;
    const float xt = x[t];
    float m = -INFINITY;
    double sumx = 0.0;
    int rank = 0, nonfinite = 0;
    for (int c = lane; c < C; c += PPT_WAVE) {
        const float v = x[c];
        m = fmaxf(m, v);
        sumx += (double)v;
        nonfinite |= met_nonfinite(v) ? 1 : 0;
        rank += (v > xt || (v == xt && c < t)) ? 1 : 0;
    }
    m = met_wave_max(m);
    double sumexp = 0.0;
    for (int c = lane; c < C; c += PPT_WAVE) sumexp += (double)expf(x[c] - m);      // (the row is in L1 from the first pass)
    sumexp = met_wave_sum(sumexp);
    sumx = met_wave_sum(sumx);
    for (int o = 32; o; o >>= 1) rank += __shfl_xor(rank, o);
    const bool any_nonfinite = __builtin_amdgcn_ballot_w64(nonfinite != 0) != 0;
    if (lane == 0) {
        const float loss = bad ? 0.0f : (float)met_row_loss(m, sumexp, sumx, xt, C, smoothing);
        int4 r;
        r.x = (int)__float_as_uint(loss);
        r.y = bad ? C : rank;
        r.z = (any_nonfinite ? (int)PPT_METRIC_NONFINITE : 0) | (bad ? (int)PPT_METRIC_BAD_LABEL : 0);
        r.w = bad ? -1 : t;
        *reinterpret_cast<int4 *>(records + (size_t)row * PPT_CLS_REC) = r;
    }
}

// RAGGED (ppt_partseg_metrics_ragged): N is the row stride of the slabs and cloud b its first lengths[b] rows; the chunks are cut
// for N, a chunk wholly behind the cloud's end counts nothing (its loss partial is 0) but still draws its ticket.  Everything the
// kernel takes from a row -- label, logits -- it takes from rows < lengths[b] only (the 16-byte staging loads may touch up to three
// floats of the next row inside the same allocation; they are dropped unlooked-at, as at a cloud boundary of the uniform form).
// A compile-time flag, lengths the last argument: the uniform instantiation is the kernel it was.
template <bool RAGGED>
__global__ __launch_bounds__(PS_TILE) void partseg_metrics_kernel(const float *__restrict__ logits, const int64_t *__restrict__ labels,
                                                                  float smoothing, int N, int P, size_t total, int chunks,
                                                                  const int32_t *__restrict__ part_start,
                                                                  const int32_t *__restrict__ part_count, int32_t *records,
                                                                  float *partial, const int32_t *__restrict__ lengths)
{
    __shared__ float tile[PS_TILE * (64 + 1) + 4];
    __shared__ int wave_counts[PS_WAVES][PS_SLOTS];
    __shared__ double wave_loss[PS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    int n_rows = N;
    if constexpr (RAGGED) n_rows = max(1, min((int)lengths[b], N));      // (clamped: a bad length must not leave the slab)
    const int n0 = chunk * PS_CHUNK, n1 = min(n_rows, n0 + PS_CHUNK);
    const int64_t *lab = labels + (size_t)b * N;
    int32_t *rec = records + (size_t)b * PPT_PARTSEG_REC;

    // the cloud's category is the one point 0's label belongs to (main_partseg.py:302, :326).  The tables are device memory the
    // host entry cannot look into: clamp what they say so that no index below can leave the row.
    const int64_t l0 = lab[0];
    const bool bad_cat = l0 < 0 || l0 >= (int64_t)P;
    int start = bad_cat ? 0 : part_start[l0];
    int count = bad_cat ? 0 : part_count[l0];
    start = max(0, min(start, P));
    count = max(0, min(count, min(PPT_PARTSEG_MAX_PARTS, P - start)));

    const int stride = P | 1;                              // odd: lanes that walk their rows in step hit 64 different banks
    int c_gt[PPT_PARTSEG_MAX_PARTS], c_pred[PPT_PARTSEG_MAX_PARTS], c_both[PPT_PARTSEG_MAX_PARTS];
#pragma unroll
    for (int j = 0; j < PPT_PARTSEG_MAX_PARTS; j++) c_gt[j] = c_pred[j] = c_both[j] = 0;
    int correct = 0, flags = bad_cat ? (int)PPT_METRIC_BAD_LABEL : 0;
    double loss = 0.0;

    for (int p0 = n0; p0 < n1; p0 += PS_TILE) {
        const int rows = min(PS_TILE, n1 - p0);
        // ---- stage rows [p0, p0 + rows) of cloud b: ONE contiguous span of floats, read as aligned float4 ------------------
        const size_t first = ((size_t)b * N + p0) * P;
        const int shift = (int)(first & 3);
        const size_t first4 = first - shift;
        const int nflt = rows * P;
        const int nquad = (shift + nflt + 3) >> 2;
        for (int q = tid; q < nquad; q += PS_TILE) {
            const size_t g = first4 + 4 * (size_t)q;
            float v[4];
            if (g + 3 < total) {
                const float4 f = *reinterpret_cast<const float4 *>(logits + g);
                v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) v[k] = g + k < total ? logits[g + k] : 0.0f;
            }
            const int e = 4 * q - shift;                   // index of v[0] in the tile (negative only in the first quad)
            int r = e > 0 ? e / P : 0;
            int c = e - r * P;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                while (c >= P) { c -= P; r++; }
                if (e + k >= 0 && e + k < nflt) tile[r * stride + c] = v[k];
                c++;
            }
        }
        __syncthreads();
        // ---- lane = point -------------------------------------------------------------------------------------------------
        const bool valid = tid < rows;
        int lbl = -1, pred = -2;
        if (valid) {
            const int64_t l64 = lab[p0 + tid];
            const bool bad = l64 < 0 || l64 >= (int64_t)P;
            lbl = bad ? -1 : (int)l64;
            const float *x = tile + tid * stride;
            float m = -INFINITY;
            double sumx = 0.0;
            int nonfinite = 0;
            for (int c = 0; c < P; c++) {
                const float v = x[c];
                m = fmaxf(m, v);
                sumx += (double)v;
                nonfinite |= met_nonfinite(v) ? 1 : 0;
            }
            double sumexp = 0.0;
            for (int c = 0; c < P; c++) sumexp += (double)expf(x[c] - m);
            if (count > 0) {                               // arg-max over the category's range only, the first maximum wins
                float best = x[start];
                pred = start;
                for (int c = start + 1; c < start + count; c++) {
                    const float v = x[c];
                    if (v > best) { best = v; pred = c; }
                }
            }
            if (!bad) loss += met_row_loss(m, sumexp, sumx, x[lbl], P, smoothing);
            flags |= (nonfinite ? (int)PPT_METRIC_NONFINITE : 0) | (bad ? (int)PPT_METRIC_BAD_LABEL : 0);
        }
        // ---- histograms: a ballot per part slot, a popcount per ballot (wave-uniform counts) --------------------------------
#pragma unroll
        for (int j = 0; j < PPT_PARTSEG_MAX_PARTS; j++) {
            if (j < count) {
                const bool g = valid && lbl == start + j, p = valid && pred == start + j;
                c_gt[j] += __popcll(__builtin_amdgcn_ballot_w64(g));
                c_pred[j] += __popcll(__builtin_amdgcn_ballot_w64(p));
                c_both[j] += __popcll(__builtin_amdgcn_ballot_w64(g && p));
            }
        }
        correct += __popcll(__builtin_amdgcn_ballot_w64(valid && pred == lbl));
        __syncthreads();                                   // the tile is rewritten by the next pass
    }

    // ---- waves -> LDS -> the cloud's record ------------------------------------------------------------------------------------
    loss = met_wave_sum(loss);
    const unsigned long long m1 = __builtin_amdgcn_ballot_w64((flags & (int)PPT_METRIC_NONFINITE) != 0);
    const unsigned long long m2 = __builtin_amdgcn_ballot_w64((flags & (int)PPT_METRIC_BAD_LABEL) != 0);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < PPT_PARTSEG_MAX_PARTS; j++) {
            wave_counts[wave][3 * j + 0] = c_gt[j];
            wave_counts[wave][3 * j + 1] = c_pred[j];
            wave_counts[wave][3 * j + 2] = c_both[j];
        }
        wave_counts[wave][3 * PPT_PARTSEG_MAX_PARTS] = correct;
        wave_counts[wave][3 * PPT_PARTSEG_MAX_PARTS + 1] = (m1 ? (int)PPT_METRIC_NONFINITE : 0) | (m2 ? (int)PPT_METRIC_BAD_LABEL : 0);
        wave_loss[wave] = loss;
    }
    __syncthreads();
    if (tid < PS_SLOTS) {
        int v = 0;
        if (tid == PS_SLOTS - 1) {
            for (int w = 0; w < PS_WAVES; w++) v |= wave_counts[w][tid];
            if (v) atomicOr(rec + 3, v);
        } else {
            for (int w = 0; w < PS_WAVES; w++) v += wave_counts[w][tid];
            if (v) atomicAdd(tid == PS_SLOTS - 2 ? rec + 2 : rec + 8 + tid, v);
        }
    }
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < PS_WAVES; w++) s += wave_loss[w];
        __hip_atomic_store(partial + (size_t)b * chunks + chunk, (float)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (chunk == 0) { rec[0] = start; rec[1] = count; }
    }
    // ---- the last workgroup of the cloud to get here folds the chunks' loss partials, in chunk order --------------------------
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        const unsigned ticket = atomicAdd(reinterpret_cast<unsigned *>(rec + 5), 1u);
        if (ticket == (unsigned)chunks - 1u) {
            __threadfence();
            double s = 0.0;
            for (int c = 0; c < chunks; c++)
                s += (double)__hip_atomic_load(partial + (size_t)b * chunks + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            rec[4] = (int)__float_as_uint((float)s);
            // the record of the cloud alone: the chunks ITS rows fill (the counter above has counted the launch's)
            if constexpr (RAGGED) rec[5] = (n_rows + PS_CHUNK - 1) / PS_CHUNK;
        }
    }
}

extern "C" int ppt_cls_metrics(const float *logits, const int64_t *labels, float smoothing, int B, int C, int32_t *records, void *stream)
{
    if (!logits || !labels || !records || B <= 0 || C <= 0) return PPT_EINVAL;
    if (((uintptr_t)records & 15) || ((uintptr_t)logits & 3)) return PPT_EINVAL;
    hipLaunchKernelGGL(cls_metrics_kernel, dim3((B + 3) / 4), dim3(256), 0, ppt_stream(stream), logits, labels, smoothing, B, C, records);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" int ppt_partseg_metrics_chunks(int N) { return N <= 0 ? 0 : (N + PS_CHUNK - 1) / PS_CHUNK; }

static int partseg_metrics_launch(const float *logits, const int64_t *labels, const int32_t *lengths, float smoothing, int B, int N,
                                  int P, const int32_t *part_start, const int32_t *part_count, int max_parts, int32_t *records,
                                  float *partial, void *stream)
{
    if (!logits || !labels || !part_start || !part_count || !records || !partial || B <= 0 || N <= 0 || P <= 0 || max_parts <= 0)
        return PPT_EINVAL;
    if (((uintptr_t)logits & 15) || ((uintptr_t)records & 3)) return PPT_EINVAL;
    if (P > 64 || max_parts > PPT_PARTSEG_MAX_PARTS) return PPT_EUNSUPPORTED;
    const int chunks = ppt_partseg_metrics_chunks(N);
    if ((int64_t)B * chunks > 0x7fffffffLL) return PPT_EINVAL;
    // the chunks of a cloud ADD into its record, and its arrival counter starts at zero
    if (hipMemsetAsync(records, 0, sizeof(int32_t) * PPT_PARTSEG_REC * (size_t)B, ppt_stream(stream)) != hipSuccess) return PPT_ELAUNCH;
    if (lengths)
        hipLaunchKernelGGL(partseg_metrics_kernel<true>, dim3((unsigned)(B * chunks)), dim3(PS_TILE), 0, ppt_stream(stream), logits,
                           labels, smoothing, N, P, (size_t)B * N * P, chunks, part_start, part_count, records, partial, lengths);
    else
        hipLaunchKernelGGL(partseg_metrics_kernel<false>, dim3((unsigned)(B * chunks)), dim3(PS_TILE), 0, ppt_stream(stream), logits,
                           labels, smoothing, N, P, (size_t)B * N * P, chunks, part_start, part_count, records, partial, lengths);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

extern "C" int ppt_partseg_metrics(const float *logits, const int64_t *labels, float smoothing, int B, int N, int P,
                                   const int32_t *part_start, const int32_t *part_count, int max_parts, int32_t *records,
                                   float *partial, void *stream)
{
    return partseg_metrics_launch(logits, labels, nullptr, smoothing, B, N, P, part_start, part_count, max_parts, records, partial, stream);
}

extern "C" int ppt_partseg_metrics_ragged(const float *logits, const int64_t *labels, const int32_t *lengths, float smoothing, int B,
                                          int Nmax, int P, const int32_t *part_start, const int32_t *part_count, int max_parts,
                                          int32_t *records, float *partial, void *stream)
{
    if (!lengths) return PPT_EINVAL;
    return partseg_metrics_launch(logits, labels, lengths, smoothing, B, Nmax, P, part_start, part_count, max_parts, records, partial,
                                  stream);
}
