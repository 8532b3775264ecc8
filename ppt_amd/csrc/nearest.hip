// nearest.hip -- the k nearest rows of a table for each of a few query rows, for gfx950: what interpret_prompt.py:34-37 asks of
// torch.cdist + argsort over the 49408 x 512 token-embedding table (Q = 32 prompt tokens, k = 10 words each).
//
// The distance is the DIRECT form sqrt(sum_j (q_j - t_j)^2), one fp32 subtraction and one FMA per term, summed over the columns in
// order: a query that is a copy of a table row is at distance exactly 0 (cdist's |q|^2 + |t|^2 - 2 q.t is not).  The order is one
// integer minimum over 64-bit keys, (bits of d^2) << 32 | row: d^2 >= +0, so its bit pattern is monotone, ties go to the lower row,
// and a NaN (bits above +inf's as an unsigned number) never precedes a finite distance.  No atomics; every sum and every minimum
// has a fixed order, so two runs write identical bytes.  No [Q, V] matrix leaves the chip.
//
// Pass 1, nearest_slice_kernel: one workgroup of 512 threads per SLICE of 256 table rows.
//   mapping   lane = table row.  Wave w works on the HALF w / 4 of the slice (128 rows: a lane owns the rows lane and lane + 64 of
//             it) and on a GROUP of 8 queries (the groups w % 4, w % 4 + 4, ...): 2 x 8 = 16 accumulators per lane, no cross-lane
//             reduction.  Over the whole table that is V Q / 16 lanes: 193 workgroups of 8 waves at the real shape, one per CU and
//             two waves per SIMD -- a SIMD issues a wave64 VALU instruction every 2 cycles, one wave alone only every 4 (measured
//             with 4 rows per lane and one wave per SIMD: 111 us for this pass, twice its VALU time).
//   queries   all Q of them in LDS (Q D floats <= 128 KiB), group-major and column-major inside a group ([group][column][8]; the
//             last group [column][Q % 8] without padding): the 8 query values of a column are two ds_read_b128 at a wave-uniform
//             address (a broadcast), and feed 2 rows x 8 queries = 32 VALU operations.
//   table     the slice is staged 16 columns at a time: 256 rows x 64 B, one 16-byte load per thread and row quarter (2 loads in
//             flight per thread, issued one chunk AHEAD into registers and written to LDS after the current chunk's arithmetic),
//             row stride 20 dwords, so that the lane = row ds_read_b128 of 16 consecutive rows touch 16 different bank quads.
//             Every table byte is loaded once per pass over the query groups: once in all for Q <= 32.  (A ring of 4 chunks in
//             registers behind LDS-only barriers was measured too: 87 us against 86 us, so the loads are hidden as it is.)
//   selection each wave extracts, for each of its queries, the k smallest keys of its 128 rows in ascending order: k rounds of
//             "smallest key above the previous one" (keys are unique), a lane minimum over its 2 rows and two 32-bit DPP minima
//             over the wave.  Rows past V give the key ~0, which also fills the list of a half with fewer than k rows.
//   budget    LDS 4 Q D + 20 480 B (151 552 B at the limit Q D = 32 768: one workgroup per CU at any shape above Q D = 15 360);
//             16 accumulators + 8 staged table values + 8 in flight + 8 query values per lane; the compiler takes 114 VGPRs, of
//             the 256 that two waves per SIMD leave each.
// Pass 2, nearest_merge_kernel: one workgroup per query merges the lists of all halves the same way -- up to 4096 keys are held in
//   registers (3860 at the real shape), more are re-read from the workspace in every round -- and writes idx and dist = sqrtf(d^2).
// Plain scalar fp32 arithmetic on purpose: no packed-fp32 forms (see build.py on -fno-slp-vectorize).
#include <cmath>

#include "ppt_common.h"

namespace {

constexpr int NR_T = 512;                        // threads per workgroup of pass 1
constexpr int NR_R = 2;                          // table rows per lane
constexpr int NR_HALF = 64 * NR_R;               // rows per list (one wave's rows)
constexpr int NR_ROWS = 2 * NR_HALF;             // rows per slice (workgroup)
constexpr int NR_QWAVES = NR_T / 64 / 2;         // waves per half = query groups per pass
constexpr int NR_G = 8;                          // queries per group
constexpr int NR_CC = 16;                        // columns per staged chunk
constexpr int NR_LD = NR_CC + 4;                 // tile row stride in dwords
constexpr int NR_TILE_BYTES = NR_ROWS * NR_LD * 4;
constexpr int NR_PIECES = NR_ROWS * (NR_CC / 4) / NR_T;          // 16-byte pieces of a chunk per thread
constexpr int NR_LDS_MAX = 160 * 1024;
constexpr int NR_QD_MAX = 32768;
constexpr int NR_K_MAX = 64;
constexpr int NR_MT = 256;                       // threads per workgroup of pass 2
constexpr int NR_MKEYS = 16;                     // keys per thread it holds in registers
constexpr uint64_t NR_NOKEY = ~0ull;

bool nr_supported(int Q, int V, int D, int k)
{
    return Q >= 1 && D >= 4 && D % 4 == 0 && (int64_t)Q * D <= NR_QD_MAX && k >= 1 && k <= NR_K_MAX && k <= V;
}

inline int nr_slices(int V) { return (V + NR_ROWS - 1) / NR_ROWS; }
inline int nr_lists(int V) { return (V + NR_HALF - 1) / NR_HALF; }

// the smallest 64-bit key of the wave, in every lane: the minimum of the high words, then of the low words that go with it
__device__ __forceinline__ uint64_t wave_min_key(uint64_t key)
{
    const uint32_t hi = wave_reduce_umin((uint32_t)(key >> 32));
    const uint32_t lo = wave_reduce_umin((uint32_t)(key >> 32) == hi ? (uint32_t)key : 0xffffffffu);
    return ((uint64_t)hi << 32) | lo;
}

// the 16-byte pieces of the chunk [c0, c0 + 16) of the slice's rows that this thread stages: piece i = t + 512 m is columns
// 4 (i % 4) .. + 3 of row i / 4.  Rows past V repeat row V - 1 and columns past D read as zero: nothing out of bounds.
__device__ __forceinline__ void load_chunk(float4 (&v)[NR_PIECES], const float *__restrict__ table, int64_t ld, int V, int D, int row0,
                                           int c0, int t)
{
#pragma unroll
    for (int m = 0; m < NR_PIECES; ++m) {
        const int i = t + NR_T * m, c = c0 + 4 * (i & 3);
        int row = row0 + (i >> 2);
        row = row < V ? row : V - 1;
        v[m] = c < D ? *reinterpret_cast<const float4 *>(table + (size_t)row * ld + c) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

__device__ __forceinline__ void store_chunk(const float4 (&v)[NR_PIECES], float *tile, int t)
{
#pragma unroll
    for (int m = 0; m < NR_PIECES; ++m) {
        const int i = t + NR_T * m;
        *reinterpret_cast<float4 *>(tile + (i >> 2) * NR_LD + 4 * (i & 3)) = v[m];
    }
}

// acc[r][e] += (t[r] - q[e])^2 for the cc columns of the staged chunk; rows: the lane's first row in the tile; qg: the group's
// values of the chunk's first column.  FULL: a group of 8 (two 16-byte reads per column); otherwise w < 8 values per column, read
// one by one, the rest zero.
template <bool FULL>
__device__ __forceinline__ void chunk_terms(float (&acc)[NR_R][NR_G], const float *rows, const float *qg, int w, int cc)
{
    for (int j = 0; j < cc; j += 4) {
        float tv[NR_R][4];
#pragma unroll
        for (int r = 0; r < NR_R; ++r) {
            const float4 x = *reinterpret_cast<const float4 *>(rows + 64 * r * NR_LD + j);
            tv[r][0] = x.x; tv[r][1] = x.y; tv[r][2] = x.z; tv[r][3] = x.w;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float qv[NR_G];
            if constexpr (FULL) {
                const float4 a = *reinterpret_cast<const float4 *>(qg + (j + c) * NR_G);
                const float4 b = *reinterpret_cast<const float4 *>(qg + (j + c) * NR_G + 4);
                qv[0] = a.x; qv[1] = a.y; qv[2] = a.z; qv[3] = a.w; qv[4] = b.x; qv[5] = b.y; qv[6] = b.z; qv[7] = b.w;
            } else {
#pragma unroll
                for (int e = 0; e < NR_G; ++e) qv[e] = e < w ? qg[(j + c) * w + e] : 0.0f;
            }
#pragma unroll
            for (int r = 0; r < NR_R; ++r)
#pragma unroll
                for (int e = 0; e < NR_G; ++e) {
                    const float d = tv[r][c] - qv[e];
                    acc[r][e] = fmaf(d, d, acc[r][e]);
                }
        }
    }
}

__global__ __launch_bounds__(NR_T) void nearest_slice_kernel(const float *__restrict__ q, int Q, const float *__restrict__ table,
                                                             int64_t ld, int V, int D, int k, int lists_n,
                                                             uint64_t *__restrict__ lists)
{
    extern __shared__ __align__(16) unsigned char smem[];
    float *tile = reinterpret_cast<float *>(smem);
    float *qs = reinterpret_cast<float *>(smem + NR_TILE_BYTES);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int half = wave / NR_QWAVES, qwave = wave % NR_QWAVES;
    const int row0 = blockIdx.x * NR_ROWS;
    const int list = blockIdx.x * 2 + half;                       // (wave-uniform; past lists_n: a half that lies beyond the table)
    const int groups = (Q + NR_G - 1) / NR_G;

    // the queries, [group][column][width of the group]: four at a time, so that four loads are in flight per thread
    for (int q0 = 0; q0 < Q; q0 += 4)
        for (int c = t; c < D; c += NR_T) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = q0 + u < Q ? q[(size_t)(q0 + u) * D + c] : 0.0f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int qi = q0 + u, g = qi / NR_G;
                const int w = Q - g * NR_G < NR_G ? Q - g * NR_G : NR_G;
                if (qi < Q) qs[g * NR_G * D + c * w + (qi - g * NR_G)] = v[u];
            }
        }

    for (int g0 = 0; g0 < groups; g0 += NR_QWAVES) {
        const int g = g0 + qwave;
        const bool active = g < groups && list < lists_n;         // (wave-uniform)
        const int w = active ? (Q - g * NR_G < NR_G ? Q - g * NR_G : NR_G) : 0;
        const float *qg = qs + (active ? g : 0) * NR_G * D;
        const float *rows = tile + (half * NR_HALF + lane) * NR_LD;
        float acc[NR_R][NR_G];
#pragma unroll
        for (int r = 0; r < NR_R; ++r)
#pragma unroll
            for (int e = 0; e < NR_G; ++e) acc[r][e] = 0.0f;

        float4 stage[NR_PIECES];
        load_chunk(stage, table, ld, V, D, row0, 0, t);
        for (int c0 = 0; c0 < D; c0 += NR_CC) {
            __syncthreads();                                      // the previous chunk has been read (first time: qs is written)
            store_chunk(stage, tile, t);
            __syncthreads();
            if (c0 + NR_CC < D) load_chunk(stage, table, ld, V, D, row0, c0 + NR_CC, t);
            const int cc = D - c0 < NR_CC ? D - c0 : NR_CC;
            if (active) {
                if (w == NR_G) chunk_terms<true>(acc, rows, qg + c0 * NR_G, w, cc);
                else chunk_terms<false>(acc, rows, qg + c0 * w, w, cc);
            }
        }

        // the k smallest keys of the half for each query of the group, ascending
        if (active) {
#pragma unroll
            for (int e = 0; e < NR_G; ++e) {
                if (e >= w) continue;                             // (wave-uniform)
                uint64_t key[NR_R];
#pragma unroll
                for (int r = 0; r < NR_R; ++r) {
                    const int row = row0 + half * NR_HALF + lane + 64 * r;
                    key[r] = row < V ? ((uint64_t)__float_as_uint(acc[r][e]) << 32) | (uint32_t)row : NR_NOKEY;
                }
                uint64_t *out = lists + ((size_t)list * Q + (g * NR_G + e)) * k;
                uint64_t prev = 0;
                for (int j = 0; j < k; ++j) {
                    uint64_t m = NR_NOKEY;
#pragma unroll
                    for (int r = 0; r < NR_R; ++r)
                        if ((j == 0 || key[r] > prev) && key[r] < m) m = key[r];
                    prev = wave_min_key(m);
                    if (lane == 0) out[j] = prev;
                }
            }
        }
    }
}

// one workgroup per query: the k smallest of the n = lists_n * k keys of its lists, ascending.  The first 4096 keys live in
// registers (key i with thread i % 256), the others are re-read in every round.
__global__ __launch_bounds__(NR_MT) void nearest_merge_kernel(const uint64_t *__restrict__ lists, int lists_n, int Q, int k,
                                                              int32_t *__restrict__ idx, float *__restrict__ dist)
{
    __shared__ uint64_t part[NR_MT / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int qi = blockIdx.x;
    const int64_t n = (int64_t)lists_n * k;
    auto key_at = [&](int64_t i) {
        const int64_t s = i / k;
        return lists[((size_t)s * Q + qi) * k + (i - s * k)];
    };
    uint64_t held[NR_MKEYS];
#pragma unroll
    for (int u = 0; u < NR_MKEYS; ++u) {
        const int64_t i = t + (int64_t)NR_MT * u;
        held[u] = i < n ? key_at(i) : NR_NOKEY;
    }
    uint64_t prev = 0;
    for (int j = 0; j < k; ++j) {
        uint64_t m = NR_NOKEY;
#pragma unroll
        for (int u = 0; u < NR_MKEYS; ++u)
            if ((j == 0 || held[u] > prev) && held[u] < m) m = held[u];
        for (int64_t i = t + (int64_t)NR_MT * NR_MKEYS; i < n; i += NR_MT) {
            const uint64_t key = key_at(i);
            if ((j == 0 || key > prev) && key < m) m = key;
        }
        m = wave_min_key(m);
        __syncthreads();                                          // the previous round's partials have been read
        if (lane == 0) part[wave] = m;
        __syncthreads();
#pragma unroll
        for (int x = 0; x < NR_MT / 64; ++x) m = part[x] < m ? part[x] : m;
        prev = m;
        if (t == 0) {
            const bool found = m != NR_NOKEY;                     // (k <= V: always)
            idx[(size_t)qi * k + j] = found ? (int32_t)(uint32_t)m : -1;
            dist[(size_t)qi * k + j] = found ? sqrtf(__uint_as_float((uint32_t)(m >> 32))) : NAN;
        }
    }
}

}  // namespace

extern "C" size_t ppt_nearest_rows_workspace_bytes(int Q, int V, int D, int k)
{
    if (!nr_supported(Q, V, D, k)) return 0;
    return (size_t)nr_lists(V) * Q * k * sizeof(uint64_t);
}

extern "C" int ppt_nearest_rows_f32(const float *q, int Q, const float *table, int64_t ld, int V, int D, int k, int32_t *idx,
                                    float *dist, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!q || !table || !idx || !dist || !workspace) return PPT_EINVAL;
    if (Q <= 0 || V <= 0 || D <= 0 || k <= 0 || ld < D) return PPT_EINVAL;
    if (!nr_supported(Q, V, D, k)) return PPT_EUNSUPPORTED;
    if ((ld & 3) || ((uintptr_t)table & 15) || ((uintptr_t)workspace & 255)) return PPT_EINVAL;          // 16-byte row loads
    if (workspace_bytes < ppt_nearest_rows_workspace_bytes(Q, V, D, k)) return PPT_EINVAL;
    hipStream_t s = ppt_stream(stream);
    const int lists_n = nr_lists(V);
    const size_t lds = NR_TILE_BYTES + (size_t)Q * D * sizeof(float);
    uint64_t *lists = static_cast<uint64_t *>(workspace);
    PPT_RAISE_LDS_ONCE(NR_LDS_MAX, (const void *)nearest_slice_kernel);
    hipLaunchKernelGGL(nearest_slice_kernel, dim3(nr_slices(V)), dim3(NR_T), lds, s, q, Q, table, ld, V, D, k, lists_n, lists);
    PPT_CHECK_LAUNCH();
    hipLaunchKernelGGL(nearest_merge_kernel, dim3(Q), dim3(NR_MT), 0, s, lists, lists_n, Q, k, idx, dist);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}
