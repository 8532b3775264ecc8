// group_lds.h -- the LDS-staged group kernel: out = epilogue( prologue(A) . W^T ) with A [32 n_tiles, K] 16-bit read ONCE from HBM
// and W [256 TJ, K] never moving.  A workgroup is 8 waves; wave w keeps columns 32 TJ w .. 32 TJ (w + 1) - 1 of W in 8 TJ K / 32 VGPRs
// for the whole kernel (128 in both instantiated shapes).  One group of 32 points is one MFMA row tile of 64 K bytes; every wave
// reads its A fragments from an LDS image of it (row pitch 2 K + 16 B: the 16 lanes of a ds_read_b128 phase hit 64 distinct banks).
// Persistent grid: workgroup b takes groups b, b + grid, ...  Same expressions and k order as ppt_gemm's path for the same
// product: results are bit-identical to it.
//   prologue  AFFINE: a = relu(a_scale[k] * a + a_shift[k]) (affine_relu_chunk16), else the rows as they are
//   epilogue  GL_POOL:  out[g, n] = max over the group's rows of (acc + add[n])   (`add` = the bias [N], may be null)
//             otherwise v = acc + add[g, n] (`add` = the per-group term [n_tiles, N]), then
//             GL_STATS: BatchNorm partials of v per group (PPT_GT_CHUNK_STATS) and / or GL_STORE: out[32 g + r, n] = v, through a
//             wave-private LDS transpose (8 tiles behind the A ring) as 64 TJ-byte row pieces.
// THE LOOP.  The images form a ring of NB = DIST + 1 slots, filled by LDS-DMA (lds_dma16: no register in between, so nothing the
// compiler could sink below the MFMAs): wave w requests rows w, w + 8, w + 16, w + 24 of a group, one piece of K / 8 lanes per row
// -- the PADDED pitch is kept (a piece never spans rows, as in mlp_fused3's image) rather than unpadded rows with a source-side
// XOR swizzle: the fragment reads, their addresses and their bank pattern are then the ones the kernel always had, and the price
// is four half-wave pieces instead of two whole ones per wave and group at K = 256.  While group `it` computes, the requests of
// groups it + 1 .. it + DIST are in flight (DIST 16 KB images at K = 256, DIST 32 KB images at K = 512).  The group term travels
// the same way: the wave's 32 TJ columns of `add[g, :]` are a fifth piece (TERM bytes, TERM / 16 lanes) into a wave-private
// slot of a second ring, requested with the group's rows and read back by the lanes in the epilogue.  (Held in registers
// one group ahead, the copy of the next term into the current one's registers at the loop's end made hipcc wait for everything
// the iteration had requested.)  Per group, in program order:
//     requests of group it + DIST (rows, term)  |  fragment reads + MFMAs of group it  |  epilogue, stores
//     |  s_waitcnt vmcnt(WAIT): this wave's pieces of group it + 1 have landed -- everything younger (the pieces of the groups
//        behind it, every store since) stays in flight; vmcnt retires in order
//     |  AFFINE: the wave passes over ITS OWN four rows of group it + 1 in place (a lane reads back the 16 bytes it requested:
//        the issuing wave's vmcnt orders that; each element meets affine_relu_chunk16 once)
//     |  lds_barrier(): ONE workgroup barrier per group, LDS only.  It hands image it + 1 to every wave, and it frees slot `it`,
//        which the next iteration's requests (group it + 1 + DIST) overwrite.
// __syncthreads() in place of that barrier is what drained the queue before: its workgroup-scope release waits for every store
// of the wave (s_waitcnt vmcnt(0) in front of the next group's first MFMA), and with an LDS-DMA pending it waits for that too.
// The loads the compiler knows (weights, prologue constants, bias) are waited for ONCE, with the first DIST images, by
// an s_waitcnt builtin in front of the loop: left to the compiler, the wait for the weights stands in front of the loop's first
// MFMA, where it would drain the ring in every iteration.  The prefetch index is clamped to the last group, so every iteration
// issues the same requests (the counts above are static); the clamped images land in slots nobody reads and are waited for at the end.
// MEASURED (profiles/r24_group_lds_pipeline.md; alone, 16 384 groups): with the ring the loop holds no wait for HBM any more, and
// the kernels gained 3-8 %, not the 30 % a latency-bound loop would have: conv3 231 -> 222 us (3.6 TB/s), its statistics pass 167
// -> 155 us, conv4 162.5 -> 158 us (3.4 TB/s), against 6.0 TB/s of a plain sweep and an MFMA floor of 55 us.  Neither HBM nor
// the matrix pipe bounds them: the rest is the chip-side work of a group between two barriers.  One workgroup per CU is all that
// fits (176-224 VGPRs: two waves per SIMD; 98-110 KB of LDS).  INSIDE the C2 step, beside the other stream's kernels and on the
// tower's share of the CUs, requests take longer and the ring is worth more: conv3 279 -> 215 us, conv4 188 -> 168 us per launch
// (rocprofv3), the step 2.564 -> 2.498 ms, C3 5.535 -> 5.431 ms (alternating runs, disjoint ranges).  With 300 groups (one or two per workgroup) a launch costs 1.5 us
// more than before: the first wait covers the weights and DIST images.
// Used by mpn3.hip (K 256, TJ 2, plain, STATS / STORE, DIST 3) and mpn4.hip (K 512, TJ 1, AFFINE, POOL, DIST 2).
#pragma once
#include "group_tile.h"

namespace {

enum { GL_POOL = 1, GL_STATS = 2, GL_STORE = 4 };

template <int K_, int TJ_> struct group_lds {                                                  // a shape and what follows from it
    static constexpr int K = K_, TJ = TJ_, N = 256 * TJ, KS = K / 16, PITCH = 2 * K + 16, BUF = 32 * PITCH;      // A image: 32 rows
    static constexpr int TP = 64 * TJ + 16, TR = 32 * TP;                                      // a wave's transpose tile
    static constexpr int LPR = K / 8;                                                          // lanes of a row's LDS-DMA piece
    static constexpr int NB = 4 * BUF <= 72 * 1024 ? 4 : 3, DIST = NB - 1;                     // ring slots; groups requested ahead
    static constexpr int ROWS = 4;                                                             // a wave's rows (requests) per group
    static constexpr int TERM = 128 * TJ, LPT = TERM / 16;                                     // a wave's group term: bytes, lanes of its piece
    static constexpr int RING = NB * BUF, TERMS = NB * 8 * TERM;                               // the A ring and the term ring behind it
    static constexpr int ROW_STORES = (32 * 4 * TJ + 63) / 64;                                 // PPT_GT_TILE_OUT's instructions
};

template <typename F, int K, int TJ, bool AFFINE, int EP>
__global__ __launch_bounds__(512, 2) void group_lds_kernel(const bf16_t *__restrict__ A, int n_tiles, const float *__restrict__ a_scale,
                                                            const float *__restrict__ a_shift, const bf16_t *__restrict__ W,
                                                            const float *__restrict__ add, bf16_t *__restrict__ out,
                                                            float *__restrict__ part_sum, float *__restrict__ part_m2)
{
    using G = group_lds<K, TJ>;
    constexpr bool POOL = EP & GL_POOL, STATS = EP & GL_STATS, STORE = EP & GL_STORE;
    static_assert((G::LPR == 32 || G::LPR == 64) && POOL != (STATS || STORE), "one output pointer; a row is one LDS-DMA piece");
    // vector-memory instructions a wave issues per group, and what is younger than the pieces of group it + 1 at the end of
    // iteration it: DIST - 1 groups of requests and DIST groups' stores
    constexpr int PIECES = G::ROWS + (POOL ? 0 : 1), STORES = POOL ? TJ : (STATS ? 2 * TJ : 0) + (STORE ? G::ROW_STORES : 0);
    constexpr int WAIT = (G::DIST - 1) * PIECES + G::DIST * STORES;
    static_assert(WAIT < 64, "vmcnt is a 6-bit counter");
    extern __shared__ __align__(16) unsigned char smem[];          // NB A images, (not POOL) NB x 8 terms, (STORE) 8 transpose tiles
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 31, h = lane >> 5;
    const int n_w = 32 * TJ * w;                                    // first column of this wave
    int t = blockIdx.x;
    if (t >= n_tiles) return;
    const int last = n_tiles - 1, grid = gridDim.x;
    // this wave's four rows of group `tile`, and its 32 TJ columns of the group's term, -> ring slot `slot`
    auto request = [&](int tile, int slot) {
        if (G::LPR == 64 || lane < G::LPR) {
            const unsigned char *src = reinterpret_cast<const unsigned char *>(A) + ((size_t)tile * 32 + w) * (2 * K) + 16 * lane;
            unsigned char *dst = smem + slot * G::BUF + w * G::PITCH;
#pragma unroll
            for (int i = 0; i < G::ROWS; ++i) lds_dma16(src + (size_t)8 * i * (2 * K), dst + 8 * i * G::PITCH);
        }
        if constexpr (!POOL)
            if (lane < G::LPT) lds_dma16(add + (size_t)tile * G::N + n_w + 4 * lane, smem + G::RING + (slot * 8 + w) * G::TERM);
    };
#pragma unroll
    for (int d = 0; d < G::DIST; ++d) request(min(t + d * grid, last), d);
    uint4 bfrag[TJ][G::KS];
    float bias[TJ];
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
        PPT_GT_LOAD_WEIGHTS(bfrag[j], G::KS, W, n_w + 32 * j + col, h);
        if constexpr (POOL) bias[j] = add ? add[n_w + 32 * j + col] : 0.f;
    }
    unsigned char *tr = smem + G::RING + G::TERMS + w * G::TR;
    float sc[8], sh[8];
    if constexpr (AFFINE)
#pragma unroll
        for (int e = 0; e < 8; ++e) { sc[e] = a_scale[8 * (lane % G::LPR) + e]; sh[e] = a_shift[8 * (lane % G::LPR) + e]; }
    // the prologue in place, on the rows this wave requested (lane l asked for chunk l of each of them)
    auto affine = [&](int slot) {
        if (G::LPR == 64 || lane < G::LPR) {
            unsigned char *d = smem + slot * G::BUF + w * G::PITCH + 16 * lane;
#pragma unroll
            for (int i = 0; i < G::ROWS; ++i) {
                uint4 v = *reinterpret_cast<const uint4 *>(d + 8 * i * G::PITCH);
                affine_relu_chunk16<F>(v, sc, sh);
                *reinterpret_cast<uint4 *>(d + 8 * i * G::PITCH) = v;
            }
        }
    };
    // Everything requested so far has landed: the first DIST images and every load the compiler keeps count of.  (vmcnt 0, the
    // other counters left alone.)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    asm volatile("" ::: "memory");
    if constexpr (AFFINE) affine(0);
    lds_barrier();
    int cur = 0;                                                    // slot of group `it`; the slot before it takes group it + DIST
    for (; t < n_tiles; t += grid) {
        const int nxt = cur + 1 == G::NB ? 0 : cur + 1;
        request(min(t + G::DIST * grid, last), cur == 0 ? G::NB - 1 : cur - 1);
        __builtin_amdgcn_sched_barrier(0);                          // the requests stand in front of the first MFMA
        const unsigned char *at = smem + cur * G::BUF + col * G::PITCH + 16 * h;
        ppt_f32x16 acc[TJ];
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
#pragma unroll
        for (int s = 0; s < G::KS; ++s) {
            const uint4 a = *reinterpret_cast<const uint4 *>(at + 32 * s);
#pragma unroll
            for (int j = 0; j < TJ; ++j) acc[j] = h16<F>::mfma32(a, bfrag[j][s], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const size_t o = (size_t)t * G::N + n_w + 32 * j + col;
            if constexpr (POOL) {
                float mx = -INFINITY;
#pragma unroll
                for (int e = 0; e < 16; ++e) mx = fmaxf(mx, acc[j][e] + bias[j]);
                mx = xor32_max(mx);
                if (h == 0) out[o] = h16<F>::from_f32(mx);
            } else {
                const float gt = *reinterpret_cast<const float *>(smem + G::RING + (cur * 8 + w) * G::TERM + 4 * (32 * j + col));
                float sm = 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    acc[j][e] += gt;
                    sm += acc[j][e];
                }
                if constexpr (STATS) PPT_GT_CHUNK_STATS(acc[j], sm, h, part_sum, part_m2, o);
                if constexpr (STORE) PPT_GT_TILE_TO_LDS(F, acc[j], tr, G::TP, j, lane, col, h);
            }
        }
        if constexpr (STORE) PPT_GT_TILE_OUT(TJ, tr, G::TP, out, (size_t)t * 32, G::N, n_w, lane);
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(WAIT) : "memory");
        if constexpr (AFFINE) affine(nxt);
        lds_barrier();
        cur = nxt;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // the clamped requests: nothing may land in LDS after the workgroup has left
}

}  // namespace
