// attention_ragged.hip -- causal attention forward over RAGGED sentence rows (head dim 64): the CLIP text tower on text other than
// the model's own prompts (zero-shot template ensembles, free captions).
//
// Replaces nn.MultiheadAttention at ULIP_models.py:38,49-51 with the causal mask of :224-230 for sentences whose EOT positions
// differ (:219 pools at argmax of the token ids): the reference pads every sentence to 77 positions; here sentence s owns rows
// [off[s], off[s + 1]) of the packed [M, 3, H, 64] qkv tensor, position p at row off[s] + p, nothing behind its EOT is stored.
//
// A sentence is 2-77 keys (6-13 for a class-name template), so the streaming kernel's grid -- one 256-thread workgroup per
// 128 queries of one (sentence, head) -- would spend a workgroup on six rows.  Here the sentences are packed into BINS of 64
// virtual rows, each sentence at a 16-row boundary of its bin (the host's plan: ops.ragged_attention_plan), and a workgroup
// takes TWO (bin, head) pairs: waves 0-1 the 64 queries of one pair, waves 2-3 of the next; the 64 virtual rows of a bin are the
// pair's one K / V tile.  With 16-row slots a bin holds four 9-token sentences: eight (sentence, head) pairs per workgroup.
// A sentence of 65-128 tokens takes two bins of its own; the unit of its second bin walks both tiles with the running softmax.
//
// The arithmetic is attn_fwd_stream's (attention_mfma.hip), member for member of AttnForm<FORM> (attn_form.h): S^T = K . Q^T with
// the K tile as the A operand and a lane's query as one B column, P = exp2(S c - m) packed straight into the B operand of
// O^T = V^T . P, fp32 statistics.  A column of either product depends on its own query and on the key ROWS only, keys of other
// sentences in the tile are masked to -inf (P = 0 exactly, like the keys behind a query in the streaming kernel), and a sentence
// starts at a multiple of 16 keys -- one k-step of the second product -- so every sum sees the same terms in the same order as
// the streaming kernel run on the sentence alone: the same bits, for every form, wherever the sentence lands in its bin.
// No atomics, no LSE (nothing on this path trains).
#include "attn_form.h"

namespace {

// plan entry of a virtual row: (sentence << 8) | position, or -1 for an empty row
constexpr int RG_POS_BITS = 8, RG_POS_MASK = 255;

template <int FORM>
__global__ __launch_bounds__(256, 2) void attn_fwd_ragged(const typename AttnForm<FORM>::T *__restrict__ qkv,
                                                       typename AttnForm<FORM>::T *__restrict__ out, const int *__restrict__ offsets,
                                                       const int *__restrict__ plan, int S, int M, int nbins, int H,
                                                       float c /* scale*log2(e) */, int prio)
{
    using A = AttnForm<FORM>;
    using E = typename A::T;
    using chunk_t = typename A::chunk_t;
    constexpr int IMG = A::IMAGES * TILE;                      // bytes of a K or V tile in LDS
    constexpr int EPC = 16 / (int)sizeof(E);                   // elements per 16-byte chunk
    __shared__ __align__(16) unsigned char smem[2 * 2 * IMG];  // unit 0: K V, unit 1: K V
    PPT_PRIO(prio);
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int u = w >> 1;                                      // this wave's unit
    const int npairs = nbins * H;
    // tiles of the two units of this workgroup (0: no such pair): a bin whose first row is position 64 continues a long sentence
    int nt[2];
#pragma unroll
    for (int uu = 0; uu < 2; ++uu) {
        const int pr = (int)blockIdx.x * 2 + uu;
        const int pe = pr < npairs ? plan[(pr / H) * KVT] : -1;
        nt[uu] = pr < npairs ? (pe >= 0 && (pe & RG_POS_MASK) >= KVT && pr / H > 0 ? 2 : 1) : 0;
    }
    const int nkt = max(nt[0], nt[1]);
    const int ntu = __builtin_amdgcn_readfirstlane(nt[u]);
    const int pair = (int)blockIdx.x * 2 + u;
    const int bin = ntu ? pair / H : 0, head = ntu ? pair % H : 0;
    const int64_t rs = 3 * (int64_t)H * HD;
    const E *qb = qkv + head * HD;
    const E *kb = qb + H * HD, *vb = qb + 2 * H * HD;

    // this lane's query: virtual row vq of the bin
    const int vq = (w & 1) * 32 + r;
    const int qe = ntu ? plan[bin * KVT + vq] : -1;
    const int qs = qe >> RG_POS_BITS, qpos = qe & RG_POS_MASK;
    int64_t qrow = -1;
    if (qe >= 0 && qs < S) qrow = (int64_t)offsets[qs] + qpos;
    const bool valid = qrow >= 0 && qrow < M;
    // keys are numbered from the first tile of the unit: this query is key qv, its sentence starts at key qv - qpos.
    // (a lane without a query keeps every key: zero scores, finite numbers, nothing stored)
    const int qv = valid ? (ntu - 1) * KVT + vq : 2 * KVT, vstart = valid ? qv - qpos : 0;
    const bool wave_on = __builtin_amdgcn_readfirstlane((int)(__ballot(valid) != 0)) != 0;

    typename A::Q q;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
        for (int j = 0; j < 8 / EPC; ++j) q.raw[kk][j] = A::zero();
        if (valid) {
            const E *qp = qb + qrow * rs + 16 * kk + 8 * h;
#pragma unroll
            for (int j = 0; j < 8 / EPC; ++j) q.raw[kk][j] = *reinterpret_cast<const chunk_t *>(qp + EPC * j);
        }
        A::prep_q(q, kk);
    }

    unsigned char *Ku = smem + (2 * u) * IMG, *Vu = smem + (2 * u + 1) * IMG;
    constexpr int NST = (KVT << A::CH_SHIFT) / 128;            // 16-byte chunks of a K (or V) tile per thread of the unit
    const int tu = threadIdx.x & 127;

    f32x16_t ot[2];
    ATTN_ZERO2(ot[0], ot[1]);
    float m = -INFINITY, l = 0.f;
    const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    const int tr_key = 4 * (g >> 1) + tq;
    const int tr_dbyte = (16 * (g & 1) + 4 * tp) * 2;

    for (int kt = 0; kt < nkt; ++kt) {
        if (kt) __syncthreads();                               // every wave is done with the previous tile
        if (kt < ntu) {
            const int tb = bin - (ntu - 1) + kt;               // the bin whose rows are this tile
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const int cidx = tu + 128 * i;
                const int row = cidx >> A::CH_SHIFT, ch = cidx & ((1 << A::CH_SHIFT) - 1);
                const int ke = tb >= 0 ? plan[tb * KVT + row] : -1;
                chunk_t sk = A::zero(), sv = A::zero();
                if (ke >= 0 && (ke >> RG_POS_BITS) < S) {
                    const int64_t krow = (int64_t)offsets[ke >> RG_POS_BITS] + (ke & RG_POS_MASK);
                    if (krow < M) {
                        sk = *reinterpret_cast<const chunk_t *>(kb + krow * rs + ch * EPC);
                        sv = *reinterpret_cast<const chunk_t *>(vb + krow * rs + ch * EPC);
                    }
                }
                A::write(Ku, Vu, row, ch, sk, sv);
            }
        }
        __syncthreads();
        if (kt < ntu && wave_on) {                             // wave-uniform
            f32x16_t st[2];
            ATTN_ZERO2(st[0], st[1]);
            A::qk(st, Ku, q, r, h);
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int key = kt * KVT + 32 * sub + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (key < vstart || key > qv) st[sub][e] = -INFINITY;
                }
            float mx = st[0][0];
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int e = 0; e < 16; ++e) mx = fmaxf(mx, st[sub][e]);
            mx = xor32_max(mx);
            const float mn = fmaxf(m, mx * c);
            const float alpha = __builtin_amdgcn_exp2f(m - mn);
            m = mn;
            float psum = 0.f;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float pv = __builtin_amdgcn_exp2f(fmaf(st[sub][e], c, -mn));
                    if constexpr (A::P_PRE != 1.0f) st[sub][e] = pv * A::P_PRE;
                    else st[sub][e] = pv;
                    psum += pv;
                }
            l = fmaf(l, alpha, psum);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) ot[i][e] *= alpha;
            A::pv(ot, st, Vu, tr_key, tr_dbyte);
        }
    }

    const float lt = xor32_sum(l);
    if (valid) {
        float inv;
        if constexpr (A::P_PRE != 1.0f) inv = 1.0f / (lt * A::P_PRE);
        else inv = 1.0f / lt;
        A::store_o(out + qrow * (H * HD) + head * HD, ot, inv, h);
    }
}

template <int FORM>
int launch_fwd_ragged(const void *qkv, void *out, const int *offsets, const int *plan, int S, int M, int nbins, int H, float scale,
                      hipStream_t s)
{
    using E = typename AttnForm<FORM>::T;
    const float c = scale * 1.4426950408889634f;
    const int64_t npairs = (int64_t)nbins * H;
    hipLaunchKernelGGL((attn_fwd_ragged<FORM>), dim3((unsigned)((npairs + 1) / 2)), dim3(256), 0, s, (const E *)qkv, (E *)out, offsets, plan,
                       S, M, nbins, H, c, ppt_get_wave_priority());
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

}  // namespace

extern "C" int ppt_attention_ragged_fwd(const void *qkv, void *out, const int *offsets, const int *plan, int S, int M, int nbins, int H,
                                        int hd, float scale, int dtype, void *stream)
{
    if (!qkv || !out || !offsets || !plan || S <= 0 || M <= 0 || nbins <= 0 || H <= 0 || hd != HD) return PPT_EINVAL;
    if ((int64_t)nbins * H > (int64_t)1 << 30) return PPT_EINVAL;
    if (((uintptr_t)qkv & 15) || ((uintptr_t)out & 15)) return PPT_EINVAL;
    hipStream_t s = ppt_stream(stream);
    if (dtype == PPT_F32) return launch_fwd_ragged<PPT_F32>(qkv, out, offsets, plan, S, M, nbins, H, scale, s);
    if (dtype == PPT_F16) return launch_fwd_ragged<PPT_F16>(qkv, out, offsets, plan, S, M, nbins, H, scale, s);
    if (dtype == PPT_BF16) return launch_fwd_ragged<PPT_BF16>(qkv, out, offsets, plan, S, M, nbins, H, scale, s);
    return PPT_EINVAL;
}
