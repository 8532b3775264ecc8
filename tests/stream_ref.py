"""Shared by tests/test_stream_ref_cpu.py and tests/test_stream_kernels_gpu.py: fp64 references of the streaming kernels between
the GEMMs of the three point encoders (csrc/pointmlp.hip, csrc/pointnet.hip, csrc/misc.hip's cls/max head), their case tables,
the a-priori error bounds a kernel's result is held to, and reference variants broken on purpose.  Plain torch on the CPU, no
ppt_amd import.

Every reference is the REFERENCE FORMULATION (gather a tensor, subtract, sum; relu(bn(x) + res); P[idx] + Q ...), not the
kernel's algebra, in fp64 on the kernel's actual inputs (16-bit inputs upcast exactly).

The criterion.  Where a kernel's arithmetic is one IEEE operation the CPU reproduces (gather_add's y, cls_max_pool, the P / Q
operands of pointmlp_pq) the result must be torch.equal.  Elsewhere, per element and with no element excluded,

    |got - exact|  <=  SLACK * r * 2^-24 * sum|terms|   (+ half an ulp of the output format at |got| when it is 16-bit)

r = the fp32 roundings on the longest path to that output, counted from the kernel's code and written out next to each bound
below; sum|terms| = the absolute values of what enters the output.  For a sum, r = the adds of one lane or thread + the depth
of the reduction; what conv1_stats, cloud_rstd and bn_finalize do in fp64 is counted in units of 2^-53.  Bounds of derived
quantities (mean, variance, 1 / std) are these bounds propagated to first order through the reference formula.  SLACK = 2 is
the only constant: it covers the second-order terms ((1 + u)^r - 1 > r u) and the ulp taken at `got` instead of `exact`.  Nothing
here was measured on a kernel.  linear3_gelu keeps the project's 1e-5 * max(1, |ref|) (erff is not an IEEE operation), with no
slack, plus the half ulp of a 16-bit output.

relu, max and the select by the sign of the scale are continuous (1-Lipschitz in each argument): a bound on the operands is a
bound on the result, no tie needs conditioning.

How much room a correct kernel has.  Where r counts a summation (group_anchor_stats, gather_add's partials and what
bn_finalize makes of them, the 1 / std that follows group_anchor_stats) a correct fp32 result in ANOTHER summation order stays
below a quarter of the bound (SPARE = 4; test_stream_ref_cpu.py).  Where the bound IS one final rounding -- an element-wise
kernel (r = 1 or 2), any 16-bit output, the single fp32 cast behind conv1_stats' and cloud_rstd's fp64 arithmetic -- a correctly
rounded result reaches 1 / SLACK of it by construction (half an ulp is up to 2^-24 of the value) and a 16-bit one nearly all of
it, so no model can have a factor 4 to spare there and r cannot be counted lower than 1: those are held to the bound itself
(SPARE = 1).
"""
import math

import torch
import torch.nn.functional as F

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
U32, U64 = 2.0 ** -24, 2.0 ** -53
SLACK = 2.0
EPS_STD, BN_EPS, BN_MOM = 1e-5, 1e-5, 0.1
GA_CHUNK, C1_CHUNK = 32, 2048                  # rows per (sum, M2) partial: ppt_gather_add, ppt_conv1_stats

MUTATIONS = ("skip_last_groups", "channels_padded_64", "cloud0_base", "biased_var", "stats_from_rounded", "tail_mean_32",
             "max_under_negative", "res_affine_no_relu", "pool_strided", "last_max")


def dtype_name(dtype):
    return {F16: "f16", BF16: "bf16", F32: "f32"}[dtype]


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# --------------------------------------------------------------------------------------------------------------- the criterion
def half_ulp(got, dtype):
    """half the spacing of `dtype` at |got| (zero for fp32 outputs: their rounding is counted in r)"""
    g = got.double().abs()
    if dtype == F32:
        return torch.zeros_like(g)
    p, emin = (8, -126) if dtype == BF16 else (11, -14)        # significand bits, exponent of the smallest normal
    _, e = torch.frexp(g)                                      # |got| = m 2^e, 0.5 <= m < 1: exponent e - 1
    E = torch.where(g == 0, torch.full_like(e, emin), torch.clamp(e - 1, min=emin))
    return torch.ldexp(torch.ones_like(g), E - p)


def ratio(got, exact, bound, out_dtype=F32, slack=SLACK):
    """max over ALL elements of |got - exact| / (slack * bound + half_ulp); 0 where got == exact, inf where a non-zero error meets a
    zero bound or got is not finite"""
    err = (got.double() - exact).abs()
    lim = slack * bound + half_ulp(got, out_dtype)
    r = torch.where(err == 0, torch.zeros_like(err), err / lim)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return r.max().item()


# ------------------------------------------------------------------------------------------ group_anchor_stats and cloud_rstd
GAS_CASES = ((3, 37, 5, 24, 64),        # 15 groups: the last workgroup of four waves is partly filled
             (2, 50, 7, 1, 40),         # D < 64 (idle lanes), K = 1
             (1, 64, 4, 24, 100),       # the second channel pass of a lane is partly filled
             (2, 33, 6, 3, 128))        # (B, Nsrc, S, K, D)


def gas_inputs(case, dtype):
    """x [B*Nsrc, D] in dtype, idx [B,S,K], anchor [B,S].  idx has duplicates and hits row 0 and row Nsrc - 1 of the LAST cloud
    (b >= 1 where B > 1); group 0 of that cloud has its anchor inside its neighbour list, group 0 of cloud 0 outside."""
    B, Nsrc, S, K, D = case
    g = _gen(*case)
    x = (torch.randn(B * Nsrc, D, generator=g) + 0.5).to(dtype)
    idx = torch.randint(0, Nsrc, (B, S, K), generator=g)
    anchor = torch.randint(0, Nsrc, (B, S), generator=g)
    b = B - 1
    idx[b, 0, 0] = 0
    idx[b, 1, K - 1] = Nsrc - 1
    idx[b, 2, 0] = idx[b, 1, K - 1]                            # a duplicate across groups ...
    if K >= 3:
        idx[b, 2, 1] = idx[b, 2, 2]                            # ... and inside one
    anchor[b, 0] = idx[b, 0, 0]
    anchor[0, 1 if B == 1 else 0] = next(r for r in range(Nsrc) if r not in idx[0, 1 if B == 1 else 0].tolist())
    return x, idx, anchor


def _gas_diff(case, x, idx, anchor, mut=None):
    """the gathered, anchor-centred tensor [B, S, K, D'] in fp64 (D' = D)"""
    B, Nsrc, S, K, D = case
    Dp = -(-D // 64) * 64 if mut == "channels_padded_64" else D
    flat = torch.cat([x.double().reshape(-1), torch.zeros(Dp, dtype=torch.float64)])
    base = torch.zeros(B, dtype=torch.int64) if mut == "cloud0_base" else torch.arange(B) * Nsrc
    cols = torch.arange(Dp)
    nb = flat[((base[:, None, None] + idx) * D)[..., None] + cols]                 # [B,S,K,Dp]
    an = flat[((base[:, None] + anchor) * D)[..., None] + cols]                    # [B,S,Dp]
    return nb - an[:, :, None, :]


def gas_exact(case, x, idx, anchor, mut=None):
    """-> (stats [B,S,2] fp64 = (sum, sum of squares) of x[idx] - x[anchor] per group, bound [B,S,2])

    r, from group_anchor_stats_kernel: the subtraction (1; for the squares the product carries it twice: 2), the adds or fmas of
    one lane (ceil(D / 64) channel passes x K neighbours), the 6 steps of the wave reduction."""
    B, Nsrc, S, K, D = case
    d = _gas_diff(case, x, idx, anchor, mut)
    st = torch.stack([d.sum((2, 3)), (d * d).sum((2, 3))], -1)
    lane = -(-D // 64) * K
    bound = torch.stack([(1 + lane + 6) * U32 * d.abs().sum((2, 3)), (2 + lane + 6) * U32 * (d * d).sum((2, 3))], -1)
    if mut == "skip_last_groups":
        st = st.clone()
        st.view(-1, 2)[B * S - (B * S) % 4:] = 0.0
    return st, bound


def gas_rstd_exact(case, x, idx, anchor, mut=None):
    """r [B] fp64 = 1 / (unbiased std over the cloud's S*K*D anchor-centred values + 1e-5)  (pointMLP.py:170-175)"""
    d = _gas_diff(case, x, idx, anchor).reshape(case[0], -1)
    return 1.0 / (d.std(dim=-1, unbiased=mut != "biased_var") + EPS_STD)


def rstd_from_stats(st, n, mut=None):
    """the same from per-group (sum, sum of squares) [B,S,2]; variance clamped at 0"""
    s = st.double().sum(1)
    var = ((s[:, 1] - s[:, 0] * s[:, 0] / n) / (n if mut == "biased_var" else n - 1.0)).clamp_min(0.0)
    return 1.0 / (var.sqrt() + EPS_STD)


def rstd_bound(st, n, dstats=None):
    """bound on r [B] given a bound dstats [B,S,2] on the statistics (None: they are the kernel's exact inputs).

    cloud_rstd_kernel in fp64 (unit 2^-53): a thread adds ceil(S / 256) values, the LDS tree has 8 levels; then the variance from
    sq - sum^2 / n (4 operations on |sq| + sum^2 / n), sqrt, + eps, reciprocal (3), and ONE cast to fp32 (r = 1, unit 2^-24).  The
    statistics' bound goes through var = (sq - sum^2 / n) / (n - 1) to first order and through 1 / (sqrt(var) + eps) as an interval
    (the map is not Lipschitz at var = 0)."""
    st = st.double()
    S = st.shape[1]
    s = st.sum(1)
    dsum = (-(-S // 256) + 8) * U64 * st[..., 0].abs().sum(1)
    dsq = (-(-S // 256) + 8) * U64 * st[..., 1].abs().sum(1)
    if dstats is not None:
        dsum, dsq = dsum + dstats[..., 0].sum(1), dsq + dstats[..., 1].sum(1)
    var = ((s[:, 1] - s[:, 0] * s[:, 0] / n) / (n - 1.0)).clamp_min(0.0)
    dvar = (dsq + (2.0 * s[:, 0].abs() * dsum + dsum * dsum) / n + 4 * U64 * (s[:, 1].abs() + s[:, 0] * s[:, 0] / n)) / (n - 1.0)
    r = 1.0 / (var.sqrt() + EPS_STD)
    lo = 1.0 / ((var + dvar).sqrt() + EPS_STD)
    hi = 1.0 / ((var - dvar).clamp_min(0.0).sqrt() + EPS_STD)
    return torch.maximum(hi - r, r - lo) + (U32 + 3 * U64) * r


RSTD_S = (1, 5, 255, 256, 257, 600)


def rstd_inputs(S):
    """stats [3,S,2] f32 and n: cloud 0 random; cloud 1 all zero and cloud 2 the statistics of a cloud whose values are all 3 (sum
    3 m, squares 9 m per group of m = 96 values: exact) -- both have variance exactly 0 in fp64"""
    g = _gen(S, 17)
    m = 96
    st = torch.rand(3, S, 2, generator=g) * torch.tensor([1.0, 40.0]) * m / 24.0
    st[1] = 0.0
    st[2, :, 0], st[2, :, 1] = 3.0 * m, 9.0 * m
    return st, float(S * m)


# ------------------------------------------------------------------------------------------------------------ bn_res_act_rows
BRA_SHAPES = ((48, 64, 1), (48, 64, 24), (10, 24, 5), (9, 20, 3), (48, 64, 48))          # (M, C, pool)


def _bra_cases():
    """(id, (M, C, pool), x / res / y formats, res_affine, x misaligned).  The id names the instantiation
    bn_res_act_rows_kernel<VEC, RES_AFF, BF16IO> the dispatch in ppt_bn_res_act_rows takes: VEC = 8 needs C % 8 == 0 and every
    pointer on 16 bytes, BF16IO all three formats bf16."""
    out = []

    def add(shape, xd, rd, yd, aff, mis=False):
        M, C, pool = shape
        vec = C % 8 == 0 and not mis
        h = vec and xd == rd == yd == BF16
        inst = f"<{8 if vec else 1},{'aff' if aff else 'res'},{'bf16io' if h else 'any'}>"
        out.append((f"{inst}-m{M}c{C}p{pool}-{dtype_name(xd)}.{dtype_name(rd)}.{dtype_name(yd)}" + ("-misaligned" if mis else ""),
                    shape, xd, rd, yd, aff, mis))
    for aff in (False, True):
        for shape in BRA_SHAPES:
            add(shape, F32, F32, F32, aff)
            add(shape, BF16, BF16, BF16, aff)
        add((48, 64, 24), BF16, F32, BF16, aff)                 # mixed formats in the non-BF16IO vector kernel
        add((48, 64, 24), F32, BF16, F32, aff)
        add((48, 64, 1), F32, F32, F32, aff, mis=True)          # C % 8 == 0 but x one element off a 16-byte boundary
        add((48, 64, 1), BF16, BF16, BF16, aff, mis=True)
    return tuple(out)


BRA_CASES = _bra_cases()
BRA_BY_ID = {c[0]: c for c in BRA_CASES}
BRA_INSTANTIATIONS = ("<8,aff,bf16io>", "<8,res,bf16io>", "<8,aff,any>", "<8,res,any>", "<1,aff,any>", "<1,res,any>")


def bra_inputs(case):
    """x, res [M,C] in their formats; scale, shift, rs, rh [C] f32 (finite, both signs).  Column 1 of pool group 0: scale 1, shift
    -50, x and res negative -- every pre-activation of the group is negative (with and without the residual affine)."""
    _, (M, C, pool), xd, rd, _, _, _ = case
    g = _gen(M, C, pool, 3)
    x, res = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    sc, sh = 1.0 + 0.5 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    rs, rh = 1.0 + 0.5 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    sc[0], sc[1], sh[1] = -0.7, 1.0, -50.0
    x[:pool, 1], res[:pool, 1] = -x[:pool, 1].abs(), -res[:pool, 1].abs()
    return x.to(xd), res.to(rd), sc, sh, rs, rh


def bra_exact(case, x, res, sc, sh, rs, rh, mut=None):
    """-> (y [M/pool, C] fp64 = max over each `pool` consecutive rows of relu(sc x + sh + res'), bound)

    r = 2, from bn_res_act_rows_kernel: fmaf(x, sc, sh) rounds once (and, in parallel, fmaf(res, rs, rh) once -- its relu is exact),
    their sum once more.  The first-order error is u (|sc x| + |sh|) + u (|rs res| + |rh|) + u |sum| <= 2 u sum|terms|; relu and
    the running max are exact and 1-Lipschitz, so a pooled element carries the largest bound among its rows."""
    _, (M, C, pool), _, _, _, aff, _ = case
    x, res, sc, sh, rs, rh = (t.double() for t in (x, res, sc, sh, rs, rh))
    if aff:
        lin = rs * res + rh
        rr, rterms = (lin if mut == "res_affine_no_relu" else torch.relu(lin)), (rs * res).abs() + rh.abs()
    else:
        rr, rterms = res, res.abs()
    y = torch.relu(sc * x + sh + rr)
    b = 2 * U32 * ((sc * x).abs() + sh.abs() + rterms)
    G = M // pool
    if mut == "pool_strided":
        return y.view(pool, G, C).amax(0), b.view(pool, G, C).amax(0)
    return y.view(G, pool, C).amax(1), b.view(G, pool, C).amax(1)


# ------------------------------------------------------------------------------------------------------------------ gather_add
GA_CASES = ((3, 40, 5, 24, 64),         # M = 360: an 8-row tail chunk, chunks straddle groups
            (2, 33, 3, 16, 200),        # C > 128 and no multiple of 128: a thread's second column, partly filled
            (1, 20, 1, 5, 8))           # one chunk shorter than 32      (B, Nsrc, S, K, C)


def ga_inputs(case):
    B, Nsrc, S, K, C = case
    g = _gen(*case)
    P = torch.randn(B * Nsrc, C, generator=g) + 0.3
    Q = torch.randn(B * S, C, generator=g)
    idx = torch.randint(0, Nsrc, (B, S, K), generator=g)
    idx[B - 1, 0, 0], idx[B - 1, S - 1, K - 1] = 0, Nsrc - 1
    if K >= 3:
        idx[0, 0, 1] = idx[0, 0, 2]
    return P, Q, idx


def _ga_rows(case, P, Q, idx):
    B, Nsrc, S, K, C = case
    src = (torch.arange(B)[:, None, None] * Nsrc + idx).reshape(-1)
    ctr = torch.arange(B * S).repeat_interleave(K)
    return P[src], Q[ctr]


def ga_y(case, P, Q, idx, y_dtype):
    """the one IEEE addition of the kernel, cast once: y must be torch.equal to this"""
    p, q = _ga_rows(case, P, Q, idx)
    return (p + q).to(y_dtype)


def _chunks(M, rows):
    return [(r0, min(rows, M - r0)) for r0 in range(0, M, rows)]


def ga_exact(case, P, Q, idx, y_dtype=F32, mut=None):
    """-> ((psum, pm2) [ceil(M/32), C] fp64, their bounds, v [M,C] fp64): per 32-row chunk (the last with its real row count)
    the sum and the M2 about the chunk's own mean of the UNROUNDED rows P[idx] + Q.

    From gather_add_kernel, n = rows of the chunk:  v = P + Q rounds once, the serial sum adds n - 1 times: r = n on sum|v|.
    mean = s / n carries the sum's bound / n and one rounding; d = v - mean carries u |v|, the mean's error and its own rounding;
    M2 = sum d^2 by n fmas: first order  sum 2 |d| dd  +  n u sum d^2."""
    B, Nsrc, S, K, C = case
    p, q = _ga_rows(case, P, Q, idx)
    v = p.double() + q.double()
    vs = (p + q).to(y_dtype).double() if mut == "stats_from_rounded" else v
    ps, pm, bs, bm = [], [], [], []
    for r0, n in _chunks(v.shape[0], GA_CHUNK):
        c, cs = v[r0:r0 + n], vs[r0:r0 + n]
        s = cs.sum(0)
        mean = s / (GA_CHUNK if mut == "tail_mean_32" else n)
        ps.append(s)
        pm.append(((cs - mean) ** 2).sum(0))
        d = c - c.mean(0)
        bsum = n * U32 * c.abs().sum(0)
        dmean = bsum / n + U32 * c.mean(0).abs()
        dd = U32 * c.abs() + dmean + U32 * d.abs()
        bs.append(bsum)
        bm.append((2.0 * d.abs() * dd).sum(0) + n * U32 * (d * d).sum(0))
    return (torch.stack(ps), torch.stack(pm)), (torch.stack(bs), torch.stack(bm)), v


def moments_exact(v):
    """fp64 mean and BIASED variance over all rows"""
    return v.mean(0), v.var(0, unbiased=False)


def finalize_bound(partials, bounds, M, rows):
    """bounds on what ppt_bn_finalize makes of (sum, M2) partials that are within `bounds`: -> (mean, biased var, rstd =
    1 / sqrt(var + eps)) bounds [C].

    The fold is fp64 (Chan's merge: M2 = sum M2_c + sum n_c (mean_c - mean)^2, evaluated as S2 + S3 - S1^2 / N: 64 x 2^-53 on
    S2 + S3 + S1^2 / N covers its adds and the cancellation).  The partials' bounds go through to first order.  Then ONE cast to fp32
    each for mean and var (r = 1), and rstd = 1 / sqrtf(var + eps): add, sqrt, divide (r = 3) behind the propagated variance."""
    ps, pm = (t.double() for t in partials)
    bs, bm = bounds
    n = torch.tensor([float(c) for _, c in _chunks(M, rows)], dtype=torch.float64)[:, None]
    mean = ps.sum(0) / M
    mc = ps / n
    var = (pm.sum(0) + (n * (mc - mean) ** 2).sum(0)) / M
    dmean = bs.sum(0) / M
    dm2 = bm.sum(0) + (2.0 * n * (mc - mean).abs() * (bs / n + dmean)).sum(0)
    dm2 = dm2 + 64 * U64 * (pm.sum(0) + 2.0 * (ps * ps / n).sum(0))
    dvar = dm2 / M
    bvar = dvar + U32 * var
    rstd = 1.0 / (var + BN_EPS).sqrt()
    return dmean + U32 * mean.abs(), bvar, rstd * 0.5 * bvar / (var + BN_EPS) + 3 * U32 * rstd


# ----------------------------------------------------------------------------------------------------------------- pool_finish
PF_CASES = tuple((pd, od, fold) for pd, od in ((F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32)) for fold in (1, 2, 4))
PF_G, PF_C = 7, 40


def pf_inputs(case):
    """pmax >= pmin [G*fold, C] in the input format; scale [C] positive, negative and (column 0) exactly 0"""
    pd, _, fold = case
    g = _gen(fold, 23)
    a, b = torch.randn(PF_G * fold, PF_C, generator=g), torch.randn(PF_G * fold, PF_C, generator=g)
    sc, sh = torch.randn(PF_C, generator=g), 0.5 * torch.randn(PF_C, generator=g)
    sc[0], sc[1], sc[2], sh[0] = 0.0, -1.3, 0.8, 0.25
    return torch.maximum(a, b).to(pd), torch.minimum(a, b).to(pd), sc, sh


def pf_exact(case, pmax, pmin, sc, sh, mut=None):
    """-> (relu(sc * (sc >= 0 ? max_f pmax : min_f pmin) + sh) [G,C] fp64, bound).  r = 1: the folds are exact, one fmaf rounds."""
    _, _, fold = case
    mx = pmax.double().view(PF_G, fold, PF_C).amax(1)
    mn = pmin.double().view(PF_G, fold, PF_C).amin(1)
    sc, sh = sc.double(), sh.double()
    sel = mx if mut == "max_under_negative" else torch.where(sc >= 0, mx, mn)
    return torch.relu(sc * sel + sh), 1 * U32 * ((sc * sel).abs() + sh.abs())


# ----------------------------------------------------------------------------------------------- conv1_stats and its bn_finalize
C1_CASES = tuple((M, C) for M in (5, 2048, 2049, 4100) for C in (3, 64, 300))


def c1_inputs(case):
    """points with a common offset of 10 (mean^2 >> variance: the cancellation the kernel's fp64 moments are there for)"""
    M, C = case
    g = _gen(M, C, 5)
    return (torch.randn(M, 3, generator=g) * 0.3 + 10.0, torch.randn(C, 3, generator=g), torch.randn(C, generator=g) * 0.1)


def c1_exact(case, pts, w1, b1):
    """-> ((psum, pm2) [ceil(M/2048), C] fp64 of y = pts @ w1.T + b1, bounds, y)

    conv1_stats_kernel works in fp64 and casts ONCE (r = 1 on |value|, unit 2^-24).  Its fp64 part, unit 2^-53: a thread adds 8
    rows into each of the nine moments, the LDS tree has 8 levels, sum^2 / n and the assembly of w . S and w^T Cov w are about ten
    more: 32 on sum_rows (|w| . |p| + |b|) for the sum, 64 on 2 sum_rows (|w| . |p|)^2 for M2 (which also covers sum^2 / n, by
    Cauchy-Schwarz)."""
    M, C = case
    y = pts.double() @ w1.double().t() + b1.double()
    mag = pts.double().abs() @ w1.double().abs().t()
    ps, pm, bs, bm = [], [], [], []
    for r0, n in _chunks(M, C1_CHUNK):
        c, m = y[r0:r0 + n], mag[r0:r0 + n]
        ps.append(c.sum(0))
        pm.append(((c - c.mean(0)) ** 2).sum(0))
        bs.append(U32 * ps[-1].abs() + 32 * U64 * (m + b1.double().abs()).sum(0))
        bm.append(U32 * pm[-1].abs() + 64 * U64 * 2.0 * (m * m).sum(0))
    return (torch.stack(ps), torch.stack(pm)), (torch.stack(bs), torch.stack(bm)), y


def bn_affine_exact(y, gamma, beta, rm, rv, momentum):
    """nn.BatchNorm1d in train() on rows y [M,C] fp64: -> scale, shift, running mean, running (unbiased) variance.  momentum: the
    fp32 value the library is handed."""
    M = y.shape[0]
    mean, var = moments_exact(y)
    sc = gamma.double() / (var + BN_EPS).sqrt()
    unb = var * (M / (M - 1.0)) if M > 1 else var
    return sc, beta.double() - mean * sc, (1.0 - momentum) * rm.double() + momentum * mean, (1.0 - momentum) * rv.double() + momentum * unb


def bn_affine_bound(y, gamma, beta, rm, rv, momentum, bmean, bvar):
    """bounds on the four, given bounds on the fp32 mean and biased variance (finalize_bound).  BN_UPDATE_RUNNING: 1 - momentum, two
    products, one add (r = 4 on |(1 - m) old| + |m new|); BN_WRITE_AFFINE: scale = gamma / sqrtf(var + eps) (r = 3), shift = beta -
    mean * scale (r = 2 on |beta| + |mean scale|), each behind the propagated statistics."""
    M = y.shape[0]
    mean, var = moments_exact(y)
    sc = gamma.double() / (var + BN_EPS).sqrt()
    dsc = sc.abs() * (0.5 * bvar / (var + BN_EPS) + 3 * U32)
    dsh = 2 * U32 * (beta.double().abs() + (mean * sc).abs()) + mean.abs() * dsc + sc.abs() * bmean
    k = M / (M - 1.0) if M > 1 else 1.0
    drm = 4 * U32 * ((1.0 - momentum) * rm.double().abs() + momentum * mean.abs()) + momentum * bmean
    drv = 4 * U32 * ((1.0 - momentum) * rv.double().abs() + momentum * k * var) + momentum * (k * bvar + U32 * k * var)
    return dsc, dsh, drm, drv


# ---------------------------------------------------------------------------------------------------------------- linear3_gelu
L3_CASES = tuple((M, C, d) for M, C in ((7, 384), (100, 5)) for d in (F32, BF16, F16))


def l3_inputs(case):
    M, C, _ = case
    g = _gen(M, C, 9)
    return torch.randn(M, 3, generator=g), torch.randn(C, 3, generator=g), torch.randn(C, generator=g) * 0.1


def l3_exact(pts, w, b):
    """erf-GELU of pts @ w.T + b in fp64, and the project's 1e-5 * max(1, |ref|) (used with slack = 1)"""
    y = F.gelu(pts.double() @ w.double().t() + b.double())
    return y, 1e-5 * y.abs().clamp_min(1.0)


# ---------------------------------------------------------------------------------------------------------------- cls_max_pool
CMP_T, CMP_D = (2, 17, 18, 65, 66, 129), (5, 64, 100)


def cmp_inputs(T, D, dtype, nonfinite=False):
    """x [2,T,D] with planted ties (column 0: two equal maxima 16 tokens apart, the same wave of the kernel; column 1: at tokens 2 and
    3, different waves; column 2: all tokens equal).  nonfinite: column 3 all NaN, column 4 all -inf, and where D > 64 (a second
    workgroup) column 5 one NaN at token 1 among finite values, 6 one NaN at token 2 only (a later wave), 7 NaN at the last token,
    8 NaNs at tokens 3 and 2, D - 1 all NaN, D - 2 all -inf."""
    g = _gen(T, D, 31)
    x = torch.randn(2, T, D, generator=g).to(dtype)
    top = 8.0
    if T >= 18:
        x[:, 1, 0] = x[:, 17, 0] = top
        x[1, 1, 0], x[1, 33 if T > 33 else 17, 0] = 0.0, top
    if T >= 4:
        x[:, 2, 1] = x[:, 3, 1] = top
    x[:, 1:, 2] = 0.5
    if nonfinite:
        x[:, 1:, 3] = math.nan
        x[:, 1:, 4] = -math.inf
        if D > 64:
            x[:, 1, 5] = math.nan
            x[:, min(2, T - 1), 6] = math.nan
            x[:, T - 1, 7] = math.nan
            x[:, min(3, T - 1), 8] = x[:, min(2, T - 1), 8] = math.nan
            x[:, 1:, D - 1] = math.nan
            x[:, 1:, D - 2] = -math.inf
    return x


def cmp_exact(x, mut=None):
    """cat(x[:,0], x[:,1:].max(1)) f32 and the token index (1-based in x) of torch's maximum: NaN is the maximum, the first wins
    (point_encoder.py:251)"""
    xf = x.float()
    if mut == "last_max":
        val, i = xf[:, 1:].flip(1).max(1)
        i = xf.shape[1] - 2 - i
    else:
        val, i = xf[:, 1:].max(1)
    return torch.cat([xf[:, 0], val], 1), (i + 1).to(torch.int32)


# ----------------------------------------------------------------------------------------------------------------- pointmlp_pq
PQ_CASES = ((3, 200, 50, 64), (3, 200, 50, 4), (3, 200, 50, 36),
            (3, 2048, 1024, 512))       # more than 4096 * 256 float4 items: the grid-stride loop runs a second round   (B, N, S, C)


def pq_inputs(case):
    B, N, S, C = case
    g = _gen(*case)
    return (torch.randn(B * N, 2 * C, generator=g), torch.rand(B, generator=g) + 0.5, torch.randint(0, N, (B, S), generator=g),
            torch.randn(C, generator=g))


def pq_ref(case, PQ, r, cidx, c0):
    """the ATen expression in fp32, every operation rounded once: P = PQ[:, :C] * r[b], Q = (c0 + PQ[a, C:]) - P[a]"""
    B, N, S, C = case
    P = (PQ[:, :C].reshape(B, N, C) * r.view(B, 1, 1)).reshape(B * N, C)
    a = (torch.arange(B).view(B, 1) * N + cidx).view(-1)
    return P, ((c0.view(1, C) + PQ[:, C:][a]) - P[a]).contiguous()


# ------------------------------------------------------------------------------------------------------------------- mutations
def mutation_ratio(mut):
    """-> (the case the mutation is shown on, the ratio of the broken reference against the criterion).  Each must exceed 1."""
    if mut in ("skip_last_groups", "channels_padded_64", "cloud0_base"):
        case = {"skip_last_groups": GAS_CASES[0], "channels_padded_64": GAS_CASES[2], "cloud0_base": GAS_CASES[3]}[mut]
        inp = gas_inputs(case, F32)
        ref, bound = gas_exact(case, *inp)
        return f"group_anchor_stats {case}", ratio(gas_exact(case, *inp, mut=mut)[0], ref, bound)
    if mut == "biased_var":
        case = GAS_CASES[0]
        inp = gas_inputs(case, F32)
        st, bound = gas_exact(case, *inp)
        n = float(case[2] * case[3] * case[4])
        return f"cloud_rstd after group_anchor_stats {case}", ratio(gas_rstd_exact(case, *inp, mut=mut), gas_rstd_exact(case, *inp),
                                                                    rstd_bound(st, n, bound))
    if mut in ("stats_from_rounded", "tail_mean_32"):
        case = GA_CASES[0]
        inp = ga_inputs(case)
        (_, m2), (_, bm2), _ = ga_exact(case, *inp)
        (_, bad), _, _ = ga_exact(case, *inp, y_dtype=BF16, mut=mut)
        return f"gather_add {case} bf16 M2", ratio(bad, m2, bm2)
    if mut == "max_under_negative":
        case = PF_CASES[1]
        inp = pf_inputs(case)
        ref, bound = pf_exact(case, *inp)
        return "pool_finish f32->bf16 fold 1", ratio(pf_exact(case, *inp, mut=mut)[0].to(BF16), ref, bound, BF16)
    if mut in ("res_affine_no_relu", "pool_strided"):
        case = BRA_BY_ID["<8,aff,bf16io>-m48c64p24-bf16.bf16.bf16"]
        inp = bra_inputs(case)
        ref, bound = bra_exact(case, *inp)
        return "bn_res_act_rows " + case[0], ratio(bra_exact(case, *inp, mut=mut)[0].to(BF16), ref, bound, BF16)
    assert mut == "last_max"
    x = cmp_inputs(66, 5, F32)
    (val, i), (bv, bi) = cmp_exact(x), cmp_exact(x, mut=mut)
    return "cls_max_pool T 66 D 5", 0.0 if torch.equal(val, bv) and torch.equal(i, bi) else math.inf
