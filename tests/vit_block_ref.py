"""Shared by tests/test_vit_block_ref_cpu.py and tests/test_vit_block_gpu.py: the three launches of a frozen PointBERT block --
ppt_lnlin (csrc/lnlin.hip), ppt_rowgemm_bf16 (csrc/rowgemm.hip), ppt_vit_mlp_bf16 / ppt_vit_mlp3_bf16 (csrc/mlp_fused.hip,
csrc/mlp_fused3.hip) -- in plain torch on the CPU (no ppt_amd import), the case table, and the two-tier criterion.

  reference  the launch in fp64 on the operands' STORED values, with the roundings the kernels DEFINE reproduced: the LayerNorm
             output h is rounded to the operand format; the fused MLP's GELU output U is rounded to the operand format -- variant 2
             rounds gelu(pre) and applies (acc + b2) * rs + residual afterwards, variant 3 rounds rs * gelu(pre), starts the fc2
             accumulators at the residual and adds rs * b2 with one fma behind them.  GELU is the polynomial each kernel runs
             (gelu_poly of csrc/ppt_act.h; gelu_poly3 of csrc/mlp_fused3.hip, with its clamp) evaluated in fp64; gelu="erf" is the
             second, looser reference with the exact GELU, its bound the polynomial one's plus the approximation term.
  standin    the same launch in fp32 in ANOTHER summation order (K in 32-wide steps, LayerNorm sums in 16 partials): a correct
             kernel's proxy for the CPU test; `mutate` (MUTATIONS) breaks it the way these kernels can break.
  check      hard tier: every element within its worst-case bound; sharp tier: every ROW within the probabilistic bound except
             floor(M / 20) rows per (case, output) -- none for M < 20.  Nothing in either is measured on a kernel.

The bound (u = 2^-24; E is carried from stage to stage; k(n) = n u in the hard tier, LAMBDA sqrt(n) u in the sharp one):
  product      E = k(K) ((|a| + F) |W|^T) + flipsum(F, W): products of 16-bit operands are exact in fp32, the sum in any order; F is
               the flip term of the 16-bit operand a (below), absent for operands read from memory; flipsum = F |W|^T, in the sharp
               tier min(F |W|^T, LAMBDA sqrt(F^2 (W^2)^T)).
  each fp32 +  E += u |v|                         (bias, residuals; x * s: E = |s| E + u |v|)
  LayerNorm    of a row x (n = 384 or 512 values, each with an error Ex from the stage before, 0 for stored rows).  The kernels sum a
               row as serial per-lane sums of 12 or 24 (32 for n = 512) terms and then a 16-lane tree (4 levels) or a 32-term serial
               fold: no term passes more than 12 + 32 = 44 additions, + the product with 1 / n and the rounding of that constant:
               LN_C = 48 covers all three shapes.
                 mean   Em = k(LN_C) mean|x| + mean(Ex)
                 d      e  = Em + Ex + u |d|                                    d = x - mean
                 var    Ev = mean(2 |d| e + e^2) + k(LN_C) var + u (var + eps)
                 rstd   Er = 1 / sqrt(var + eps - Ev) - rstd + 6 u rstd         (sqrtf, the division and the sum's rounding).  RELATIVE
                        to var + eps: on a nearly constant row (var -> 0, |mean| large) Ev / (var + eps) grows like
                        k(LN_C) |mean| / spread and the bound with it -- by this formula, not by a special case; Ev >= var + eps
                        makes it infinite.
                 h      Eh = |g| (e rstd + |d| Er + e Er) + 3 u |d rstd g| + u |h|
               ln_stats: mean within Em + u |mean| (absolute), rstd within Er.
  flips        a 16-bit intermediate (h, U) is round16(value): where the fp64 value lies within its E of a rounding boundary the
               kernel's rounding may land on the other side: F = one ulp (+ one more per further ulp of E, at most E + one ulp), else 0.
               F |W| of the next product is carried on (first line), summed as the worst case in the hard tier: through the two
               rounded layers of the MLP (h, then U) that sum is what makes the hard tolerance ~2e-2 at unit scale, and with the
               proj prologue (whose product error moves ~15 % of a bf16 h row across a boundary) ~0.5 in bf16 and ~0.36 in fp16
               (medians on mlp-331): there the hard tier sees gross errors only.  The sharp tier recomputes the candidates from its
               own, smaller E and sums many of them in quadrature (_flipsum).
  GELU         E = GELU_LIP E + poly32 + u |w|: GELU_LIP = 1.14 bounds the polynomials' slope (the CPU test measures it on the
               restated polynomials), poly32 = 18 u sum_k |c_k| |x|^(2k+1) |x| / 2 the fp32 Horner evaluation of the 8-coefficient
               polynomial (cancellation makes it 3e-4 at |x| = 4, 5e-7 at 1); gelu_poly JUMPS at |x| = 4 (select of +-1), so where
               |x| is within E of 4 another 2 GELU_POLY_BOUND is added (gelu_poly3 is continuous there: the clamp).  gelu="erf"
               adds the approximation term: GELU_POLY_BOUND for gelu_poly, max(GELU_POLY_BOUND, |x| CLAMP3 / 2) for gelu_poly3.
  QuickGELU    E = 1.13 E + u (2 (1 + 1.5 |v|) |v| + 4 |w|)         (gemm_ref's, doubled for __expf)
  variant 3    acc starts at the residual: E = Ex + F |W2|^T + k(1537) (|x_mid| + (|U| + F) |W2|^T); a row whose DropPath factor is
               exactly 0 has U = 0 exactly, adds exact zeros and keeps E = Ex (+ u |v| for residual2): the branch contributes nothing.
  store        + half an ulp of the output format at |v| + E (gemm_ref's)

LAMBDA.  Higham & Mary (SIAM J. Sci. Comput. 41, 2019): with rounding errors modelled as independent and mean-free, an inner
product of n terms errs by more than LAMBDA sqrt(n) u sum |a_i b_i| with probability <= 2 exp(-LAMBDA^2 (1 - u)^2 / 2).  The largest
case here has 787 rows x 392 columns or 513 rows x (1536 + 384 + 384) inner products, < 1.2e6; LAMBDA = 7 gives 2 exp(-24.5) =
4.6e-11 per inner product, 5.5e-5 per such case, ~1e-2 over the table: the sharp tier's own exception budget is for the flips and for
the model's assumption, not for LAMBDA.  Not tuned.
"""
import collections
import functools
import math
import zlib

import torch

from gemm_ref import (ACT_GELU, ACT_NONE, ACT_QUICKGELU, FMT, GELU_POLY_BOUND, ROUND, U, Slot, _sentinel, _slot_in, _slot_out,  # noqa: F401
                      any_sentinel_inside, bits, gelu_poly, outside_intact, untouched, view)

LAMBDA = 7.0
LN_C = 48
GELU_LIP = 1.14
CLAMP3 = 1.07e-4               # csrc/mlp_fused3.hip: beyond |x| = 4 the erf factor stays 4 P(16) = 1 - 1.066e-4 while erf goes on to 1
D, HID, R_MLP = 384, 1536, 80
_MINHALF = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -150}
_COEF = (-3.161567230e-09, 2.434219084e-07, -8.201724995e-06, 1.613346976e-04, -2.096408280e-03, 1.932974532e-02, -1.323507577e-01,
         7.976950407e-01)
F64 = torch.float64

_FIELDS = dict(kernel="", M=0, N=384, K=384, family="unit", form="", bias=False, act=ACT_NONE, out2=False, ln_stats=False, rs_rows=0,
               zeros=False, res2=False, inplace=False, walkers=0, variant=0, workgroups=0, occupancy=100, proj="", prs_rows=0, note="")
Case = collections.namedtuple("Case", list(_FIELDS), defaults=list(_FIELDS.values()))
Ref = collections.namedtuple("Ref", "exact hard sharp")
Inputs = collections.namedtuple("Inputs", "dt x A W bias gam bet rs res res2 W1 b1 W2 b2 pa Wp pb prs outs")
EPS = 1e-5


def case_id(c):
    s = f"{c.kernel}-{c.M}x{c.N}x{c.K}"
    for k, d in _FIELDS.items():
        v = getattr(c, k)
        if k in ("kernel", "M", "N", "K", "note") or v == d:
            continue
        s += f"-{k}" if v is True else f"-{k}{v}"
    return s


# ------------------------------------------------------------------------------------------------ the host's chunk arithmetic
def geometry(M, workgroups, cus, occupancy=100):
    """csrc/mlp_fused.hip ppt_vit_mlp_bf16 / csrc/mlp_fused3.hip ppt_vit_mlp3_bf16, restated ->
    (n_chunks, rows_per_chunk, rows of the last chunk, chunks of the busiest workgroup)"""
    wgs = workgroups if workgroups > 0 else cus
    rounds = 1
    while rounds * wgs * R_MLP < M:
        rounds += 1
    if workgroups <= 0 and occupancy < 100:
        wgs = (M + rounds * R_MLP - 1) // (rounds * R_MLP)
    n = rounds * wgs
    rpc = (M + n - 1) // n
    n = (M + rpc - 1) // rpc
    grid = min(n, wgs)
    return n, rpc, M - (n - 1) * rpc, (n + grid - 1) // grid


def case_geometry(c, cus=256):
    return geometry(c.M, c.workgroups, cus, c.occupancy)


def family(c):
    """the kernel and form a case runs (for the failure messages)"""
    if c.kernel == "mlp":
        return f"vit_mlp{'3' if c.variant == 3 else ''}_kernel" + (" + proj prologue" if c.proj else "")
    if c.kernel == "lnlin":
        return f"lnlin_kernel, {c.N // 384} slice(s)"
    return f"rowgemm_kernel<K = {c.K}, {'LayerNorm' if c.form == 'ln' else 'residual form' if c.form == 'res' else '16-bit form'}>"


# ------------------------------------------------------------------------------------------------ inputs
def _rows(c, gen, K):
    """the fp32 rows of a case by input family"""
    M = c.M
    rn = lambda *s: torch.randn(*s, generator=gen)
    x = rn(M, K) * 2 + rn(M, 1)
    if c.family == "mean30":
        x = 30.0 + 0.5 * rn(M, K)
    elif c.family == "const":                      # nearly constant rows (large mean / small spread; small everything) and an exactly constant one
        i = torch.arange(M)
        x[i % 8 == 3] = (30.0 + 0.01 * rn(M, K))[i % 8 == 3]
        x[i % 8 == 5] = (0.01 * rn(M, K))[i % 8 == 5]
        if M > 1:
            x[1] = 30.0
    elif c.family == "outlier":
        x[:, ::37] *= 20.0
    elif c.family == "bias":                       # a small product under a bias spread over [-4, 4]: the tolerance is the polynomial's own
        x = 0.02 * rn(M, K)
    return x


def _vec(v):
    return _slot_in(v.reshape(1, 1, -1).contiguous(), v.numel(), 16)


def _mat(v):
    return _slot_in(v[None].contiguous(), v.shape[1], 16)


def vec(s, buf=None):
    return view(s, buf, z=0)[0]


def mat(s, buf=None):
    return view(s, buf, z=0)


@functools.lru_cache(maxsize=4)
def inputs(c, fmt):
    """every operand of a case as a window in a NaN-filled buffer (NaN in front of it and in one more row behind it: rows past M
    and bytes either side poison what reads them), every output as a window in a sentinel-filled buffer with a row behind it"""
    gen = torch.Generator().manual_seed(zlib.crc32((case_id(c) + fmt).encode()))
    rn = lambda *s: torch.randn(*s, generator=gen)
    dt, M, N, K = FMT[fmt], c.M, c.N, c.K
    wide = 4.0 if c.family == "wide" else 1.0
    z = dict.fromkeys(Inputs._fields)
    z["dt"] = dt
    nrs = lambda rows: (M + rows - 1) // rows
    factors = lambda n, zeros: torch.floor(0.7 + torch.rand(n, generator=gen)) / 0.7 if zeros else 0.5 + torch.rand(n, generator=gen)
    if c.kernel == "rowgemm" and c.form != "ln":
        z["A"] = _mat(_rows(c, gen, K).to(dt))
    else:
        z["x"] = _mat(_rows(c, gen, K))
    if c.kernel != "rowgemm" or c.form == "ln":
        z["gam"], z["bet"] = _vec(1.0 + 0.1 * rn(K)), _vec(0.1 * rn(K))
    if c.kernel == "mlp":
        z["W1"], z["b1"] = (wide * rn(HID, D) / math.sqrt(D)).to(dt), _vec(0.1 * wide * wide * rn(HID))
        z["W2"], z["b2"] = (rn(D, HID) / math.sqrt(HID)).to(dt), _vec(0.5 * rn(D))
        if c.proj:
            z["pa"], z["Wp"] = _mat(rn(M, D).to(dt)), (rn(D, D) / math.sqrt(D)).to(dt)
            z["pb"] = _vec(0.5 * rn(D)) if "b" in c.proj else None
            z["prs"] = _vec(factors(nrs(c.prs_rows), c.zeros)) if "s" in c.proj else None
        outs = {} if c.inplace else {"out": _slot_out(torch.float32, 1, M, D, D, 16)}
    else:
        z["W"] = (wide * rn(N, K) / math.sqrt(K)).to(dt)
        z["bias"] = _vec(8.0 * (torch.rand(N, generator=gen) - 0.5) if c.family == "bias" else 0.5 * wide * rn(N)) if c.bias else None
        outs = {}
        if c.kernel == "rowgemm" and c.form == "res":
            z["res"] = _mat(rn(M, N))
            if not c.inplace:
                outs["C"] = _slot_out(torch.float32, 1, M, N, N, 16)
        else:
            outs["C"] = _slot_out(dt, 1, M, N, N, 16)
            if c.out2:
                outs["out2"] = _slot_out(dt, 1, M, N, N, 16)
            if c.ln_stats:
                outs["mean"], outs["rstd"] = _slot_out(torch.float32, 1, 1, M, M, 16), _slot_out(torch.float32, 1, 1, M, M, 16)
    if c.rs_rows:
        z["rs"] = _vec(factors(nrs(c.rs_rows), c.zeros))
    if c.res2:
        z["res2"] = _mat(rn(M, N if c.kernel != "mlp" else D))
    z["outs"] = outs
    I = Inputs(**z)
    if c.family == "wide" and (c.kernel == "mlp" or c.form == "16"):       # at least a tenth of the GELU arguments beyond the clamp
        if c.kernel == "mlp":
            pre = torch.nn.functional.layer_norm(mat(I.x), (D,), vec(I.gam), vec(I.bet), EPS) @ I.W1.float().t() + vec(I.b1)
        else:
            pre = mat(I.A).float() @ I.W.float().t() + vec(I.bias)
        assert float((pre.abs() > 4.0).float().mean()) >= 0.1, case_id(c)
    return I


def out_name(c):
    """the output an in-place case overwrites"""
    return "out" if c.kernel == "mlp" else "C"


# ------------------------------------------------------------------------------------------------ pieces of the bound
def _k(n, tier):
    return n * U if tier == "hard" else min(n, LAMBDA * math.sqrt(n)) * U          # (n <= LAMBDA^2: the worst case is the sharper one)


def _half_ulp(v, dt):
    return (ROUND[dt] * torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(1e-300))))).clamp_min(_MINHALF[dt])


def _store(v, E, dt):
    return _half_ulp(v.abs() + E, dt)


def _flip(v, E, dt):
    """how far round_dt of a value within E of v can lie from round_dt(v): 0 unless a rounding boundary is within E (docstring)"""
    r = v.to(dt).double()
    hu = _half_ulp(v, dt)
    dist = (hu - (v - r).abs()).clamp_min(0.0)                             # to the boundary on v's side of r
    big = 2.0 * _half_ulp(v.abs() + E, dt)
    # (one ulp per ulp of E beyond the boundary; never more than E + one ulp: two roundings of values E apart -- what counts
    # where v is near 0 and its own ulp tiny)
    steps = torch.minimum(big * (1.0 + torch.floor((E - dist) / (2.0 * hu))), E + big)
    return torch.where((E > 0) & (E >= dist), steps, torch.zeros_like(v))


def _ln(x, Ex, g, b, tier):
    """LayerNorm of fp64 rows x, each value known to the kernel within Ex -> dict of the exact values and their bounds (docstring)"""
    c = _k(LN_C, tier)
    mean = x.mean(1, keepdim=True)
    Em = c * x.abs().mean(1, keepdim=True) + Ex.mean(1, keepdim=True)
    d = x - mean
    e = Em + Ex + U * d.abs()
    var = (d * d).mean(1, keepdim=True)
    Ev = (2 * d.abs() * e + e * e).mean(1, keepdim=True) + c * var + U * (var + EPS)
    t = var + EPS
    r = t.rsqrt()
    lo = t - Ev
    Er = torch.where(lo > 0, lo.clamp_min(1e-300).rsqrt() - r, torch.full_like(r, float("inf"))) + 6 * U * r
    h = d * r * g + b
    Eh = g.abs() * (e * r + d.abs() * Er + e * Er) + 3 * U * (d * r * g).abs() + U * h.abs()
    return dict(h=h, Eh=Eh, mean=mean[:, 0], Em=(Em + U * mean.abs())[:, 0], rstd=r[:, 0], Er=Er[:, 0])


def _prod(a, Fa, w, tier):
    """a [M, K] . w [N, K]^T with the flip term Fa of a (None: a is read from memory) -> value, E"""
    K = a.shape[1]
    aw = (a.abs() if Fa is None else a.abs() + Fa) @ w.abs().t()
    E = _k(K, tier) * aw
    if Fa is not None:
        E = E + _flipsum(Fa, w, tier)
    return a @ w.t(), E


def _flipsum(F, w, tier):
    """what the flips F of a 16-bit operand can move its product with w [N, K]: the worst case sum_k F_k |w_nk|; in the sharp tier
    no more than LAMBDA sqrt(sum_k (F_k w_nk)^2) -- each flip is a rounding event of its own, modelled like the others as
    independent with a mean-free direction (Hoeffding: the same 2 exp(-LAMBDA^2 / 2) per inner product); it is the smaller of the
    two only where more than LAMBDA^2 = 49 operands of a row are candidates, i.e. for U"""
    worst = F @ w.abs().t()
    return worst if tier == "hard" else torch.minimum(worst, LAMBDA * torch.sqrt((F * F) @ (w * w).t()))


def _erf_factor(xc):
    """x P(x^2) of csrc/ppt_act.h, in xc's precision"""
    u = xc * xc
    p = torch.full_like(xc, _COEF[0]) * u + _COEF[1]
    for k in _COEF[2:]:
        p = p * u + k
    return p * xc


def gelu_poly3(x, hs=0.5):
    """csrc/mlp_fused3.hip gelu_poly3, in x's precision: the erf argument clamped to [-4, 4]; hs = half the DropPath factor"""
    e = _erf_factor(x.clamp(-4.0, 4.0))
    h = hs * x
    return h * e + h


def gelu_exact(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def _poly32(x):
    """the fp32 Horner evaluation's error in h e + h (docstring): 8 fma + the square + the product with x"""
    a = x.abs().clamp_max(4.0)
    s, p = torch.zeros_like(a), a.clone()
    for k in reversed(_COEF):
        s = s + abs(k) * p
        p = p * a * a
    return 18 * U * s * x.abs() / 2


def approx_term(x, variant):
    """|polynomial GELU - exact GELU| as the sources state it"""
    if variant == 3:
        return torch.where(x.abs() > 4.0, (x.abs() * CLAMP3 / 2).clamp_min(GELU_POLY_BOUND), torch.full_like(x, GELU_POLY_BOUND))
    return torch.full_like(x, GELU_POLY_BOUND)


def _gelu_stage(v, E, variant, gelu):
    """-> (value without the DropPath factor, E)"""
    w = gelu_exact(v) if gelu == "erf" else (gelu_poly3(v) if variant == 3 else gelu_poly(v))
    E = GELU_LIP * E + _poly32(v) + U * w.abs()
    if variant != 3:
        E = E + torch.where((v.abs() - 4.0).abs() <= E, 2 * GELU_POLY_BOUND, 0.0)
    if gelu == "erf":
        E = E + approx_term(v, variant)
    return w, E


def _per_row(slot, rows, M):
    return vec(slot).double()[torch.arange(M) // rows][:, None]


# ------------------------------------------------------------------------------------------------ the launches in fp64
def _chain(c, fmt, tier, gelu):
    """-> {output: (exact, tolerance)} of one tier (module docstring)"""
    I = inputs(c, fmt)
    dt, M = I.dt, c.M
    out = {}
    if c.kernel == "mlp":
        x = mat(I.x).double()
        Ex = torch.zeros_like(x)
        if c.proj:
            v, E = _prod(mat(I.pa).double(), None, I.Wp.double(), tier)
            if I.pb is not None:
                v = v + vec(I.pb).double()
                E = E + U * v.abs()
            if I.prs is not None:
                s1 = _per_row(I.prs, c.prs_rows, M)
                v = v * s1
                E = s1 * E + U * v.abs()
            x = x + v
            Ex = E + U * x.abs()
        L = _ln(x, Ex, vec(I.gam).double(), vec(I.bet).double(), tier)
        h, Fh = L["h"].to(dt).double(), _flip(L["h"], L["Eh"], dt)
        pre, Ep = _prod(h, Fh, I.W1.double(), tier)
        pre = pre + vec(I.b1).double()
        Ep = Ep + U * pre.abs()
        s = _per_row(I.rs, c.rs_rows, M) if I.rs is not None else torch.ones(M, 1, dtype=F64)
        g, Eg = _gelu_stage(pre, Ep, c.variant, gelu)
        W2, b2 = I.W2.double(), vec(I.b2).double()
        if c.variant == 3:
            uv, Eu = s * g, s * Eg + 2 * U * (s * g).abs()
            ur, Fu = uv.to(dt).double(), _flip(uv, Eu, dt)
            live = s != 0
            uw = (ur.abs() + Fu) @ W2.abs().t()
            E = Ex + _flipsum(Fu, W2, tier) + torch.where(live, _k(HID + 1, tier) * (x.abs() + uw), 0.0)
            v = x + ur @ W2.t() + b2 * s
            E = E + torch.where(live, U * v.abs(), 0.0)
        else:
            ur, Fu = g.to(dt).double(), _flip(g, Eg, dt)
            t, E = _prod(ur, Fu, W2, tier)
            t = t + b2
            E = E + U * t.abs()
            if I.rs is not None:
                t = t * s
                E = s * E + U * t.abs()
            v = x + t
            E = E + Ex + torch.where((s != 0) | (Ex > 0), U * v.abs(), 0.0)
        if I.res2 is not None:
            v = v + mat(I.res2).double()
            E = E + U * v.abs()
        out["out"] = (v, E + _store(v, E, torch.float32))
        return out
    W = I.W.double()
    if c.kernel == "lnlin" or c.form == "ln":
        L = _ln(mat(I.x).double(), torch.zeros(M, c.K, dtype=F64), vec(I.gam).double(), vec(I.bet).double(), tier)
        a, Fa = L["h"].to(dt).double(), _flip(L["h"], L["Eh"], dt)
        if c.ln_stats:
            out["mean"], out["rstd"] = (L["mean"][None], L["Em"][None]), (L["rstd"][None], L["Er"][None])
    else:
        a, Fa = mat(I.A).double(), None
    v, E = _prod(a, Fa, W, tier)
    if I.bias is not None:
        v = v + vec(I.bias).double()
        E = E + U * v.abs()
    if c.form == "res":
        if I.rs is not None:
            s = _per_row(I.rs, c.rs_rows, M)
            v = v * s
            E = s * E + U * v.abs()
        for r in (I.res, I.res2):
            if r is not None:
                v = v + mat(r).double()
                E = E + U * v.abs()
        out["C"] = (v, E + _store(v, E, torch.float32))
        return out
    if c.out2:
        out["out2"] = (v, E + _store(v, E, dt))
    if c.act == ACT_GELU:
        v, E = _gelu_stage(v, E, 2, gelu)
    elif c.act == ACT_QUICKGELU:
        w = v * torch.sigmoid(1.702 * v)
        E = 1.13 * E + U * (2 * (1 + 1.5 * v.abs()) * v.abs() + 4 * w.abs())
        v = w
    out["C"] = (v, E + _store(v, E, dt))
    return out


@functools.lru_cache(maxsize=4)
def reference(c, fmt, gelu="poly"):
    """-> {output: Ref(exact, hard tolerance, sharp tolerance)}, each [rows, columns] of the output's window"""
    hard, sharp = _chain(c, fmt, "hard", gelu), _chain(c, fmt, "sharp", gelu)
    return {k: Ref(hard[k][0], hard[k][1], sharp[k][1]) for k in hard}


def uses_gelu(c):
    return c.kernel == "mlp" or c.act == ACT_GELU


# ------------------------------------------------------------------------------------------------ the stand-in
MUTATIONS = ("drop_k_fc1", "drop_k_fc2", "drop_k_proj", "drop_k_rowblock", "ring_slip", "bias_next16", "rs_chunk_first", "rs_swapped",
             "res2_prev_row", "ragged_dup", "slice_neighbour", "var_single_pass", "eps_outside", "bf16_in_f16", "exact_gelu", "no_clamp")


def _mm32(a, w, drop_rows=None, slip=False):
    """fp32, K in 32-wide steps; drop_rows: bool [M], rows whose LAST k-step is left out; slip: k-step 1 takes the weights of k-step 0"""
    K = a.shape[1]
    v = torch.zeros(a.shape[0], w.shape[0])
    for k0 in range(0, K, 32):
        ak = a[:, k0:k0 + 32]
        if drop_rows is not None and k0 + 32 >= K:
            ak = ak * (~drop_rows)[:, None]
        kw = 0 if (slip and k0 == 32) else k0
        v = v + ak @ w[:, kw:kw + 32].t()
    return v


def _r16(t, dt, mutate):
    if mutate == "bf16_in_f16":
        assert dt == torch.float16
        t = t.to(torch.bfloat16).float()
    return t.to(dt)


def _ln32(x, g, b, dt, mutate):
    M, K = x.shape
    s16 = lambda t: t.view(M, 16, K // 16).sum(2).sum(1, keepdim=True)
    mean = s16(x) / K
    d = x - mean
    var = s16(x * x) / K - mean * mean if mutate == "var_single_pass" else s16(d * d) / K
    rstd = 1.0 / (torch.sqrt(var) + EPS) if mutate == "eps_outside" else 1.0 / torch.sqrt(var + EPS)
    return _r16(d * rstd * g + b, dt, mutate).float(), mean[:, 0], rstd[:, 0]


def _block_rows(c, rows_per):
    """bool [M]: the rows in the second 16-row block of their chunk / tile"""
    m = torch.arange(c.M)
    return (m % rows_per) // 16 == 1


def standin(c, fmt, mutate=None, cus=256):
    """the launch in fp32 -> {output name: tensor in the output's format, [rows, columns]}"""
    assert mutate is None or mutate in MUTATIONS
    I = inputs(c, fmt)
    dt, M = I.dt, c.M
    m = torch.arange(M)
    all_rows = torch.ones(M, dtype=torch.bool)
    prev = (m - 1).clamp_min(0)
    out = {}
    if c.kernel == "mlp":
        n_chunks, rpc, last, _ = case_geometry(c, cus)
        x = mat(I.x)
        sel = lambda slot, rows, idx=m: vec(slot)[idx // rows][:, None]
        first = (m // rpc) * rpc
        rs = sel(I.rs, c.rs_rows, first if mutate == "rs_chunk_first" else m) if I.rs is not None else None
        if c.proj:
            v = _mm32(mat(I.pa).float(), I.Wp.float(), all_rows if mutate == "drop_k_proj" else None)
            if I.pb is not None:
                v = v + vec(I.pb)
            if I.prs is not None:
                rs1 = sel(I.prs, c.prs_rows)
                if mutate == "rs_swapped":
                    assert rs is not None
                    rs, rs1 = rs1, rs
                v = v * rs1
            x = x + v
        else:
            assert mutate not in ("drop_k_proj", "rs_swapped")
        h = _ln32(x, vec(I.gam), vec(I.bet), dt, mutate if mutate in ("var_single_pass", "eps_outside", "bf16_in_f16") else None)[0]
        pre = _mm32(h, I.W1.float(), all_rows if mutate == "drop_k_fc1" else None) + vec(I.b1)
        if mutate == "exact_gelu":
            g = gelu_exact(pre)
        elif c.variant == 3:
            g = 0.5 * pre * _erf_factor(pre) + 0.5 * pre if mutate == "no_clamp" else gelu_poly3(pre)
        else:
            assert mutate != "no_clamp"
            g = gelu_poly(pre)
        b2 = vec(I.b2).roll(-16) if mutate == "bias_next16" else vec(I.b2)
        one = torch.ones(M, 1) if rs is None else rs
        u = (_r16(g * one, dt, None) if c.variant == 3 else _r16(g, dt, None)).float()
        if mutate == "ring_slip":
            u = u.clone()
            u[:, 128:256] = u[:, 0:128]
        drop = all_rows if mutate == "drop_k_fc2" else None
        if mutate == "drop_k_rowblock":
            assert rpc > 16
            drop = _block_rows(c, rpc)
        if c.variant == 3:
            v = x + _mm32(u, I.W2.float(), drop) + b2 * one
        else:
            t = _mm32(u, I.W2.float(), drop) + b2
            v = x + (t if rs is None else t * rs)
        if I.res2 is not None:
            v = v + (mat(I.res2)[prev] if mutate == "res2_prev_row" else mat(I.res2))
        else:
            assert mutate != "res2_prev_row"
        if mutate == "ragged_dup":
            assert M > 1
            v = v.clone()
            v[M - 1] = v[M - 2]
        out["out"] = v
        return out
    assert mutate not in ("drop_k_fc1", "drop_k_fc2", "drop_k_proj", "rs_swapped", "no_clamp")
    if c.kernel == "lnlin" or c.form == "ln":
        a, mean, rstd = _ln32(mat(I.x), vec(I.gam), vec(I.bet), dt, mutate)
        if c.ln_stats:
            out["mean"], out["rstd"] = mean[None], rstd[None]
    else:
        assert mutate not in ("var_single_pass", "eps_outside")
        a = mat(I.A).float()
    tile = 64 if c.kernel == "lnlin" else 32
    v = _mm32(a, I.W.float(), _block_rows(c, tile) if mutate == "drop_k_rowblock" else None, slip=mutate == "ring_slip")
    if I.bias is not None:
        v = v + (vec(I.bias).roll(-16) if mutate == "bias_next16" else vec(I.bias))
    else:
        assert mutate != "bias_next16"
    if c.form == "res":
        if I.rs is not None:
            idx = (m // 32) * 32 if mutate == "rs_chunk_first" else m
            v = v * vec(I.rs)[idx // c.rs_rows][:, None]
        else:
            assert mutate != "rs_chunk_first"
        v = v + mat(I.res)
        if I.res2 is not None:
            v = v + (mat(I.res2)[prev] if mutate == "res2_prev_row" else mat(I.res2))
        else:
            assert mutate != "res2_prev_row"
    else:
        assert mutate not in ("rs_chunk_first", "res2_prev_row")
        if c.out2:
            out["out2"] = _r16(v, dt, mutate)
        if c.act == ACT_GELU:
            v = gelu_exact(v) if mutate == "exact_gelu" else gelu_poly(v)
        elif c.act == ACT_QUICKGELU:
            v = v / (1.0 + torch.exp(-1.702 * v))
        assert mutate != "exact_gelu" or c.act == ACT_GELU
        v = _r16(v, dt, mutate)
    if mutate == "ragged_dup":
        assert M > 1
        v = v.clone()
        v[M - 1] = v[M - 2]
    if mutate == "slice_neighbour":
        assert c.kernel == "lnlin" and c.N >= 768
        v = torch.cat([v[:, 384:768], v[:, :384], v[:, 768:]], 1)
    out["C"] = v
    return out


# ------------------------------------------------------------------------------------------------ the criterion
def cap(M):
    """rows per (case, output) that may miss the sharp bound"""
    return M // 20


Verdict = collections.namedtuple("Verdict", "hard at sharp over rows")


STATS = ("mean", "rstd")


def _orient(t, name):
    """ln_stats ([1, M]) -> [M, 1]: every entry is a row's and is judged as one; every other output stays [rows, columns]"""
    return t.t() if name in STATS else t


def judge(x, ref, name="C"):
    """x [rows, columns] against a Ref -> Verdict(worst hard ratio, its (row, column), worst sharp ratio, rows over the sharp
    bound, which rows).  NaN counts as infinite.  The ln_stats outputs (`name` in STATS, [1, M]) are judged per element."""
    err = (x.double() - ref.exact).abs()

    def ratio(tol):
        r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
        return torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)

    rh, rs = _orient(ratio(ref.hard), name), _orient(ratio(ref.sharp), name)
    i = int(rh.argmax())
    rows = rs.amax(1)
    bad = torch.nonzero(rows > 1.0)[:, 0].tolist()
    return Verdict(float(rh.reshape(-1)[i]), (i // rh.shape[1], i % rh.shape[1]), float(rows.max()), len(bad), bad)


def describe(c, fmt, cus=256):
    s = f"{case_id(c)} {fmt} [{family(c)}]"
    if c.kernel == "mlp":
        s += " (n_chunks, rows_per_chunk, last chunk, chunks per workgroup) = " + str(case_geometry(c, cus))
    return s + f" ({c.note})"


def check(c, fmt, result, errors=None, what="VIT", gelu="poly", cus=256):
    """result {name: [rows, columns]} against reference(c, fmt, gelu) -> {name: Verdict}; appends what fails to `errors`; prints
    output=hard ratio@row.column/sharp ratio/rows over the sharp bound (and every such row)"""
    ref, res = reference(c, fmt, gelu), {}
    assert set(result) == set(ref), (sorted(result), sorted(ref))
    n = c.M
    for name, x in result.items():
        v = res[name] = judge(x, ref[name], name)
        if errors is not None and not v.hard <= 1.0:
            errors.append(f"{describe(c, fmt, cus)} {name} [{gelu}]: HARD bound: |x - exact| / tol = {v.hard:.3g} > 1 at (row, column) {v.at}: "
                          f"x {float(_orient(x, name)[v.at]):.6g}, exact {float(_orient(ref[name].exact, name)[v.at]):.6g}, "
                          f"tol {float(_orient(ref[name].hard, name)[v.at]):.3g}")
        if errors is not None and v.over > cap(n):
            errors.append(f"{describe(c, fmt, cus)} {name} [{gelu}]: SHARP bound: {v.over} rows over, {cap(n)} allowed; worst ratio "
                          f"{v.sharp:.3g}; rows {v.rows[:12]}")
    print(f"{what} {case_id(c)} {fmt} {gelu} " + " ".join(
        f"{k}={v.hard:.3f}@{v.at[0]}.{v.at[1]}/{v.sharp:.3f}/{v.over}" + (f"{v.rows}" if v.over else "") for k, v in res.items()))
    return res


# ------------------------------------------------------------------------------------------------ the cases
def _cases():
    cs = []
    mlp = lambda M, wg, note, **kw: [Case("mlp", M, D, D, variant=v, workgroups=wg, note=note, **kw) for v in (2, 3)]
    full = dict(rs_rows=13, zeros=True, res2=True, proj="wbs", prs_rows=11)
    # A. vit_mlp chunk geometry through workgroups=: each with every epilogue operand (DropPath factors with exact zeros, sample
    # boundaries of 13 / 11 rows inside the row blocks), and bare
    geo = [(2, 2, "rows_per_chunk 1"), (2, 30, "rows_per_chunk 15"), (2, 32, "rows_per_chunk 16: whole row blocks"),
           (2, 33, "rows_per_chunk 17: one row in the second row block; last chunk one row block shorter"),
           (2, 64, "rows_per_chunk 32"), (2, 96, "rows_per_chunk 48"), (2, 128, "rows_per_chunk 64"),
           (2, 129, "rows_per_chunk 65; last chunk one row block shorter"), (2, 158, "rows_per_chunk 79"),
           (2, 160, "rows_per_chunk 80: full chunks"), (1, 81, "two chunks per workgroup, 41 + 40"),
           (2, 331, "three chunks per workgroup: six chunks of 56, last 51"), (4, 9, "n_chunks shrunk by the second division"),
           (8, 57, "last chunk of one row"), (0, 77, "default grid: one row per chunk on any part with >= 77 CUs")]
    for wg, M, note in geo:
        cs += mlp(M, wg, note, **full)
        if M in (2, 33, 129, 160, 81, 331, 57, 77):
            cs += mlp(M, wg, note + "; bare")
    for M in (160, 513):
        cs += mlp(M, 0, "persistent_occupancy(50): as few workgroups as the rounds allow, full chunks", occupancy=50, **full)
        cs += mlp(M, 0, "persistent_occupancy(50); bare", occupancy=50)
    # B. vit_mlp operands, on the three-chunk loop (rows_per_chunk 56)
    for kw, note in ((dict(rs_rows=56, zeros=True), "sample boundary AT the chunk boundary"),
                     (dict(rs_rows=37, zeros=True), "sample boundaries inside row blocks and in the ragged chunk"),
                     (dict(rs_rows=37), "factors without zeros"), (dict(res2=True), "residual2 alone"),
                     (dict(proj="w"), "proj prologue, weight only"), (dict(proj="wb"), "proj prologue with bias"),
                     (dict(proj="wbs", prs_rows=37, rs_rows=56, zeros=True), "both branches' factors, different sample sizes"),
                     (dict(inplace=True, rs_rows=37, res2=True), "in place"), (dict(inplace=True, **full), "in place, proj prologue")):
        cs += mlp(331, 2, note, **kw)
    # C. input families
    for fam in ("mean30", "const", "wide", "outlier"):
        cs += mlp(19, 1, "input family, M < 20: no row may miss the sharp bound", family=fam, rs_rows=7)
        cs += mlp(81, 1, "input family, two chunks", family=fam, **full)
    # D. lnlin
    ln = lambda M, N, note, **kw: Case("lnlin", M, N, D, note=note, **kw)
    notes = {1: "one row", 31: "one LayerNorm pass, ragged", 32: "one LayerNorm pass", 33: "second pass of one row", 63: "ragged chunk",
             64: "one whole chunk", 65: "second chunk of one row", 512: "8 chunks: no idle workgroup", 513: "9 chunks: 7 idle workgroups return",
             577: "10 chunks, ragged"}
    for M, note in notes.items():                  # every M x 1 / 2 / 3 slices x with and without bias
        cs += [ln(M, 384 * s, f"{note}; {s} slice{'s' * (s > 1)}", bias=b) for s in (1, 2, 3) for b in (False, True)]
    for fam in ("mean30", "const", "outlier"):
        cs += [ln(19, 768, "input family, M < 20", family=fam, bias=True), ln(70, 384, "input family", family=fam)]
    # E. rowgemm
    rg = lambda M, N, K, form, note, **kw: Case("rowgemm", M, N, K, form=form, note=note, **kw)
    wk = "walkers=8 over 25 tiles: seven walkers take three tiles, one takes four"
    cs += [rg(787, 392, 384, "16", wk, walkers=8, bias=True, act=ACT_GELU, out2=True),
           rg(787, 264, 512, "16", wk, walkers=8, act=ACT_QUICKGELU, out2=True),
           rg(787, 392, 384, "ln", wk, walkers=8, bias=True, act=ACT_GELU, ln_stats=True),
           rg(787, 388, 384, "res", wk, walkers=8, bias=True, rs_rows=37, zeros=True, res2=True),
           rg(787, 516, 512, "res", wk, walkers=8, inplace=True)]
    for M in (1, 31, 32, 33, 65):
        e = f"M = {M}: tile edge"
        cs += [rg(M, 8, 384, "16", e + ", N = 8"), rg(M, 200, 384, "16", e + ", N no whole column group", bias=True),
               rg(M, 384, 384, "16", e + ", whole column groups only: no weight row clamped", bias=True, act=ACT_GELU, out2=True),
               rg(M, 392, 384, "16", e + ", one column group and 8 columns of the next", act=ACT_QUICKGELU),
               rg(M, 264, 512, "16", e + ", one column group and 8 columns of the next", bias=True),
               rg(M, 8, 512, "16", e, bias=True, act=ACT_GELU), rg(M, 256, 512, "16", e + ", one whole column group", act=ACT_QUICKGELU, out2=True),
               rg(M, 384, 384, "ln", e, ln_stats=True), rg(M, 264, 512, "ln", e, bias=True, act=ACT_GELU, out2=True),
               rg(M, 4, 384, "res", e + ", N = 4"), rg(M, 516, 512, "res", e + ", N % 8 = 4", bias=True, rs_rows=7, zeros=True, res2=True)]
    for K, N, form in ((384, 392, "16"), (512, 264, "ln"), (512, 264, "16"), (384, 392, "ln")):
        for act in (ACT_NONE, ACT_GELU, ACT_QUICKGELU):
            for o2 in ((False,) if act == ACT_NONE else (False, True)):
                for b in ((False, True) if act == ACT_NONE else (True,)):
                    cs.append(rg(65, N, K, form, "activation table", act=act, out2=o2, bias=b, ln_stats=(form == "ln" and not o2)))
    for rs in (0, 7):
        for r2 in (False, True):
            for ip in (False, True):
                cs.append(rg(65, 388, 384, "res", "residual table", bias=True, rs_rows=rs, zeros=bool(rs), res2=r2, inplace=ip))
    for fam in ("mean30", "const", "outlier", "wide"):
        cs += [rg(19, 392, 384, "ln", "input family, M < 20", family=fam, bias=True, act=ACT_GELU, ln_stats=True),
               rg(70, 264, 512, "ln", "input family", family=fam, ln_stats=True)]
    cs += [rg(70, 392, 384, "16", "pre-activations beyond |4|", family="wide", bias=True, act=ACT_GELU),
           rg(70, 264, 512, "16", "pre-activations beyond |4|", family="wide", bias=True, act=ACT_GELU, out2=True),
           rg(70, 392, 384, "16", "GELU arguments over [-4, 4] under a small product", family="bias", bias=True, act=ACT_GELU),
           rg(70, 264, 512, "16", "GELU arguments over [-4, 4] under a small product", family="bias", bias=True, act=ACT_GELU, out2=True)]
    seen = set()                                   # (the tables overlap in a few entries: each case once)
    return [c for c in cs if not (case_id(c) in seen or seen.add(case_id(c)))]


CASES = _cases()
assert len({case_id(c) for c in CASES}) == len(CASES)
FMTS = ("bf16", "f16")
RUNS = [(c, f) for c in CASES for f in FMTS]
BY_ID = {case_id(c): c for c in CASES}


def run_id(r):
    return f"{case_id(r[0])}-{r[1]}"


def coverage(cus=256):
    """what the vit_mlp table reaches, for the assertions of the CPU test (and of the GPU test with the device's CU count)"""
    g = [(c, case_geometry(c, cus)) for c in CASES if c.kernel == "mlp"]
    blocks = lambda n: (n + 15) // 16
    return dict(rows_per_chunk={x[1] for _, x in g}, last_one_row=any(x[2] == 1 and x[0] > 1 for _, x in g),
                last_block_shorter=any(x[0] > 1 and blocks(x[2]) == blocks(x[1]) - 1 for _, x in g),
                chunks_per_workgroup={x[3] for _, x in g},
                second_division=any(c.workgroups > 0 and x[0] < c.workgroups and c.M >= c.workgroups for c, x in g),
                occupancy={(c.M, x[1]) for c, x in g if c.occupancy < 100},
                boundary_in_block=any(c.rs_rows and c.rs_rows % 16 for c, _ in g),
                boundary_at_chunk=any(c.rs_rows == x[1] and x[0] > 1 for c, x in g),
                boundary_in_ragged=any(c.rs_rows and x[2] < x[1] and (c.M - 1) // c.rs_rows > (c.M - x[2]) // c.rs_rows for c, x in g),
                zeros=any(c.zeros for c, _ in g))


def _assert_coverage():
    cov = coverage()
    assert {1, 15, 16, 17, 32, 48, 64, 65, 79, 80} <= cov["rows_per_chunk"] and {1, 2, 3} <= cov["chunks_per_workgroup"], cov
    assert cov["last_one_row"] and cov["last_block_shorter"] and cov["second_division"] and cov["occupancy"] == {(160, 80), (513, 74)}, cov
    assert cov["boundary_in_block"] and cov["boundary_at_chunk"] and cov["boundary_in_ragged"] and cov["zeros"], cov


_assert_coverage()


# ------------------------------------------------------------------------------------------------ refusals (the host functions)
EINVAL, EUNSUPPORTED = -1, -3
# (kernel, name, {field: value}, expected code).  Values: an int; ("null",) the field cleared; ("off", bytes) the field's pointer
# moved; ("buf", name) another tensor of the base launch.  The base launches are valid (the GPU test runs them first).
REFUSALS = [
    ("lnlin", "K-not-384", dict(K=512), EUNSUPPORTED), ("lnlin", "N-not-a-slice", dict(N=392), EUNSUPPORTED),
    ("lnlin", "M-zero", dict(M=0), EINVAL), ("lnlin", "M-negative", dict(M=-3), EINVAL), ("lnlin", "dtype-fp32", dict(dtype=0), EINVAL),
    ("lnlin", "dtype-unknown", dict(dtype=3), EINVAL), ("lnlin", "no-ln-weight", dict(ln_w=("null",)), EINVAL),
] + [("lnlin", f"{f}-misaligned", {f: ("off", 8)}, EINVAL) for f in ("x", "W", "C", "ln_w", "ln_b", "bias")] + [
    ("mlp", "D-not-384", dict(D=512), EUNSUPPORTED), ("mlp", "hidden-not-1536", dict(hidden=2048), EUNSUPPORTED),
    ("mlp", "M-zero", dict(M=0), EINVAL), ("mlp", "dtype-unknown", dict(dtype=3), EINVAL),
    ("mlp", "row-scale-rows-0", dict(row_scale=("buf", "rs"), row_scale_rows=0), EINVAL),
    ("mlp", "proj-row-scale-rows-0", dict(proj_a=("buf", "pa"), proj_W=("buf", "wp"), proj_row_scale=("buf", "rs"), proj_row_scale_rows=0), EINVAL),
    ("mlp", "proj-without-weight", dict(proj_a=("buf", "pa")), EINVAL), ("mlp", "no-ln-bias", dict(ln_b=("null",)), EINVAL),
    ("mlp", "proj-a-misaligned", dict(proj_a=("buf+", "pa", 8), proj_W=("buf", "wp")), EINVAL),
    ("mlp", "proj-W-misaligned", dict(proj_a=("buf", "pa"), proj_W=("buf+", "wp", 8)), EINVAL),
    ("mlp", "proj-b-misaligned", dict(proj_a=("buf", "pa"), proj_W=("buf", "wp"), proj_b=("buf+", "rs", 4)), EINVAL),
    ("mlp", "residual2-misaligned", dict(residual2=("buf+", "r2", 8)), EINVAL),
] + [("mlp", f"{f}-misaligned", {f: ("off", 8)}, EINVAL) for f in ("x", "out", "W1", "W2")] + [
    ("rowgemm", "K-256", dict(K=256), EUNSUPPORTED), ("rowgemm", "N-not-8", dict(N=388), EUNSUPPORTED),
    ("rowgemm", "residual-N-not-4", dict(N=390, residual_form=1, residual=("buf", "res")), EUNSUPPORTED),
    ("rowgemm", "M-zero", dict(M=0), EINVAL), ("rowgemm", "N-zero", dict(N=0), EINVAL), ("rowgemm", "dtype-unknown", dict(dtype=3), EINVAL),
    ("rowgemm", "row-scale-rows-0", dict(residual_form=1, residual=("buf", "res"), row_scale=("buf", "rs"), row_scale_rows=0), EINVAL),
    ("rowgemm", "ln-without-weights", dict(a_ln=1), EINVAL),
    ("rowgemm", "ln-mean-without-rstd", dict(ln_mean=("buf", "st")), EINVAL),
    ("rowgemm", "residual-form-without-residual", dict(residual_form=1), EINVAL),
    ("rowgemm", "residual-form-with-ln", dict(residual_form=1, residual=("buf", "res"), a_ln=1, ln_w=("buf", "g"), ln_b=("buf", "g")), EUNSUPPORTED),
    ("rowgemm", "residual-form-with-activation", dict(residual_form=1, residual=("buf", "res"), act=ACT_GELU), EUNSUPPORTED),
    ("rowgemm", "residual-form-with-C2", dict(residual_form=1, residual=("buf", "res"), C2=("buf", "c2")), EUNSUPPORTED),
    ("rowgemm", "C2-without-activation", dict(C2=("buf", "c2")), EUNSUPPORTED), ("rowgemm", "activation-relu", dict(act=1), EUNSUPPORTED),
    ("rowgemm", "C2-misaligned", dict(act=ACT_GELU, C2=("buf+", "c2", 8)), EINVAL),
    ("rowgemm", "residual-misaligned", dict(residual_form=1, residual=("buf+", "res", 8)), EINVAL),
    ("rowgemm", "residual2-misaligned", dict(residual_form=1, residual=("buf", "res"), residual2=("buf+", "res", 8)), EINVAL),
] + [("rowgemm", f"{f}-misaligned", {f: ("off", 8)}, EINVAL) for f in ("A", "W", "C")]
