"""Shared by tests/test_gemm_ref_cpu.py and tests/test_gemm_gpu.py: ppt_gemm / ppt_gemm256 (include/ppt_hip.h, csrc/gemm.hip,
csrc/gemm256.hip) in plain torch on the CPU (no ppt_amd import), the case table, and the criterion that compares a kernel's
result with the reference.

  reference  the whole launch in fp64 on the operands' STORED values (16-bit and fp32 inputs convert exactly), every output
             with its elementwise a-priori bound -> {output: (exact, tol)}.  exact() / tol() return the two halves.
  standin    the same launch in fp32 in ANOTHER summation order (K in 16-wide steps): a correct kernel's proxy for the CPU test;
             `mutate` (MUTATIONS) breaks it on purpose.
  worst      max |x - exact| / tol and its index; a result passes iff that is <= 1 and nothing is NaN.  tol = E + R: E what the
             arithmetic may err, R the half ulp of the store.

Order of a launch: A prologue, product, + bias, + group_add[m / group_rows], [statistics; out2 when out2_pre], activation or
* act'(dact_pre), * row_scale[m / row_scale_rows], + residual, + residual2, C, [out2 otherwise], pools of that value.

The bound (u = 2^-24; E is carried through the stages; nothing in it is measured):
  product      E = k u (|A| |B|^T)_ij, k = K for 16-bit operands (their products are exact in fp32) and K + 1 for fp32: any order.
  each fp32 +  E += u |v|                                                  (bias, group term, residuals)
  activation   E = L E + approx + u (c |v| + c' |act(v)|), c' = 1 (GELU) / 3 (QuickGELU: sum, reciprocal, product),
               L = 1 (ReLU) / 1.13 (GELU, QuickGELU: sup |act'|).  approx: gelu_poly's
               2e-4 (csrc/ppt_act.h) where the 16-bit register / vec8 tiers run it.  c = 4 for GELU (0.5 v (1 + erf(v / sqrt 2)):
               the argument's two roundings reach erf as <= u, erff <= 2 u, the sum 2 u, the product u, all times |v / 2|) and
               c = 1 + 1.5 |v| for QuickGELU (v / (1 + e), e = exp2(-1.702 log2(e) v): the argument's roundings are a relative
               (2 + 5 |v|) u of e, and |d out / d e| e <= |v| / 4).
  derivative   E = |act'(x)| E + |v| D + u |v act'(x)|, D = 8 u (+ 0.5 * 1.5e-7 for erf_fast) for GELU, (8 + 8 |x|) u for
               QuickGELU, 0 for ReLU: x is a stored value, only the evaluation of act' errs.
  row scale    E = |s| E + u |v|
  store        tol = E + half an ulp of the format at |v| + E: r 2^floor(log2(|v| + E)), r = 2^-8 / 2^-11 / 2^-24 for bf16 / fp16 /
               fp32 (between r / 2 and r of the value: a value just above a power of two is a full r of itself away from its
               neighbour's midpoint), + 2^-25 for fp16 (its subnormal spacing)
  pools        |max a - max b| <= max |a - b|: the largest E of the pool's rows, then the store term of the pool's format
  statistics   sum: the sum of its rows' E + n u sum |v| (n rows of a chunk, any order).  M2: sum_r 2 |d_r| (E_r + E_mean)
               + (E_r + E_mean)^2, + (n + 4) u M2 for its own fp32 subtraction, square and sum; E_mean = tol(sum) / n + u |mean|.
The A prologues are defined as fp32 operations rounded to the operand format (relu(fma(a, scale, shift)); the first conv as
fma(wz', z, fma(wy', y, fma(wx', x, b'))) on the BatchNorm-folded constants): prologue() reproduces those roundings, so a' is an
operand like any other and adds nothing to the bound.
"""
import collections
import functools
import math
import zlib

import torch

A_PLAIN, A_AFFINE_RELU, A_CONV1 = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_GELU, ACT_QUICKGELU = 0, 1, 2, 3
FMT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
ROUND = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}      # half an ulp of a value in [1, 2)
U = 2.0 ** -24
GELU_POLY_BOUND, ERF_FAST_BOUND = 2e-4, 1.5e-7           # what csrc/ppt_act.h states; test_gemm_ref_cpu.py pins both
SENTINEL = {4: 0x5EA7C0DE, 2: 0x5EA7}                    # finite in every format; by element size

_FIELDS = dict(group="", M=0, N=0, K=0, k32=0, fmts=("bf16", "f16", "f32"), a_mode=A_PLAIN, c="f32", ldc_pad=0, c_off=0, ld_pad=8,
               bias=False, bias_off=0, act=ACT_NONE, group_rows=0, group_off=0, rs_rows=0, res=False, res2=False, dact=False,
               out2="", out2_pre=False, stats=False, pool="", pool_rows=0, pool_min=False, batch=1, strideB=False, zc_extra=0,
               core="", tier="", note="", expect="ok")
Case = collections.namedtuple("Case", list(_FIELDS), defaults=list(_FIELDS.values()))
Slot = collections.namedtuple("Slot", "buf off rows cols ld zs nz")          # a [nz, rows, cols] window of a flat buffer
Inputs = collections.namedtuple("Inputs", "K dt A B bias group row_scale res res2 dact a_scale a_shift pts w1 b1 outs")


def case_id(c):
    s = f"{c.group}-{c.M}x{c.N}x{c.K}"
    for k, d in _FIELDS.items():
        v = getattr(c, k)
        if k in ("group", "M", "N", "K", "k32", "fmts", "note", "tier", "ld_pad") or v == d:
            continue
        s += f"-{k}" if v is True else f"-{k}{v}"
    return s + f"-{c.tier}"


def kdim(c, fmt):
    return c.k32 if (fmt == "f32" and c.k32) else c.K


def family(c, fmt):
    """the kernel a case is expected to run (for the failure messages; the shapes choose, csrc/gemm.hip launch_gemm)"""
    K, plain = kdim(c, fmt), c.a_mode == A_PLAIN
    if c.core == "256":
        return "gemm256_kernel"
    t128 = ((c.N + 127) // 128) * ((c.M + 127) // 128) * c.batch
    if plain and t128 >= 768 and K % (16 if fmt == "f32" else 32) == 0 and c.tier == "regs":
        return "gemm_kernel_glds_h<128, 128>"
    if c.stats or c.pool:
        return "gemm_kernel<128, 128>"
    return "gemm_kernel_glds<64, 64>" if plain and K % (32 if fmt == "f32" else 64) == 0 else "gemm_kernel<64, 64>"


# ------------------------------------------------------------------------------------------------ inputs
def view(s, buf=None, z=None):
    """the window of a slot inside `buf` (the slot's own buffer, or a copy of it on another device): [rows, cols] of slice z,
    or all slices [nz, rows, cols]"""
    buf = s.buf if buf is None else buf
    if z is None:
        return buf.as_strided((s.nz, s.rows, s.cols), (s.zs, s.ld, 1), s.off)
    return buf.as_strided((s.rows, s.cols), (s.ld, 1), s.off + z * s.zs)


def _slot_in(vals, ld, off, zs=None):
    """vals [nz, rows, cols] -> a slot whose buffer holds NaN in front of the window, in the padding columns, between the slices
    and in one more row behind it"""
    nz, rows, cols = vals.shape
    zs = rows * ld if zs is None else zs
    buf = torch.full((off + (nz - 1) * zs + (rows + 1) * ld,), float("nan"), dtype=vals.dtype)
    s = Slot(buf, off, rows, cols, ld, zs, nz)
    view(s).copy_(vals)
    return s


def _slot_out(dt, nz, rows, cols, ld, off, zs=None):
    zs = rows * ld if zs is None else zs
    buf = torch.empty((off + (nz - 1) * zs + (rows + 1) * ld + 16,), dtype=dt)
    buf.view(torch.int32 if buf.element_size() == 4 else torch.int16).fill_(_sentinel(dt))
    return Slot(buf, off, rows, cols, ld, zs, nz)


def _sentinel(dt):
    return SENTINEL[torch.empty((), dtype=dt).element_size()]


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def outside_intact(s, buf):
    """every element of `buf` outside the slot's window still holds the sentinel"""
    inside = torch.zeros(buf.numel(), dtype=torch.bool)
    view(s, inside).fill_(True)
    return bool((bits(buf.cpu())[~inside] == _sentinel(buf.dtype)).all())


def untouched(s, buf):
    return bool((bits(buf.cpu()) == _sentinel(buf.dtype)).all())


def any_sentinel_inside(s, buf):
    return bool((bits(view(s, buf.cpu()).contiguous()) == _sentinel(buf.dtype)).any())


def _odt(kind, dt):
    return torch.float32 if kind == "f32" or dt == torch.float32 else dt


@functools.lru_cache(maxsize=3)
def inputs(c, fmt):
    """every operand of a case as a window inside a NaN-padded buffer, every output as a window inside a sentinel-filled one;
    seeded per (case, format)"""
    gen = torch.Generator().manual_seed(zlib.crc32((case_id(c) + fmt).encode()))
    rn = lambda *s: torch.randn(*s, generator=gen)
    dt, K, M, N, nz = FMT[fmt], kdim(c, fmt), c.M, c.N, c.batch
    pad = c.ld_pad
    A = _slot_in(rn(nz, M, K).to(dt), K + pad, 16) if c.a_mode != A_CONV1 else None
    B = _slot_in((rn(nz if c.strideB else 1, N, K) / math.sqrt(K)).to(dt), K + pad, 16)
    bias = _slot_in(rn(1, 1, N), N, c.bias_off) if c.bias else None
    ng = (M + c.group_rows - 1) // c.group_rows if c.group_rows else 0
    group = _slot_in(rn(1, ng, N), N, c.group_off) if ng else None
    nrs = (M + c.rs_rows - 1) // c.rs_rows if c.rs_rows else 0
    row_scale = _slot_in(0.5 + torch.rand(1, 1, nrs, generator=gen), nrs, 0) if nrs else None
    res = _slot_in(rn(1, M, N), N + 8, 16) if c.res else None
    res2 = _slot_in(rn(1, M, N), N + 16, 16) if c.res2 else None
    dact = _slot_in((1.5 * rn(1, M, N)).to(dt), N + 8, 16) if c.dact else None
    pro = c.a_mode != A_PLAIN
    a_scale, a_shift = (rn(K), rn(K)) if pro else (None, None)
    pts, w1, b1 = (rn(M, 3), rn(K, 3), rn(K)) if c.a_mode == A_CONV1 else (None, None, None)
    outs = {}
    if c.c != "none":
        ldc = N + c.ldc_pad
        outs["C"] = _slot_out(_odt(c.c, dt), nz, M, N, ldc, c.c_off, M * ldc + c.zc_extra)
    if c.out2:
        outs["out2"] = _slot_out(_odt(c.out2, dt), 1, M, N, N + 8, 16)
    if c.stats:
        outs["col_sum"] = _slot_out(torch.float32, 1, (M + 31) // 32, N, N, 16)
        outs["col_sqsum"] = _slot_out(torch.float32, 1, (M + 31) // 32, N, N, 16)
    if c.pool:
        pr = c.pool_rows or 32
        outs["pool_max"] = _slot_out(_odt(c.pool, dt), 1, (M + pr - 1) // pr, N, N, 16)
        if c.pool_min:
            outs["pool_min"] = _slot_out(_odt(c.pool, dt), 1, (M + pr - 1) // pr, N, N, 16)
    return Inputs(K, dt, A, B, bias, group, row_scale, res, res2, dact, a_scale, a_shift, pts, w1, b1, outs)


# ------------------------------------------------------------------------------------------------ the launch
def _fma32(a, b, c):
    """fmaf on fp32 values: the fp64 product of two floats is exact, the sum rounds once more at 2^-53 -- below anything here"""
    return (a.double() * b.double() + c.double()).float()


def prologue(c, I):
    """A as the tile loops see it, [nz, M, K] in the operand format (module docstring)"""
    if c.a_mode == A_PLAIN:
        return view(I.A)
    if c.a_mode == A_AFFINE_RELU:
        return _fma32(view(I.A).float(), I.a_scale, I.a_shift).clamp_min(0).to(I.dt)
    s, h = I.a_scale, I.a_shift
    w = (s[:, None] * I.w1)                                              # fp32 products, as the LDS table holds them
    wb = _fma32(s, I.b1, h)
    x, y, z = I.pts[:, 0:1], I.pts[:, 1:2], I.pts[:, 2:3]
    f = _fma32(w[:, 2][None], z, _fma32(w[:, 1][None], y, _fma32(w[:, 0][None], x, wb[None].expand(c.M, -1))))
    return f.clamp_min(0).to(I.dt)[None]


def _act(v, act):
    if act == ACT_RELU:
        return v.clamp_min(0)
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v * 0.7071067811865476))
    if act == ACT_QUICKGELU:
        return v * torch.sigmoid(1.702 * v)
    return v


def _dact(x, act):
    if act == ACT_RELU:
        return (x > 0).to(x.dtype)
    if act == ACT_GELU:
        return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)
    if act == ACT_QUICKGELU:
        s = torch.sigmoid(1.702 * x)
        return s * (1.0 + 1.702 * x * (1.0 - s))
    return torch.ones_like(x)


def _chunks(t, n, fill):
    """[M, N] -> ([ceil(M / n), n, N] padded with `fill`, the same shape of bool: row exists)"""
    M, N = t.shape
    g = (M + n - 1) // n
    p = torch.full((g * n, N), fill, dtype=t.dtype)
    p[:M] = t
    ok = (torch.arange(g * n) < M).view(g, n, 1)
    return p.view(g, n, N), ok


def _stats(v):
    ch, ok = _chunks(v, 32, 0.0)
    cnt = ok.sum(1).to(v.dtype)
    s = ch.sum(1)
    d = (ch - (s / cnt)[:, None]) * ok
    return s, (d * d).sum(1), ch, d, cnt, ok


def _fast16(c, fmt):
    return fmt != "f32" and c.tier != "scalar"


@functools.lru_cache(maxsize=2)
def reference(c, fmt):
    """-> {output name: (exact, E, R)} of a case in fp64, shaped as the output's window [nz, rows, cols]: tol = E + R, R the
    store's half ulp (module docstring)"""
    I = inputs(c, fmt)
    D = torch.float64
    a = prologue(c, I).to(D)
    b = view(I.B).to(D)
    v = a @ b.transpose(-1, -2)                                           # [nz, M, N] (B broadcasts when strideB == 0)
    E = (I.K + (1 if fmt == "f32" else 0)) * U * (a.abs() @ b.abs().transpose(-1, -2))
    del a, b
    out = {}
    if c.bias:
        v = v + view(I.bias, z=0).to(D)
        E = E + U * v.abs()
    if c.group_rows:
        v = v + view(I.group, z=0).to(D)[torch.arange(c.M) // c.group_rows]
        E = E + U * v.abs()
    if c.stats:
        s, m2, ch, d, cnt, ok = _stats(v[0])
        Ec, _ = _chunks(E[0], 32, 0.0)
        ts = Ec.sum(1) + cnt * U * ch.abs().sum(1)
        em = ts / cnt + U * (s / cnt).abs()
        er = Ec + em[:, None]
        out["col_sum"] = (s[None], ts[None], 0.0)
        out["col_sqsum"] = (m2[None], (((2 * d.abs() * er + er * er) * ok).sum(1) + (cnt + 4) * U * m2)[None], 0.0)

    def store(val, err, dt):
        top = (val.abs() + err).clamp_min(1e-300)
        return err, ROUND[dt] * torch.exp2(torch.floor(torch.log2(top))) + (2.0 ** -25 if dt == torch.float16 else 0.0)

    if c.out2 and c.out2_pre:
        out["out2"] = (v,) + store(v, E, I.outs["out2"].buf.dtype)
    if c.dact:
        x = view(I.dact, z=0).to(D)
        g = _dact(x, c.act)
        Dv = {ACT_GELU: 8 * U + (0.5 * ERF_FAST_BOUND if _fast16(c, fmt) else 0.0), ACT_QUICKGELU: (8 + 8 * x.abs()) * U}.get(c.act, 0.0)
        E = g.abs() * E + v.abs() * Dv + U * (v * g).abs()
        v = v * g
    elif c.act != ACT_NONE:
        w = _act(v, c.act)
        if c.act == ACT_RELU:
            pass
        elif c.act == ACT_GELU:
            E = 1.13 * E + (GELU_POLY_BOUND if _fast16(c, fmt) else 0.0) + U * (4 * v.abs() + w.abs())
        else:
            E = 1.13 * E + U * ((1 + 1.5 * v.abs()) * v.abs() + 3 * w.abs())
        v = w
    if c.rs_rows:
        s = view(I.row_scale, z=0).to(D)[0][torch.arange(c.M) // c.rs_rows][:, None]
        v = v * s
        E = s.abs() * E + U * v.abs()
    for r in (I.res, I.res2):
        if r is not None:
            v = v + view(r, z=0).to(D)
            E = E + U * v.abs()
    if c.c != "none":
        out["C"] = (v,) + store(v, E, I.outs["C"].buf.dtype)
    if c.out2 and not c.out2_pre:
        out["out2"] = (v,) + store(v, E, I.outs["out2"].buf.dtype)
    if c.pool:
        pr, pdt = c.pool_rows or 32, I.outs["pool_max"].buf.dtype
        Ep = _chunks(E[0], pr, 0.0)[0].amax(1)
        mx = _chunks(v[0], pr, float("-inf"))[0].amax(1)
        out["pool_max"] = (mx[None],) + tuple(t[None] for t in store(mx, Ep, pdt))
        if c.pool_min:
            mn = _chunks(v[0], pr, float("inf"))[0].amin(1)
            out["pool_min"] = (mn[None],) + tuple(t[None] for t in store(mn, Ep, pdt))
    return out


def exact(c, fmt):
    return {k: v[0] for k, v in reference(c, fmt).items()}


def tol(c, fmt):
    return {k: v[1] + v[2] for k, v in reference(c, fmt).items()}


MUTATIONS = ("drop_k_last", "drop_slab", "double_surplus", "bias_next_col", "group_neighbour", "row_scale_next", "res_ldc",
             "act_before_bias", "out2_wrong_side", "stats_after_act", "pool_beyond_m", "stale_last_row", "bf16_in_f16")


def standin(c, fmt, mutate=None):
    """the launch in fp32, K in 16-wide steps -> {output name: tensor in the output's format, [nz, rows, cols]}"""
    assert mutate is None or mutate in MUTATIONS
    I = inputs(c, fmt)
    K, M, N = I.K, c.M, c.N
    a = prologue(c, I).float()
    b = view(I.B).float()
    if mutate == "pool_beyond_m":                                      # the tile's rows beyond M: products of zero operands
        assert c.pool
        pr = c.pool_rows or 32
        a = torch.cat([a, torch.zeros(a.shape[0], (M + pr - 1) // pr * pr - M, K)], 1)
    slab = 32 if fmt == "f32" else 64
    if mutate == "drop_k_last":
        a = a.clone()
        a[..., K - 1] = 0
    v = torch.zeros(a.shape[0], a.shape[1], N)
    for k0 in range(0, K, 16):
        if mutate == "drop_slab" and (K // slab - 1) * slab <= k0 < (K // slab) * slab:
            assert K >= 2 * slab
            continue
        v = v + a[..., k0:k0 + 16] @ b[..., k0:k0 + 16].transpose(-1, -2)
    if mutate == "double_surplus":
        k0 = (K - 1) // slab * slab
        v = v + a[..., k0:] @ b[..., k0:].transpose(-1, -2)
    Mx = v.shape[1]
    rows = torch.arange(Mx).clamp_max(M - 1)
    out = {}

    def add_bias(t):
        if not c.bias:
            return t
        bv = view(I.bias, z=0)[0]
        return t + (bv.roll(-1) if mutate == "bias_next_col" else bv)

    if mutate != "act_before_bias":
        v = add_bias(v)
    if c.group_rows:
        gi = rows // c.group_rows
        if mutate == "group_neighbour":
            assert c.group_rows == 16
            gi = torch.where(rows % 32 >= 16, gi - 1, gi)
        v = v + view(I.group, z=0)[gi]
    pre = v
    if c.dact:
        v = v * _dact(view(I.dact, z=0).float(), c.act)
    else:
        v = _act(v, c.act)
    if mutate == "act_before_bias":
        assert c.bias and c.act != ACT_NONE and not c.dact
        v = add_bias(v)
    if c.stats:
        s, m2 = _stats((v if mutate == "stats_after_act" else pre)[0][:M])[:2]
        out["col_sum"], out["col_sqsum"] = s[None], m2[None]
    if c.rs_rows:
        ri = (rows + 1 if mutate == "row_scale_next" else rows) // c.rs_rows
        v = v * view(I.row_scale, z=0)[0][ri.clamp_max(I.row_scale.cols - 1)][:, None]
    if c.res:
        if mutate == "res_ldc":
            ld = N + c.ldc_pad
            assert ld != I.res.ld
            v = v + I.res.buf.as_strided((M, N), (ld, 1), I.res.off)
        else:
            v = v + view(I.res, z=0)
    if c.res2:
        v = v + view(I.res2, z=0)

    def rd(t, name):
        dt = I.outs[name].buf.dtype
        if mutate == "bf16_in_f16" and dt == torch.float16:
            t = t.to(torch.bfloat16).float()
        return t.to(dt)

    if c.c != "none":
        cc = v[:, :M].clone()
        if mutate == "stale_last_row":
            assert M > 1
            cc[:, M - 1] = cc[:, M - 2]
        out["C"] = rd(cc, "C")
    if c.out2:
        first = c.out2_pre != (mutate == "out2_wrong_side")
        out["out2"] = rd((pre if first else v)[:, :M], "out2")
    if c.pool:
        pr = c.pool_rows or 32
        out["pool_max"] = rd(_chunks(v[0], pr, float("-inf"))[0].amax(1)[None], "pool_max")
        if c.pool_min:
            out["pool_min"] = rd(_chunks(v[0], pr, float("inf"))[0].amin(1)[None], "pool_min")
    return out


# ------------------------------------------------------------------------------------------------ the criterion
def worst(x, ex, E, Rs=0.0, cap=1.0):
    """-> (max |x - exact| / (cap E + R), index tuple); NaN or an empty tolerance with an error counts as inf.  cap = 1: the
    criterion, |x - exact| <= tol.  cap < 1 (the CPU test of the stand-in) asks the margin of E alone: round-to-nearest errs
    uniformly up to exactly R, so the worst of a few thousand correctly rounded values sits AT the store's half ulp."""
    err = (x.double() - ex).abs()
    tl = cap * E + Rs
    ratio = torch.where(tl > 0, err / tl.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    where, j = [], i
    for n in reversed(ratio.shape):
        where.insert(0, j % n)
        j //= n
    return float(ratio.reshape(-1)[i]), tuple(where)


def check(c, fmt, result, errors=None, cap=1.0, what="GEMM"):
    """result {name: tensor [nz, rows, cols]} against reference(c, fmt) -> {name: worst ratio}; appends to `errors` what is
    above 1 (cap: see worst); prints output=ratio@slice.row.column"""
    ref, res, at = reference(c, fmt), {}, {}
    assert set(result) == set(ref), (sorted(result), sorted(ref))
    for name, x in result.items():
        ex, E, Rs = ref[name]
        ratio, where = worst(x, ex, E, Rs, cap)
        res[name], at[name] = ratio, where
        if errors is not None and not ratio <= 1.0:
            errors.append(f"{case_id(c)} {fmt} [{family(c, fmt)}, {c.tier}] {name}: |x - exact| / ({cap:g} E + R) = {ratio:.3g} > 1 at "
                          f"(slice, row, column) {where}: x {float(x[where]):.6g}, exact {float(ex[where]):.6g}, "
                          f"tol {float((cap * E + Rs)[where]):.3g}")
    print(f"{what} {case_id(c)} {fmt} " + " ".join(f"{k}={v:.3f}@{'.'.join(map(str, at[k]))}" for k, v in res.items()))
    return res


# ------------------------------------------------------------------------------------------------ csrc/ppt_act.h, transcribed
def gelu_poly(x):
    """csrc/ppt_act.h gelu_poly, in x's precision"""
    u = x * x
    p = torch.full_like(x, -3.161567230e-09) * u + 2.434219084e-07
    for k in (-8.201724995e-06, 1.613346976e-04, -2.096408280e-03, 1.932974532e-02, -1.323507577e-01, 7.976950407e-01):
        p = p * u + k
    e = torch.where(x.abs() >= 4.0, torch.sign(x), p * x)
    h = 0.5 * x
    return h * e + h


def erf_fast(x):
    """csrc/ppt_act.h erf_fast, in x's precision"""
    a = x.abs()
    t = 1.0 / (0.3275911 * a + 1.0)
    poly = torch.full_like(x, 1.061405429) * t - 1.453152027
    for k in (1.421413741, -0.284496736, 0.254829592):
        poly = poly * t + k
    return torch.sign(x) * (1.0 - poly * t * torch.exp(-a * a))


# ------------------------------------------------------------------------------------------------ the cases
def _tiered(group, M, N, K, note, tiers=("vec8", "regs", "scalar"), **kw):
    """one case per epilogue tier, chosen by the output as group C does: fp32 contiguous C -> vec8 (for fp32 operands always);
    16-bit contiguous C -> registers, or the 16-byte walk where reg_epilogue_ok refuses the operands (the tier field says which);
    ldc = N + 4 -> scalar"""
    needs_walk = kw.get("res") or kw.get("res2") or kw.get("dact") or kw.get("rs_rows") or kw.get("out2") or \
        kw.get("group_rows", 0) not in (0, 16, 32, 64)
    cs = []
    for t in tiers:
        if t == "vec8":
            cs.append(Case(group, M, N, K, **{**dict(c="f32", tier="vec8", note=note), **kw}))
        elif t == "regs":
            cs.append(Case(group, M, N, K, c="16", fmts=("bf16", "f16"), tier="vec8" if needs_walk else "regs",
                           note=note + ("; 16-bit C, refused by reg_epilogue_ok: the 16-byte walk" if needs_walk else ""), **kw))
        else:
            cs.append(Case(group, M, N, K, c="f32", ldc_pad=4, tier="scalar", note=note, **kw))
            cs.append(Case(group, M, N, K, c="16", ldc_pad=4, fmts=("bf16", "f16"), tier="scalar", note=note, **kw))
    return cs


def _cases():
    cs = []
    # A. slab rings: 2 x 2 tiles of 64 x 64, ragged both ways, plain operands, fp32 contiguous C
    ring = {8: "one tail-only slab", 56: "one tail-only slab, 7 of 8 chunks", 64: "1 whole slab: LDS-DMA ring, min(i, last) prologue",
            72: "1 slab + tail: breaks at s+2", 128: "2 slabs (DMA)", 136: "2 slabs + tail: breaks at s+3", 192: "3 slabs (DMA)",
            200: "3 slabs + tail: second trip of the ring", 256: "4 slabs (DMA)"}
    cs += [Case("A", 70, 72, K, k32=K // 2, tier="vec8", note="slab ring: " + n) for K, n in ring.items()]
    cs += [Case("A", 77, 64, 2048, tier="vec8", note="long K, 32 slabs (64 in fp32)")]
    # B. tile edges
    for K in (64, 72):
        for M, N in ((1, 8), (1, 1), (63, 7), (33, 40), (64, 64), (65, 130), (127, 72), (129, 136)):
            cs.append(Case("B", M, N, K, tier="vec8" if N % 8 == 0 else "scalar", note="tile edge" + ("" if N % 8 == 0 else ", N % 8 != 0")))
    # C. tiers on one product
    for K in (72, 64):
        cs += [Case("C", 130, 136, K, tier="vec8", note="fp32 C contiguous; lda, ldb = K + 8 as in every case of this table"),
               Case("C", 130, 136, K, c="16", fmts=("bf16", "f16"), tier="regs", note="16-bit C contiguous"),
               Case("C", 130, 136, K, c="16", ldc_pad=8, fmts=("bf16", "f16"), tier="regs", note="16-bit C, ldc = N + 8"),
               Case("C", 130, 136, K, ldc_pad=8, tier="vec8", note="fp32 C, ldc = N + 8"),
               Case("C", 130, 136, K, ldc_pad=4, tier="scalar", note="ldc = N + 4"),
               Case("C", 130, 136, K, c="16", ldc_pad=4, fmts=("bf16", "f16"), tier="scalar", note="16-bit C, ldc = N + 4"),
               Case("C", 130, 136, K, c_off=18, tier="scalar", note="fp32 C 8 bytes past a 16-byte boundary"),
               Case("C", 130, 136, K, c="16", c_off=20, fmts=("bf16", "f16"), tier="scalar", note="16-bit C 8 bytes past a 16-byte boundary"),
               Case("C", 130, 132, K, tier="scalar", note="N = 132"),
               Case("C", 130, 136, K, bias=True, bias_off=1, tier="scalar", note="bias view at element 1, fp32 C"),
               Case("C", 130, 136, K, c="16", bias=True, bias_off=1, fmts=("bf16", "f16"), tier="regs",
                    note="bias view at element 1, 16-bit C: registers read it one float at a time")]
    # D. epilogue operands on all three tiers
    D = lambda note, **kw: _tiered("D", 130, 136, 72, note, **kw)
    cs += D("bias", bias=True)
    for act in (ACT_RELU, ACT_GELU, ACT_QUICKGELU):
        cs += D("bias + activation", bias=True, act=act)
    cs += D("activation alone", act=ACT_GELU)
    for g in (16, 32, 24, 64):
        cs += D("group term, partial last group", group_rows=g)
    for r in (1, 7, 64, 513):
        cs += D("row scale", rs_rows=r)
    cs += D("residual", res=True) + D("residual + residual2 (prefetched on 64 x 64 tiles)", res=True, res2=True, bias=True)
    for act in (ACT_NONE, ACT_RELU, ACT_GELU, ACT_QUICKGELU):
        cs += D("saved pre-activation, ld_dact = N + 8", dact=True, act=act)
    cs += D("group + residual: the group term is prefetched", group_rows=32, res=True)
    cs += D("group + dact", group_rows=16, dact=True, act=ACT_GELU)
    cs += D("residual + dact: the residual is prefetched", res=True, dact=True, act=ACT_QUICKGELU)
    for o2 in ("f32", "16"):
        for pre in (False, True):
            cs += D("second output, ldc2 = N + 8", out2=o2, out2_pre=pre, bias=True, act=ACT_GELU, rs_rows=64)
    cs += _tiered("D", 130, 136, 72, "pool only, no C", tiers=("vec8",), c="none", pool="f32", pool_rows=32, bias=True, res=True) \
        + [Case("D", 130, 136, 72, c="none", pool="16", pool_rows=32, bias=True, fmts=("bf16", "f16"), tier="regs", note="pool only, no C")]
    # E. statistics and pools: the 128 x 128 register-staged kernel
    for M, N, K in ((200, 136, 72), (70, 136, 64), (1040, 128, 64)):
        for c16 in (False, True):
            kw = dict(c="16", fmts=("bf16", "f16"), tier="regs") if c16 else dict(c="f32", tier="vec8")
            E = lambda note, **k2: Case("E", M, N, K, note=note, **{**kw, **k2})
            cs += [E("statistics, M % 32 != 0", stats=True, bias=True),
                   E("statistics + activation", stats=True, group_rows=32, act=ACT_RELU)]
            for pr, pm in ((16, True), (32, False), (64, True)):
                for pd in ("f32", "16"):
                    cs.append(E("pool, ragged last group", pool=pd, pool_rows=pr, pool_min=pm, bias=True, act=ACT_GELU))
            cs.append(E("statistics + pool", stats=True, pool="16", pool_rows=32, pool_min=True, group_rows=16))
        cs.append(Case("E", M, N, K, stats=True, res=True, res2=True, tier="vec8", note="residual + residual2 + statistics: PRE2 false"))
        for am in (A_AFFINE_RELU, A_CONV1):
            cs.append(Case("E", M, N, K, stats=True, a_mode=am, bias=True, tier="vec8", note="A prologue + statistics, fp32 C"))
            cs.append(Case("E", M, N, K, stats=True, pool="16", pool_rows=32, a_mode=am, c="16", fmts=("bf16", "f16"), tier="regs",
                           note="A prologue + statistics + pool, 16-bit C"))
    # ... and the launches the scalar tier would have taken without filling them: refused (csrc/gemm.hip ppt_gemm)
    for M, N, K in ((200, 136, 72), (70, 136, 64)):
        H = lambda note, **kw: Case("Ehole", M, N, K, tier="scalar", expect="raise", note=note + ": refused", **kw)
        for what in (dict(stats=True), dict(pool="f32", pool_rows=32, pool_min=True), dict(stats=True, pool="16", pool_rows=16)):
            cs += [H("ldc = N + 4", ldc_pad=4, bias=True, **what),
                   H("16-bit C, ldc = N + 4", c="16", ldc_pad=4, fmts=("bf16", "f16"), **what),
                   H("misaligned C", c_off=18, **what),
                   H("misaligned bias, fp32 C", bias=True, bias_off=1, **what),
                   H("misaligned group_add, fp32 C", group_rows=32, group_off=1, **what),
                   H("misaligned group_add, 16-bit C, 24-row groups", c="16", group_rows=24, group_off=1, fmts=("bf16", "f16"), **what)]
    # F. prologues on 64 x 64 tiles, and on 128 x 128 (statistics)
    for am in (A_AFFINE_RELU, A_CONV1):
        for K, k32 in ((8, 4), (64, 32), (72, 36), (1024, 1024)):
            for M in (33, 130):
                cs.append(Case("F", M, 72, K, k32=k32, a_mode=am, bias=True, tier="vec8", note="A prologue, 64 x 64 tiles"))
                cs.append(Case("F", M, 72, K, k32=k32, a_mode=am, stats=True, c="16", fmts=("bf16", "f16"), tier="regs",
                               note="A prologue, 128 x 128 tiles"))
                cs.append(Case("F", M, 72, K, k32=k32, a_mode=am, stats=True, fmts=("f32",), tier="vec8", note="A prologue, 128 x 128 tiles"))
    # G. batched
    for sb in (False, True):
        cs += [Case("G", 70, 72, 72, batch=3, strideB=sb, tier="vec8", note="strideC = M N"),
               Case("G", 70, 72, 64, batch=3, strideB=sb, zc_extra=8, bias=True, act=ACT_RELU, tier="vec8", note="strideC = M N + 8: a gap"),
               Case("G", 70, 72, 72, batch=3, strideB=sb, zc_extra=4, bias=True, act=ACT_GELU, tier="vec8+scalar",
                    note="strideC = M N + 4: slices 0 and 2 vec8, slice 1 (zc % 8 == 4) scalar"),
               Case("G", 70, 72, 64, batch=3, strideB=sb, c="16", fmts=("bf16", "f16"), bias=True, tier="regs", note="16-bit C, strideC = M N"),
               Case("G", 70, 72, 72, batch=3, strideB=sb, c="16", zc_extra=4, fmts=("bf16", "f16"), bias=True, act=ACT_GELU,
                    tier="regs+scalar", note="16-bit C, strideC = M N + 4: zc % 8 moves slice 1 from registers to scalar")]
    # H. the half-slab kernel: >= 768 tiles of 128 x 128, register epilogue
    h = dict(c="16", fmts=("bf16", "f16"), tier="regs")
    for K in (32, 64, 96):
        cs.append(Case("H", 12288 - 37, 1024, K, note="half-slab kernel, plain", **h))
    cs += [Case("H", 12288 - 37, 1024, 64, bias=True, act=ACT_GELU, note="half-slab kernel, EPI_GELU", **h),
           Case("H", 12288 - 37, 1024, 32, group_rows=32, stats=True, note="half-slab kernel, EPI_GROUP | EPI_STATS", **h),
           Case("H", 12288 - 37, 1024, 96, bias=True, act=ACT_RELU, pool="16", pool_rows=32, note="half-slab kernel, general mask", **h),
           Case("H", 59 * 128 - 37, 13 * 128, 64, note="767 tiles: just under the gate, 64 x 64 LDS-DMA kernel", **h),
           Case("H", 12288 - 37, 1024, 40, stats=True, note="K = 40 is no half-slab multiple: register-staged 128 x 128", **h)]
    # I. ppt_gemm256 called explicitly
    i16 = dict(core="256", fmts=("bf16", "f16"))
    for M, N, K in ((1, 128, 64), (255, 136, 96), (257, 256, 128), (300, 264, 160), (300, 1152, 64), (255, 256, 96)):
        cs += [Case("I", M, N, K, c="16", tier="regs", note="256 core, plain", **i16),
               Case("I", M, N, K, c="16", bias=True, act=ACT_GELU, tier="regs", note="256 core, GELU", **i16)]
    cs += [Case("I", 300, 256, 96, c="16", group_rows=32, stats=True, tier="regs", note="256-wide tile: group + statistics", **i16),
           Case("I", 300, 1152, 64, c="16", group_rows=16, stats=True, tier="regs", note="256-wide tile, ragged N: group + statistics", **i16),
           Case("I", 257, 136, 64, c="16", res=True, bias=True, tier="vec8", note="256 core, LDS walk: residual", **i16),
           Case("I", 257, 256, 160, c="16", rs_rows=64, act=ACT_QUICKGELU, tier="vec8", note="256 core, LDS walk: row scale", **i16),
           Case("I", 300, 264, 96, c="16", dact=True, act=ACT_GELU, tier="vec8", note="256 core, LDS walk: dact", **i16),
           Case("I", 255, 128, 128, c="16", out2="f32", out2_pre=True, bias=True, act=ACT_GELU, tier="vec8", note="256 core, LDS walk: out2", **i16),
           Case("I", 300, 256, 64, c="f32", bias=True, tier="vec8", note="256 core, LDS walk: fp32 C", **i16),
           Case("I", 257, 128, 96, c="16", batch=3, strideB=True, tier="regs", note="256 core, batched", **i16),
           Case("I", 130, 256, 64, c="f32", batch=3, zc_extra=8, res=False, bias=True, tier="vec8", note="256 core, batched, fp32 C with a gap", **i16)]
    return cs


CASES = _cases()
assert len({case_id(c) for c in CASES}) == len(CASES)
RUNS = [(c, f) for c in CASES for f in c.fmts]


def run_id(r):
    return f"{case_id(r[0])}-{r[1]}"
