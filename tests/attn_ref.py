"""Shared by tests/test_attention_ref_cpu.py and tests/test_attention_gpu.py: references of softmax(q k^T * scale [+ causal]) v
and its backward in plain torch on the CPU (no ppt_amd import), the case table of the 16-bit attention kernels, and the
criterion that compares a kernel's result with them.

  exact          fp64, gradients by autograd: the truth.
  rounded        fp32 with a round-to-nearest-even cast to the 16-bit format where the MFMA kernels of csrc/attention_mfma.hip
                 round: the yardstick.  Its distance from `exact` is what 16-bit operands cost; a kernel that makes the same
                 roundings lands at the same distance.
  rounded_tiled  `rounded` with the kernels' summation structure (online softmax over 64-key tiles, dK / dV over 32-query tiles):
                 a stand-in for a correct kernel, for the CPU test of the criterion.
  row_ratio      per (physical row, head) of 64 values: ||x - exact|| / (||rounded - exact|| + floor); a test passes at <= CAP.

Layouts (csrc/attn_rowmap.h): plain, qkv [n_seq * T, 3 * H * 64], lse [n_seq, H, T]; prefix-shared (P > 0, causal), C prompts whose
first P positions are stored once, qkv [P + C (T - P), 3 * H * 64], lse [rows, H].
"""
import collections
import functools
import zlib

import torch

HD = 64
CAP = 2.0                                                   # the criterion's cap: a condition, not a measurement
Ref = collections.namedtuple("Ref", "out lse dqkv mag_out mag_dqkv sens_dqkv lse_tol")
Model = collections.namedtuple("Model", "out lse dqkv")


# ------------------------------------------------------------------------------------------------ layout
def rowmap(n_seq, T, P):
    """[n_seq, T] int64: physical row of position pos of sequence c"""
    pos = torch.arange(T).expand(n_seq, T)
    c = torch.arange(n_seq)[:, None]
    return c * T + pos if P == 0 else torch.where(pos < P, pos, P + c * (T - P) + pos - P)


def owned(n_seq, T, P):
    """[n_seq, T] bool: the copy of a row that produces its output and carries its dout (shared rows: copy 0 only)"""
    own = torch.ones(n_seq, T, dtype=torch.bool)
    if P:
        own[1:, :P] = False
    return own


def n_rows(n_seq, T, P):
    return P + n_seq * (T - P) if P else n_seq * T


def _expand(x, rm):
    """x [rows, k * 64] -> [n_seq, k, T, 64]"""
    return x.view(x.shape[0], -1, HD)[rm].permute(0, 2, 1, 3)


def _keymask(T, causal, width=0):
    """[T, T] bool, True = masked"""
    if not causal:
        return torch.zeros(T, T, dtype=torch.bool)
    return torch.ones(T, T, dtype=torch.bool).triu(1 + width)


def _to_rows(full, rm, own, rows):
    """full [n_seq, k, T, d] -> physical [rows, k * d], every row from the copy that owns it"""
    t = full.permute(0, 2, 1, 3)
    out = torch.zeros((rows,) + tuple(t.shape[2:]), dtype=full.dtype)
    out[rm[own]] = t[own]
    return out.reshape(rows, -1)


def _fold(dq, dk, dv, rm, rows, copies=None):
    """gradients of the expanded sequences [n_seq, H, T, 64] -> dqkv [rows, 3 * H * 64]: rows that several sequences share are
    summed over `copies` (all of them by default; dq of the shared rows is non-zero in copy 0 only)"""
    g = torch.stack([dq, dk, dv], 1).permute(0, 3, 1, 2, 4)                 # [n, T, 3, H, 64]
    if copies is not None:
        g, rm = g[copies], rm[copies]
    acc = torch.zeros((rows,) + tuple(g.shape[2:]), dtype=g.dtype)
    acc.index_add_(0, rm.reshape(-1), g.reshape((-1,) + tuple(g.shape[2:])))
    return acc.reshape(rows, -1)


# ------------------------------------------------------------------------------------------------ fp64
def exact(qkv, dout, n_seq, T, P, H, scale, causal):
    """fp64 on the 16-bit inputs upcast -> Ref(out [rows, H*64], lse (layout as the kernels'), dqkv [rows, 3*H*64] by autograd,
    mag_out, mag_dqkv: the same sums over absolute values (what fp32 accumulation noise is relative to), sens_dqkv: what a unit
    relative error of delta's input does to dQ and dK (both for row_ratio's floor), lse_tol: the bound of lse_check).  The prefix-shared layout is expanded to C full sequences; dout of the duplicate prefix
    rows of copies 1 .. C-1 is zero; autograd through the expansion folds back -- dQ of the shared rows from copy 0, their
    dK / dV summed over the copies."""
    rows = qkv.shape[0]
    assert rows == n_rows(n_seq, T, P) and (not P or causal)
    rm, own = rowmap(n_seq, T, P), owned(n_seq, T, P)
    x = qkv.double().view(rows, 3 * H, HD).requires_grad_()
    full = x[rm].permute(0, 2, 1, 3)                                        # [n, 3H, T, 64]
    q, k, v = full[:, :H], full[:, H:2 * H], full[:, 2 * H:]
    mask = _keymask(T, causal)
    s = (q @ k.transpose(-1, -2) * scale).masked_fill(mask, float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = p @ v
    g = _expand(dout.double(), rm) * own[:, None, :, None]
    (o * g).sum().backward()
    with torch.no_grad():
        qa, ka, va, ga = q.abs(), k.abs(), v.abs(), g.abs()
        ds_abs = p * (ga @ va.transpose(-1, -2) + (o.abs() * ga).sum(-1, keepdim=True)) * scale
        mag = _fold(ds_abs @ ka, ds_abs.transpose(-1, -2) @ qa, p.transpose(-1, -2) @ ga, rm, rows)
        # delta = rowsum(out * dout) reads the ROUNDED out: one scalar error per query row, w = ||out * dout||_2 times a relative
        # rounding, that reaches dQ as w scale (P K) and dK as the independent sum of w scale P^T Q (row_ratio's `sens`)
        w2 = ((o * g) ** 2).sum(-1, keepdim=True) * scale ** 2
        sens = _fold(w2 * (p @ k) ** 2, (p ** 2 * w2).transpose(-1, -2) @ q ** 2, torch.zeros_like(q), rm, rows).sqrt()
        qk_abs = (qa @ ka.transpose(-1, -2)).masked_fill(mask, 0.0).amax(-1)
        tol = 2.0 ** -23 * 64 * scale * qk_abs + 1e-5
        stat = (lambda t: _to_rows(t[..., None], rm, own, rows)) if P else (lambda t: t.clone())
        return Ref(_to_rows(o, rm, own, rows), stat(lse), x.grad.reshape(rows, -1), _to_rows(p @ va, rm, own, rows), mag, sens, stat(tol))


# ------------------------------------------------------------------------------------------------ the rounding model
MUTATIONS = ("mask_wide", "drop_last_key", "cross_prompt", "delta_unrounded", "bf16_inside", "fold_missing_copy")


def _model(qkv, dout, n_seq, T, P, H, scale, causal, dtype, tiled=False, mutate=None):
    rows = qkv.shape[0]
    assert rows == n_rows(n_seq, T, P) and (not P or causal) and qkv.dtype == dtype and mutate in (None,) + MUTATIONS
    inner = torch.bfloat16 if mutate == "bf16_inside" else dtype

    def rd(t, fmt=inner):
        return t.to(fmt).float()

    rm, own = rowmap(n_seq, T, P), owned(n_seq, T, P)
    x = qkv.float()
    q = _expand(x, rm)[:, :H]
    rm_kv = rm
    if mutate == "cross_prompt":                              # prompt c continues its prefix with prompt c + 1's own rows
        assert P and n_seq > 1
        rm_kv = torch.cat([rm[:, :P], rm.roll(-1, 0)[:, P:]], 1)
    kv = _expand(x, rm_kv)
    k, v = kv[:, H:2 * H], kv[:, 2 * H:]
    mask = _keymask(T, causal, 1 if mutate == "mask_wide" else 0)
    if mutate == "drop_last_key":
        assert T > 1
        mask = mask.clone()
        mask[:, T - 1] = True
    s = (q @ k.transpose(-1, -2) * scale).masked_fill(mask, float("-inf"))
    g = _expand(dout.float(), rm) * own[:, None, :, None]

    # ---- forward: P = exp(s - max) rounded before P.V, the sum of the unrounded P in fp32, out rounded on store
    if not tiled:
        m = s.amax(-1, keepdim=True)
        p = torch.exp(s - m)
        l = p.sum(-1, keepdim=True)
        o = rd(p) @ v / l
    else:
        m = torch.full(s.shape[:-1] + (1,), float("-inf"))
        l = torch.zeros_like(m)
        acc = torch.zeros_like(q)
        for k0 in range(0, T, 64):
            st = s[..., k0:k0 + 64]
            mn = torch.maximum(m, st.amax(-1, keepdim=True))
            alpha = torch.exp(m - mn)
            p = torch.exp(st - mn)
            l = l * alpha + p.sum(-1, keepdim=True)
            acc = acc * alpha + rd(p) @ v[..., k0:k0 + 64, :]
            m = mn
        o = acc / l
    lse = (m + torch.log(l))[..., 0]
    out = rd(o, dtype)

    # ---- backward from the stored out and lse: P rounded before P^T.dO, dS before dS.K and dS^T.Q, dqkv rounded on store
    pn = torch.exp(s - lse[..., None])
    delta = ((o if mutate == "delta_unrounded" else out) * g).sum(-1, keepdim=True)
    ds = pn * (g @ v.transpose(-1, -2) - delta) * scale
    if not tiled:
        dq = rd(ds) @ k
        dk = rd(ds).transpose(-1, -2) @ q
        dv = rd(pn).transpose(-1, -2) @ g
    else:
        dq, dk, dv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
        for k0 in range(0, T, 64):
            dq += rd(ds[..., k0:k0 + 64]) @ k[..., k0:k0 + 64, :]
        for q0 in range(0, T, 32):
            dk += rd(ds[..., q0:q0 + 32, :]).transpose(-1, -2) @ q[..., q0:q0 + 32, :]
            dv += rd(pn[..., q0:q0 + 32, :]).transpose(-1, -2) @ g[..., q0:q0 + 32, :]
    if mutate == "cross_prompt":                              # (its gradients go back where it read from)
        dkv = _fold(torch.zeros_like(dq), dk, dv, rm_kv, rows)
        dqkv = _fold(dq, torch.zeros_like(dq), torch.zeros_like(dq), rm, rows) + dkv
    elif mutate == "fold_missing_copy":
        assert P and n_seq > 1
        dqkv = _fold(dq, dk, dv, rm, rows, copies=slice(0, n_seq - 1))
        last = rm[n_seq - 1, P:]
        dqkv[last] = _fold(dq, dk, dv, rm, rows)[last]
    else:
        dqkv = _fold(dq, dk, dv, rm, rows)
    stat = (lambda t: _to_rows(t[..., None], rm, own, rows)) if P else (lambda t: t)
    return Model(_to_rows(out, rm, own, rows), stat(lse), rd(dqkv, dtype))


def rounded(qkv, dout, n_seq, T, P, H, scale, causal, dtype, mutate=None):
    """The rounding model: the mathematics of `exact` in fp32, dense, with a round-to-nearest-even cast to `dtype` where the
    16-bit kernels round (attn_fwd_stream, attn_fwd_resident, attn_bwd_dkv_body, attn_bwd_dq_body, attn_bwd_tiny_mfma,
    attn_delta) -> Model(out, lse, dqkv) as fp32 tensors holding 16-bit values (lse: fp32).

      forward   scores, max and sum in fp32 on the 16-bit inputs; P = exp(s - max) cast before P.V (pack8 / pack2), the sum runs
                over the UNROUNDED P; out = O / sum cast on store.
      backward  P = exp(s - lse) with the forward's fp32 lse, cast before P^T.dO; delta = rowsum(out * dout) in fp32 from the
                STORED (rounded) out; dS = P (dP - delta) scale from the unrounded P, cast before dS.K and dS^T.Q; dQ, dK, dV
                accumulate in fp32 (the shared rows' dK / dV over all copies, in fp32 partial slots) and are cast once on store.

    Where the kernels differ from this list (all of them round LESS than the model, so they sit closer to `exact`):
      * the peeled last key of T = 64 n + 1 (non-causal): its weight enters as the initial state, in fp32, never cast;
      * attn_fwd_resident's last query row runs on the vector ALU: its P is never cast;
      * the kernels cast P relative to the RUNNING maximum and rescale O in fp32 afterwards: the same relative rounding, at
        values that are larger by the later rescale factor (fewer fp16 subnormals than the model);
      * the fallbacks for unaligned pointers (attn_fwd_quad, attn_bwd_dq / attn_bwd_dkv of csrc/attention.hip) keep P and dS in
        fp32: only delta's input and the stores are 16-bit.
    `mutate` (MUTATIONS) breaks the model on purpose, for the CPU test of the criterion."""
    return _model(qkv, dout, n_seq, T, P, H, scale, causal, dtype, False, mutate)


def rounded_tiled(qkv, dout, n_seq, T, P, H, scale, causal, dtype):
    """`rounded` with an online softmax over 64-key tiles (P cast relative to the running maximum), dQ summed over 64-key tiles
    and dK / dV over 32-query tiles: the same roundings, another summation order."""
    return _model(qkv, dout, n_seq, T, P, H, scale, causal, dtype, True, None)


# ------------------------------------------------------------------------------------------------ the criterion
def row_ratio(x, model, ref, mag=None, sens=None, u=0.0):
    """x, model, ref [rows, H * 64] -> (max over (row, head) of ||x - ref|| / (||model - ref|| + floor), (row, head)) with
    floor = median(||model - ref||) + 2^-23 ||mag|| + 2 u ||sens||.

    The last two terms repair the floor where one row's error is not a 64-component draw that concentrates around its scale:
      * mag: `ref` by default; exact()'s sums of absolute values for the parts where `ref` can cancel to zero while fp32
        accumulation noise does not (T = 1: dS = P (dP - delta) is 0 exactly in fp64 and the difference of two 64-term fp32 sums in a
        kernel).  |mag| >= |ref| elementwise, and the term stays orders of magnitude below a 16-bit rounding of the same sums.
      * sens (exact()'s sens_dqkv), u = 2^-p the format's largest relative rounding error: delta = rowsum(out * dout) reads the
        stored out, every element of which carries two roundings of at most u (P before P.V, out on store) -- at most 2 u per
        element, in quadrature over the 64 elements 2 u ||out * dout||_2.  That ONE scalar per query row scales a whole dQ row
        (scale delta_err P.K) and enters dK through P^T: with a peaked softmax it is the larger part of the row's error, and a
        correct result whose forward rounds P at other values (relative to a running maximum) draws it independently of the
        model's: ||x - ref|| reaches three times ||model - ref|| in a few rows per thousand (rounded_tiled against rounded,
        gain 2 and 3) although both make the same roundings.  Zero for out and dV."""
    H = x.shape[1] // HD
    r = ref.double().reshape(-1, HD)
    e_x = (x.double().reshape(-1, HD) - r).norm(dim=1)
    e_m = (model.double().reshape(-1, HD) - r).norm(dim=1)
    den = e_m + e_m.median() + 2.0 ** -23 * (r if mag is None else mag.double().reshape(-1, HD)).norm(dim=1)
    if sens is not None:
        den = den + 2.0 * u * sens.double().reshape(-1, HD).norm(dim=1)
    ratio = torch.where(den > 0, e_x / den.clamp_min(1e-300), torch.where(e_x > 0, float("inf"), 0.0).double())
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    return float(ratio[i]), (i // H, i % H)


UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def parts(H, out, dqkv):
    n = H * HD
    return (("out", out), ("dq", dqkv[:, :n]), ("dk", dqkv[:, n:2 * n]), ("dv", dqkv[:, 2 * n:]))


def ratios(H, out, dqkv, model, ref, dtype):
    """-> {part: (max ratio, (row, head))} of a result (out, dqkv) against the rounding model and the fp64 reference"""
    res = {}
    for (name, x), (_, m), (_, r), (_, g), (_, sn) in zip(parts(H, out, dqkv), parts(H, model.out, model.dqkv), parts(H, ref.out, ref.dqkv),
                                                          parts(H, ref.mag_out, ref.mag_dqkv), parts(H, None, ref.sens_dqkv)):
        res[name] = row_ratio(x, m, r, g, sn, UNIT[dtype])
    return res


def lse_check(lse, ref):
    """-> (max of |lse - exact| / bound, flat index, that error, its bound); passes at <= 1.  bound = 2^-23 * 64 * scale *
    max_j sum_d |q_d k_jd| (fp32 accumulation of 64 exact products) + 1e-5 (the exp2 / log2 approximations)"""
    err = (lse.double() - ref.lse).abs().reshape(-1)
    rel = err / ref.lse_tol.reshape(-1)
    rel = torch.where(torch.isnan(rel), torch.full_like(rel, float("inf")), rel)
    i = int(rel.argmax())
    return float(rel[i]), i, float(err[i]), float(ref.lse_tol.reshape(-1)[i])


# ------------------------------------------------------------------------------------------------ the cases
SCALE = 0.125
Case = collections.namedtuple("Case", "group n T P H causal gain gscale note")


def _plain(n, T, H, causal, note, gain=1.0, gscale=1.0):
    both = causal == "both"
    return [Case("plain", n, T, 0, H, c, gain, gscale, note) for c in ((False, True) if both else (causal,))]


CASES = (
    _plain(3, 1, 2, "both", "one key; tiny backward; out = v")
    + _plain(2, 5, 1, False, "below one tile")
    + _plain(2, 63, 3, "both", "masked tile tail")
    + _plain(1, 64, 8, "both", "full tile; 8 pairs: XCD map on; last tiny-backward T")
    + _plain(7, 65, 2, "both", "peeled last key (non-causal); first short-backward T")
    + _plain(3, 77, 8, True, "text tower; 24 pairs: XCD map on, two role workgroups")
    + _plain(40, 77, 8, True, "320 pairs: both roles in one workgroup", gscale=1e-4)
    + _plain(2, 127, 3, "both", "")
    + _plain(2, 128, 4, "both", "last short-backward T; 8 pairs")
    + _plain(3, 129, 3, "both", "second query block of one row; peel; first dkv + dq backward; 9 pairs: XCD map off")
    + _plain(3, 200, 2, False, "ragged")
    + _plain(2, 300, 4, True, "5 key tiles, 3 query blocks; 8 pairs", gain=3.0)
    + _plain(2, 513, 6, False, "streaming ViT shape, peel; 12 pairs")
    + _plain(1, 513, 8, False, "same with the XCD map on", gain=2.0)
    + [Case("resident", 22, 449, 0, 6, False, 1.0, 1.0, "the n == 7 instantiation; the last row on the vector ALU"),
       Case("resident", 22, 385, 0, 6, False, 1.0, 1.0, "n == 6")]
    + [Case("prefix", C, T, P, H, True, 1.0, 1.0, note) for C, T, P, H, note in (
        (5, 37, 17, 8, ""), (40, 37, 17, 8, "tiny kernel, 328 pairs"),
        (40, 77, 17, 8, "the prompt chain's shape; short kernel, one workgroup for both roles"), (6, 20, 1, 2, ""),
        (3, 77, 76, 2, "one own row"), (2, 130, 70, 1, "long kernels"), (3, 150, 130, 2, "prefix longer than a query block"))]
    + [Case("fallback", 3, 77, 0, 8, True, 1.0, 1.0, "qkv 8 bytes into its buffer: attn_fwd_quad, attn_bwd_dq / attn_bwd_dkv"),
       Case("fallback", 2, 129, 0, 3, False, 1.0, 1.0, "the same, non-causal, two query blocks")]
)
DTYPES = (torch.float16, torch.bfloat16)


def case_id(c):
    s = f"{c.group}-n{c.n}-T{c.T}" + (f"-P{c.P}" if c.P else "") + f"-H{c.H}-" + ("causal" if c.causal else "full")
    return s + (f"-gain{c.gain:g}" if c.gain != 1.0 else "") + (f"-g{c.gscale:g}" if c.gscale != 1.0 else "")


def family(c):
    """the kernels a case is expected to run (for the failure messages)"""
    if c.group == "fallback":
        return "attn_fwd_quad + attn_delta / attn_bwd_dq / attn_bwd_dkv (unaligned qkv)"
    fwd = "attn_fwd_resident" if c.group == "resident" else "attn_fwd_stream"
    bwd = "attn_bwd_tiny_mfma" if c.T <= 64 else "attn_bwd_short_mfma" if c.T <= 128 else "attn_delta + attn_bwd_dkv_mfma + attn_bwd_dq_mfma"
    return f"{fwd} + {bwd}" + (" + attn_prefix_reduce (prefix-shared layout)" if c.P else "")


def dtype_name(dtype):
    return {torch.float16: "f16", torch.bfloat16: "bf16"}[dtype]


@functools.lru_cache(maxsize=None)
def inputs(c, dtype):
    """-> (qkv [rows, 3*H*64], dout [rows, H*64]) in `dtype` on the CPU: randn, q times gain, dout times gscale; seeded per case"""
    gen = torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()))
    rows = n_rows(c.n, c.T, c.P)
    qkv = torch.randn(rows, 3 * c.H * HD, generator=gen)
    qkv[:, :c.H * HD] *= c.gain
    dout = torch.randn(rows, c.H * HD, generator=gen) * c.gscale
    return qkv.to(dtype), dout.to(dtype)


@functools.lru_cache(maxsize=4)
def references(c, dtype):
    """-> (Ref, Model) of a case, built once (the fp64 autograd of the largest case is the cost of a test)"""
    qkv, dout = inputs(c, dtype)
    a = (qkv, dout, c.n, c.T, c.P, c.H, SCALE, c.causal)
    return exact(*a), rounded(*a, dtype)
