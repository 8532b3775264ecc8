"""Shared by tests/test_decoder_ref_cpu.py and tests/test_partseg_decoder_gpu.py: references of the three fused autograd nodes of
the part-segmentation decoder (ppt_amd/autograd.py: _FeaturePropagation, _DGCNNLayer, _ConvBNReLURows) in plain torch on the CPU
(no ppt_amd import), their case table with conditioned inputs, and the criterion that compares a node's result with them.

  exact          fp64 on the node's fp32 inputs, the reference formulation (3-NN interpolation + concatenation + conv + biased-
                 variance BatchNorm + ReLU; graph feature + conv + F.group_norm + leaky_relu(0.2) + max over k), gradients by
                 autograd: the truth.
  rounded(T)     fp32, the same mathematics with the backward written out and a round-to-nearest-even cast to T (float16 |
                 bfloat16) where the node rounds: the yardstick.  Its distance from `exact` is what 16-bit operands cost.
  rounded_tiled  `rounded` with another summation structure (products over K chunks of 64, row reductions over chunks of 64 rows,
                 statistics as chunk partials merged in fp64): stands in for a correct kernel in the CPU test of the criterion.
  ratio          per output tensor and per output channel (last dimension): ||x - exact|| / (||rounded - exact|| + floor),
                 floor = median over the channels of ||rounded - exact|| + 2^-23 ||mag||; a test passes at <= CAP.

Where the node rounds (read from ppt_amd/autograd.py and the kernels it calls; no deviation from the list in the issue that asked
for this file):
  conv + BN + ReLU   both GEMM operands in T; product + bias fp32; statistics, scale / shift and the activation from that fp32
                     tensor; the output cast to T only where it feeds the next GEMM.  Backward: ReLU mask from the fp32
                     fma(y, scale, shift) > 0; dgamma = sum g xhat and dbeta = sum g from the unrounded masked gradient g; the
                     BatchNorm input gradient dY cast to T; dW = T(dY)^T x, db = column sums of T(dY), dX = T(dY) T(W) in fp32.
                     eval(): running statistics, and dY = scale g without the two batch terms.
  feature propagation  weights 1 / (d + 1e-8) normalised and the interpolated rows in fp32, cast once as the first operand (the
                     zero K padding changes no value and is not modelled); dp2 = weighted scatter of the fp32 dX columns.
  DGCNN layer        Wa and Wb - Wa formed in fp32, then cast; P, Q, y = P[idx] + Q, GroupNorm, LeakyReLU, max in fp32; the
                     gradient goes to the FIRST maximising neighbour; dy fp32; dP (scatter) and dQ (sum over k) fp32, cast to T
                     for the two weight-gradient and the two input-gradient GEMMs; dW = [dWa - dWd | dWd].
  gradient scale     incoming gradient times S, every outgoing gradient times 1 / S (S a power of two: exact in fp32, but the
                     casts to T see S-times larger values -- float16's subnormals are modelled).

The floor: the median term is what attn_ref.row_ratio uses -- a channel whose own model error happens to be small is measured
against the typical one.  `mag` is `exact` except for the bias-like sums dbeta (BatchNorm and GroupNorm), which no 16-bit rounding
reaches in the last layer: there ||rounded - exact|| is fp32 summation noise only, and the sum of the ABSOLUTE values of the
terms (what that noise is relative to; exact()'s second result) takes exact's place, as attn_ref's mag_dqkv does.
Channels are compared in groups of 8 (GROUP): per single channel rounded_tiled reaches 1.1 - 1.5, above CAP / 2, in float16 on
the gradient of a conv bias in front of a train() BatchNorm -- zero in exact arithmetic, so the whole value is rounding: the sum
of the roundings of T(dY), of which a correct result in another summation order flips a few (a flip in one layer moves the next
layer's gradient row by 2^-11, which flips more).  One channel's sum is one draw; eight concentrate.  The cap is not raised.

Conditioning.  A ReLU mask and an arg-max are discrete: fp32 and fp64 may legitimately disagree next to a tie.  inputs() moves the
data away from ties: every BatchNorm pre-activation |scale y + shift| >= 1e-3 in train() and eval(), every DGCNN winner leads the
runner-up by >= 1e-3 (fp64; >= 1e-4 in the two rounding models, which a kernel follows to fp32 noise) -- except between the two
identical source rows of the tie case.  The knob is ONE element of the conv weight row of an offending channel (it moves that
channel only); the share of nudged elements among all of a case's input values is asserted <= 1 %.
"""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = (F16, BF16)
CAP = 2.0                                                   # the criterion's cap: a condition, not a measurement
GROUP = 8                                                   # channels per ratio (module docstring)
BN_EPS, BN_MOM, GN_GROUPS, GN_EPS, SLOPE = 1e-5, 0.1, 4, 1e-5, 0.2
MARGIN, MARGIN_ROUNDED, MAX_NUDGED = 1e-3, 1e-4, 0.01

ZERO_IN_TRAIN = ("b0", "b1", "b2")                           # a conv bias in front of a train() BatchNorm: its gradient is zero in exact arithmetic
MUTATIONS = ("bn_train_terms_dropped", "bn_eval_terms_kept", "ragged_chunk", "last_quad", "dgamma_from_rounded", "db_unmasked",
             "interp_unnormalised", "wd_is_wb", "tie_to_all", "gn_n_without_cg", "unscale_missing")


def dtype_name(dtype):
    return {F16: "f16", BF16: "bf16", torch.float32: "f32"}[dtype]


class Opt:
    """how a model computes: T the 16-bit format (None: no cast), S the gradient scale, tiled the summation structure, mut one of
    MUTATIONS, ft the arithmetic (float64 with T = None: the written-out backward in fp64, for the conditioning and self-checks)"""

    def __init__(self, T=None, S=1.0, tiled=False, mut=None, ft=torch.float32):
        assert mut in (None,) + MUTATIONS
        self.T, self.S, self.tiled, self.mut, self.ft = T, float(S), tiled, mut, ft


def _rd(t, o):
    return t if o.T is None else t.to(o.T).to(t.dtype)


def _mm(a, b, o):
    """a [M,K] @ b [K,N]; tiled: fp32 accumulation over K chunks of 64"""
    if not o.tiled:
        return a @ b
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=a.dtype)
    for k0 in range(0, a.shape[1], 64):
        acc = acc + a[:, k0:k0 + 64] @ b[k0:k0 + 64]
    return acc


def _rowsum(x, o):
    """sum over the rows (dim 0); tiled: chunks of 64 rows folded in order"""
    M = x.shape[0]
    if o.mut == "ragged_chunk" and M % 64:
        x = x[:M - M % 64]
    if not o.tiled:
        return x.sum(0)
    acc = torch.zeros(x.shape[1:], dtype=x.dtype)
    for r0 in range(0, x.shape[0], 64):
        acc = acc + x[r0:r0 + 64].sum(0)
    return acc


def _chan(sums, m2s, counts):
    """(sum, M2) chunk partials [P, ...] with counts [P] -> (mean, M2) in fp64 by Chan's formula, in chunk order"""
    n, mean, m2 = 0.0, None, None
    for s, q, c in zip(sums.double(), m2s.double(), counts):
        if mean is None:
            n, mean, m2 = float(c), s / c, q
            continue
        d = s / c - mean
        tot = n + c
        mean, m2, n = mean + d * (c / tot), m2 + q + d * d * (n * c / tot), tot
    return mean, m2


# ------------------------------------------------------------------------------------------------ conv + BatchNorm + ReLU layers
Layer = collections.namedtuple("Layer", "W b gamma beta rm rv")          # W [N,K], the rest [N]; fp32 on the CPU


def _batch_stats(y, o):
    M = y.shape[0]
    if not o.tiled:
        mean = y.mean(0)
        return mean, ((y - mean) ** 2).mean(0)
    ch = [y[r0:r0 + 64] for r0 in range(0, M, 64)]
    mean, m2 = _chan(torch.stack([c.sum(0) for c in ch]), torch.stack([((c - c.mean(0)) ** 2).sum(0) for c in ch]), [c.shape[0] for c in ch])
    return mean.to(y.dtype), (m2 / M).to(y.dtype)


def _cbr_fwd(x, lay, training, o):
    """x [M,K] holding T values -> (h [M,N] fp32, what the backward needs, (mean, biased var) of the batch | None)"""
    ft = o.ft
    Wt = _rd(lay.W.to(ft), o)
    y = _mm(x, Wt.t(), o) + lay.b.to(ft)
    if training:
        mean, var = _batch_stats(y, o)
    else:
        mean, var = lay.rm.to(ft), lay.rv.to(ft)
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    sc = lay.gamma.to(ft) * rstd
    sh = lay.beta.to(ft) - mean * sc
    pre = y * sc + sh
    return torch.relu(pre), (x, Wt, y, sc, mean, rstd, pre), ((mean, var) if training else None)


def _cbr_bwd(dh, saved, training, o):
    """-> (dX fp32, dW, db, dgamma, dbeta)"""
    x, Wt, y, sc, mean, rstd, pre = saved
    M = y.shape[0]
    g = dh * (pre > 0)
    xhat = (y - mean) * rstd
    sg = _rowsum(g, o)
    sgx = _rowsum((_rd(g, o) if o.mut == "dgamma_from_rounded" else g) * xhat, o)
    terms = training
    if (training and o.mut == "bn_train_terms_dropped") or (not training and o.mut == "bn_eval_terms_kept"):
        terms = not terms
    dY = sc * (g - sg / M - xhat * sgx / M) if terms else sc * g
    dYT = _rd(dY, o)
    dW = _mm(dYT.t(), x, o)
    if o.mut == "db_unmasked":
        sd = _rowsum(dh, o)
        db = _rowsum(_rd(sc * (dh - sd / M - xhat * _rowsum(dh * xhat, o) / M) if terms else sc * dh, o), o)
    else:
        db = _rowsum(dYT, o)
    dX = _mm(dYT, Wt, o)
    if o.mut == "last_quad":
        db, sgx, sg = db.clone(), sgx.clone(), sg.clone()
        db[-4:], sgx[-4:], sg[-4:] = 0, 0, 0
    return dX, dW, db, sgx, sg


def _mlp_forward(x_rows, layers, training, o):
    """-> (out fp32, saved per layer, batch statistics per layer)"""
    x = _rd(x_rows, o)
    saved, stats = [], []
    for li, lay in enumerate(layers):
        h, sv, st = _cbr_fwd(x, lay, training, o)
        saved.append(sv)
        stats.append(st)
        x = _rd(h, o) if li < len(layers) - 1 else h
    return x, saved, stats


def _mlp_model(x_rows, layers, dout_rows, training, o):
    """-> (outputs without the input gradient, d x_rows fp32 still times S)"""
    out, saved, stats = _mlp_forward(x_rows, layers, training, o)
    res = {"out": out}
    dh = dout_rows.to(o.ft) * o.S
    for li in reversed(range(len(layers))):
        dh, dW, db, dg, dbe = _cbr_bwd(dh, saved[li], training, o)
        res.update({f"W{li}": dW, f"b{li}": db, f"g{li}": dg, f"be{li}": dbe})
    M = x_rows.shape[0]
    for li, (lay, st) in enumerate(zip(layers, stats)):
        if st is not None:
            res[f"rm{li}"] = (1 - BN_MOM) * lay.rm.to(o.ft) + BN_MOM * st[0]
            res[f"rv{li}"] = (1 - BN_MOM) * lay.rv.to(o.ft) + BN_MOM * st[1] * (M / (M - 1.0))
    return res, dh


def _unscale(res, o):
    for k in res:
        if k != "out" and not k.startswith("r") and not (o.mut == "unscale_missing" and k == "g0"):
            res[k] = res[k] * (1.0 / o.S)
    return res


def _mlp_exact(x_rows, layers, dout_rows, training):
    """x_rows: an fp64 tensor inside an autograd graph -> (outputs, mags); the caller takes the input gradient from its own leaf"""
    ps = [[t.double().requires_grad_() for t in (l.W, l.b, l.gamma, l.beta)] for l in layers]
    x, keep, res, mag = x_rows, [], {}, {}
    M = x_rows.shape[0]
    for li, (lay, (W, b, ga, be)) in enumerate(zip(layers, ps)):
        y = x @ W.t() + b
        rm, rv = lay.rm.double().clone(), lay.rv.double().clone()
        x = torch.relu(F.batch_norm(y, rm, rv, ga, be, training, BN_MOM, BN_EPS))
        x.retain_grad()
        keep.append((y, x, rm, rv))
        if training:
            res[f"rm{li}"], res[f"rv{li}"] = rm, rv
    x.backward(dout_rows.double())
    res["out"] = x.detach()
    for li, ((W, b, ga, be), (y, h, rm, rv)) in enumerate(zip(ps, keep)):
        res.update({f"W{li}": W.grad, f"b{li}": b.grad, f"g{li}": ga.grad, f"be{li}": be.grad})
        mag[f"be{li}"] = (h.grad * (h.detach() > 0)).abs().sum(0)
    return res, mag


# ------------------------------------------------------------------------------------------------ feature propagation
def _interp(inp, o):
    p2, idx, dist = inp["p2"].to(o.ft), inp["idx"], inp["dist"].to(o.ft)
    B = idx.shape[0]
    recip = 1.0 / (dist + 1e-8)
    w = recip if o.mut == "interp_unnormalised" else recip / recip.sum(-1, keepdim=True)
    rows = (p2[torch.arange(B)[:, None, None], idx] * w[..., None]).sum(2)
    if inp["p1"] is not None:
        rows = torch.cat([inp["p1"].to(o.ft), rows], -1)
    return rows.reshape(-1, rows.shape[-1]), w


def fp_model(inp, training, o):
    idx = inp["idx"]
    B, N, _ = idx.shape
    S, D2 = inp["p2"].shape[1:]
    rows, w = _interp(inp, o)
    res, d_rows = _mlp_model(rows, inp["layers"], inp["dout"].reshape(B * N, -1), training, o)
    res["out"] = res["out"].view(B, N, -1)
    flat = (idx + torch.arange(B).view(B, 1, 1) * S).reshape(-1)
    contrib = d_rows[:, rows.shape[1] - D2:].view(B, N, 1, D2) * w[..., None]
    res["dp2"] = torch.zeros(B * S, D2, dtype=o.ft).index_add_(0, flat, contrib.reshape(-1, D2)).view(B, S, D2)
    return _unscale(res, o)


def fp_exact(inp, training):
    idx = inp["idx"]
    B, N, _ = idx.shape
    p2 = inp["p2"].double().requires_grad_()
    recip = 1.0 / (inp["dist"].double() + 1e-8)
    w = recip / recip.sum(-1, keepdim=True)
    rows = (p2[torch.arange(B)[:, None, None], idx] * w[..., None]).sum(2)
    if inp["p1"] is not None:
        rows = torch.cat([inp["p1"].double(), rows], -1)
    res, mag = _mlp_exact(rows.reshape(B * N, -1), inp["layers"], inp["dout"].reshape(B * N, -1), training)
    res["out"] = res["out"].view(B, N, -1)
    res["dp2"] = p2.grad
    return res, mag


def cbr_model(inp, training, o):
    res, dx = _mlp_model(inp["x"].to(o.ft), inp["layers"], inp["dout"], training, o)
    res["dx"] = dx
    return _unscale(res, o)


def cbr_exact(inp, training):
    x = inp["x"].double().requires_grad_()
    res, mag = _mlp_exact(x, inp["layers"], inp["dout"], training)
    res["dx"] = x.grad
    return res, mag


# ------------------------------------------------------------------------------------------------ DGCNN layer
def _first_max(v):
    """v [B,Q,K,C] -> (max over K, one-hot of the FIRST maximising k, mask of all maximising k)"""
    mx = v.amax(2, keepdim=True)
    eq = v == mx
    return mx[:, :, 0], eq & (eq.cumsum(2) == 1), eq


def _dg_forward(inp, o):
    ft = o.ft
    x_k, idx, W = inp["x_k"].to(ft), inp["idx"], inp["W"].to(ft)
    B, S, C = x_k.shape
    Nq, K = idx.shape[1:]
    Co = W.shape[0]
    WaT = _rd(W[:, :C], o)
    WdT = _rd(W[:, C:] if o.mut == "wd_is_wb" else W[:, C:] - W[:, :C], o)
    xk = _rd(x_k.reshape(B * S, C), o)
    xq = xk if inp["x_q"] is None else _rd(inp["x_q"].to(ft).reshape(B * Nq, C), o)
    P, Q = _mm(xk, WaT.t(), o), _mm(xq, WdT.t(), o)
    if inp.get("dup") is not None:                    # identical source rows give identical P rows, whatever the host GEMM's blocking
        P.view(B, S, Co)[:, inp["dup"][1]] = P.view(B, S, Co)[:, inp["dup"][0]]
    y = P.view(B, S, Co)[torch.arange(B)[:, None, None], idx] + Q.view(B, Nq, 1, Co)
    Cg = Co // GN_GROUPS
    n = Nq * K * Cg
    yg = y.view(B, Nq * K, GN_GROUPS, Cg)
    if not o.tiled:
        mean = yg.mean((1, 3))
        var = ((yg - mean[:, None, :, None]) ** 2).mean((1, 3))
    else:                                             # fp32 (sum, sum of squares) per 64-row chunk and channel, folded in fp64
        s = torch.stack([yg[:, r0:r0 + 64].sum(1) for r0 in range(0, Nq * K, 64)]).double().sum(0).sum(-1)
        q = torch.stack([(yg[:, r0:r0 + 64] ** 2).sum(1) for r0 in range(0, Nq * K, 64)]).double().sum(0).sum(-1)
        mean = (s / n).to(ft)
        var = (q / n - (s / n) ** 2).clamp_min(0).to(ft)
    rstd = 1.0 / torch.sqrt(var + GN_EPS)
    mean_c, rstd_c = mean.repeat_interleave(Cg, 1)[:, None, None], rstd.repeat_interleave(Cg, 1)[:, None, None]
    xhat = (y - mean_c) * rstd_c
    v = F.leaky_relu(xhat * inp["gamma"].to(ft) + inp["beta"].to(ft), SLOPE)
    return v, (xk, xq, WaT, WdT, xhat, rstd_c, n, Cg)


def dg_model(inp, o):
    ft = o.ft
    idx = inp["idx"]
    B, S, C = inp["x_k"].shape
    Nq, K = idx.shape[1:]
    v, (xk, xq, WaT, WdT, xhat, rstd_c, n, Cg) = _dg_forward(inp, o)
    Co = v.shape[-1]
    out, first, eq = _first_max(v)
    gamma = inp["gamma"].to(ft)
    t = inp["dout"].to(ft) * o.S * torch.where(out > 0, torch.ones((), dtype=ft), torch.full((), SLOPE, dtype=ft))
    tz = (eq if o.mut == "tie_to_all" else first) * t[:, :, None]                 # [B,Nq,K,Co]: t at the elements the gradient enters
    if o.tiled:                                       # per-channel fp32 sums over chunks of 32 queries, folded in order
        dgamma, dbeta = torch.zeros(Co, dtype=ft), torch.zeros(Co, dtype=ft)
        a1, a2 = torch.zeros(B, Co, dtype=torch.float64), torch.zeros(B, Co, dtype=torch.float64)
        for q0 in range(0, Nq, 32):
            c_t, c_x = tz[:, q0:q0 + 32], xhat[:, q0:q0 + 32]
            dgamma, dbeta = dgamma + (c_t * c_x).sum((0, 1, 2)), dbeta + c_t.sum((0, 1, 2))
            a1, a2 = a1 + (gamma * c_t).sum((1, 2)).double(), a2 + (gamma * c_t * c_x).sum((1, 2)).double()
        a1, a2 = a1.to(ft), a2.to(ft)
    else:
        dgamma, dbeta = (tz * xhat).sum((0, 1, 2)), tz.sum((0, 1, 2))
        a1, a2 = (gamma * tz).sum((1, 2)), (gamma * tz * xhat).sum((1, 2))
    nn = float(Nq * K) if o.mut == "gn_n_without_cg" else float(n)
    S1 = (a1.view(B, GN_GROUPS, Cg).sum(-1) / nn).repeat_interleave(Cg, 1)[:, None, None]
    S2 = (a2.view(B, GN_GROUPS, Cg).sum(-1) / nn).repeat_interleave(Cg, 1)[:, None, None]
    dy = rstd_c * (gamma * tz - (S1 + xhat * S2))
    flat = (idx + torch.arange(B).view(B, 1, 1) * S).reshape(-1)
    dP = torch.zeros(B * S, Co, dtype=ft).index_add_(0, flat, dy.reshape(-1, Co))
    dQ = dy.sum(2).reshape(B * Nq, Co)
    dPT, dQT = _rd(dP, o), _rd(dQ, o)
    dWa, dWd = _mm(dPT.t(), xk, o), _mm(dQT.t(), xq, o)
    dxk, dxq = _mm(dPT, WaT, o).view(B, S, C), _mm(dQT, WdT, o).view(B, Nq, C)
    res = {"out": out, "W": torch.cat([dWa - dWd, dWd], 1), "g0": dgamma, "be0": dbeta}
    if inp["x_q"] is None:
        res["dx_k"] = dxk + dxq
    else:
        res["dx_k"], res["dx_q"] = dxk, dxq
    return _unscale(res, o)


def dg_exact(inp):
    idx = inp["idx"]
    B = idx.shape[0]
    xk = inp["x_k"].double().requires_grad_()
    xq = xk if inp["x_q"] is None else inp["x_q"].double().requires_grad_()
    W, ga, be = (inp[k].double().requires_grad_() for k in ("W", "gamma", "beta"))
    nb = xk[torch.arange(B)[:, None, None], idx]                                  # [B,Nq,K,C]
    q = xq[:, :, None].expand(-1, -1, idx.shape[2], -1)
    y = (torch.cat([nb - q, q], -1) @ W.t()).permute(0, 3, 1, 2)                 # [B,Co,Nq,K]
    v = F.leaky_relu(F.group_norm(y, GN_GROUPS, ga, be, GN_EPS), SLOPE).permute(0, 2, 3, 1)
    _, first, _ = _first_max(_dg_forward(inp, Opt(ft=torch.float64))[0])          # (the twin rows of the tie case: exact ties there)
    out = (v * first).sum(2)                                                      # the max, gradient to the first maximiser
    out.backward(inp["dout"].double())
    res = {"out": out.detach(), "W": W.grad, "g0": ga.grad, "be0": be.grad, "dx_k": xk.grad}
    if inp["x_q"] is not None:
        res["dx_q"] = xq.grad
    t = inp["dout"].double() * torch.where(out.detach() > 0, torch.ones((), dtype=torch.float64), torch.full((), SLOPE, dtype=torch.float64))
    return res, {"be0": t.abs().sum((0, 1))}


def dg_margin(inp, o):
    """[B,Nq,Co]: the winner's lead over the best neighbour that is not the same source row (nor its declared duplicate)"""
    v, _ = _dg_forward(inp, o)
    return _margin(v, inp["idx"], inp.get("dup"))


def _margin(v, idx, dup):
    src = idx if dup is None else torch.where(idx == dup[1], dup[0], idx)
    best, first, _ = _first_max(v)
    win = (src[..., None] * first).sum(2)                                         # [B,Nq,Co]: the winner's source row
    other = src[..., None] != win[:, :, None]
    return best - torch.where(other, v, torch.full_like(v, float("-inf"))).amax(2)


# ------------------------------------------------------------------------------------------------ the criterion
def ratio(x, model, ref, mag=None):
    """tensors [..., C] -> (max over channel groups of ||x - ref|| / (||model - ref|| + floor), first channel of that group)"""
    C = ref.shape[-1]
    r = ref.double().reshape(-1, C)
    e_x = ((x.double().reshape(-1, C) - r) ** 2).sum(0)
    e_m = ((model.double().reshape(-1, C) - r) ** 2).sum(0)
    m = ((r if mag is None else mag.double().reshape(-1, C)) ** 2).sum(0)
    if GROUP > 1:
        pad = (-C) % GROUP
        e_x, e_m, m = (F.pad(t, (0, pad)).view(-1, GROUP).sum(1) for t in (e_x, e_m, m))
    e_x, e_m, m = e_x.sqrt(), e_m.sqrt(), m.sqrt()
    den = e_m + e_m.median() + 2.0 ** -23 * m
    q = torch.where(den > 0, e_x / den.clamp_min(1e-300), torch.where(e_x > 0, float("inf"), 0.0).double())
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    i = int(q.argmax())
    return float(q[i]), i * GROUP


def ratios(x, model, ref, mag, skip=()):
    """dicts of outputs -> {name: (ratio, channel)} over the outputs of `ref`"""
    return {k: ratio(x[k], model[k], ref[k], mag.get(k)) for k in ref if k not in skip}


# ------------------------------------------------------------------------------------------------ the cases
Case = collections.namedtuple("Case", "node name shape note")
CASES = (
    Case("fp", "m640", (2, 320, 96, 19, 64, (128, 48)), "M = 640: statistics from the GEMM epilogue; K = 83 is padded"),
    Case("fp", "m330", (1, 330, 96, 19, 64, (128, 48)), "M % 32 != 0: rows_stats, transposed-copy weight gradient, last chunk of 10 rows"),
    Case("fp", "nop1", (2, 96, 40, 0, 64, (128, 48)), "points1 = None"),
    Case("dg", "layer1", (1, 2, 96, 160, False), "distinct sources and queries"),
    Case("dg", "layer2", (2, 2, 96, 96, False), "one tensor is both operands: the gradient reaches it twice"),
    Case("dg", "nq33", (1, 2, 40, 33, False), "a ragged chunk of 32 queries in the backward sums"),
    Case("dg", "tie", (1, 1, 40, 33, True), "two identical source rows: ties in every channel of their queries"),
    Case("cbr", "m640", (640, 83, 128), "statistics from the GEMM epilogue; dX comes back with K = 83 columns"),
    Case("cbr", "m330", (330, 147, 128), "ragged everything"),
)
GENERIC = (      # the un-fused path of PointNetFeaturePropagation (ops through _Linear and _BatchNormReLURows): fp32 bound only
    Case("fp", "s1", (2, 96, 1, 19, 64, (128, 48)), "S == 1: points2 repeated"),
    Case("fp", "mlp3", (2, 96, 40, 19, 64, (64, 32, 24)), "three layers"),
)
BY_ID = {f"{c.node}-{c.name}": c for c in CASES + GENERIC}
DG_WIDTHS = {1: (384, 512), 2: (512, 384)}                                       # layer -> (C, Cout) of DGCNN_Propagation
DG_K = 4


def case_id(c):
    return f"{c.node}-{c.name}"


def knn(query, source, k):
    """[B,Q,3], [B,S,3] -> (idx [B,Q,k] i64, squared distances [B,Q,k] f32): the k nearest under (distance, index)"""
    d = ((query.double()[:, :, None] - source.double()[:, None]) ** 2).sum(-1)
    ds, idx = torch.sort(d, dim=-1, stable=True)
    return idx[..., :k].contiguous(), ds[..., :k].float().contiguous()


def _layer(gen, K, N):
    r = lambda *s: torch.randn(*s, generator=gen)
    return Layer(r(N, K) / K ** 0.5, 0.1 * r(N), 1 + 0.2 * r(N), 0.3 * r(N), 0.3 * r(N), 0.5 + torch.rand(N, generator=gen))


def _raw_inputs(c, gen):
    r = lambda *s: torch.randn(*s, generator=gen)
    if c.node == "cbr":
        M, K, N = c.shape
        return {"x": r(M, K), "layers": [_layer(gen, K, N)], "dout": r(M, N)}
    if c.node == "fp":
        B, N, S, D1, D2, mlp = c.shape
        xyz1, xyz2 = r(B, N, 3), r(B, S, 3)
        idx, dist = knn(xyz1, xyz2, min(3, S))
        layers, K = [], D1 + D2
        for n in mlp:
            layers.append(_layer(gen, K, n))
            K = n
        return {"xyz1": xyz1, "xyz2": xyz2, "idx": idx, "dist": dist, "p1": r(B, N, D1) if D1 else None, "p2": r(B, S, D2),
                "layers": layers, "dout": r(B, N, mlp[-1])}
    layer, B, S, Nq, tie = c.shape
    C, Co = DG_WIDTHS[layer]
    coor, x_k = r(B, S, 3), r(B, S, C)
    dup = None
    if tie:
        dup = (5, 6)
        coor[:, 6], x_k[:, 6] = coor[:, 5], x_k[:, 5]
    same = layer == 2
    coor_q = coor if same else r(B, Nq, 3)
    if tie:
        coor_q[:, :8] = coor[:, 5:6] + 0.05 * r(B, 8, 3)                          # eight queries next to the twin rows
    idx, _ = knn(coor_q, coor, DG_K)
    return {"coor": coor, "coor_q": coor_q, "x_k": x_k, "x_q": None if same else r(B, Nq, C), "idx": idx, "W": r(Co, 2 * C) / (2 * C) ** 0.5,
            "gamma": 1 + 0.2 * r(Co), "beta": 0.1 * r(Co), "dout": r(B, Nq, Co), "dup": dup}


_VIEWS = ((Opt(ft=torch.float64), MARGIN), (Opt(T=F16), MARGIN_ROUNDED), (Opt(T=BF16), MARGIN_ROUNDED))


def _nudge(W, bad_channels, ok, gen, ncols=None):
    """one element (among the first ncols) of each offending row of W moved until ok(channel, row) -> number of elements changed"""
    scale = float(W.std())
    for c in bad_channels:
        for _ in range(5000):
            w2 = W[c].clone()
            col = int(torch.randint(ncols or W.shape[1], (1,), generator=gen))
            w2[col] += scale * float(0.05 + 0.25 * torch.rand(1, generator=gen)) * (1 if torch.rand(1, generator=gen) < 0.5 else -1)
            if ok(c, w2):
                W[c] = w2
                break
        else:
            raise RuntimeError("conditioning: no nudge found")
    return len(bad_channels)


def _mlp_operands(inp, c, li):
    """the operand of layer li in every (model, mode) it is computed in"""
    ops_ = []
    for o, thr in _VIEWS:
        for training in (True, False):
            rows = _interp(inp, o)[0] if c.node == "fp" else inp["x"].to(o.ft)
            x = _rd(rows, o)
            for lj in range(li):
                x = _rd(_cbr_fwd(x, inp["layers"][lj], training, o)[0], o)
            ops_.append((x, o, training, thr))
    return ops_


def _condition_mlp(inp, c, gen):
    nudged = 0
    for li in range(len(inp["layers"])):
        for _ in range(8):
            lay = inp["layers"][li]
            views = _mlp_operands(inp, c, li)

            def worst(ch, wrow):
                """min over the views of min |pre-activation| / threshold of channel ch with the weight row wrow"""
                m = float("inf")
                one = Layer(wrow[None], lay.b[ch:ch + 1], lay.gamma[ch:ch + 1], lay.beta[ch:ch + 1], lay.rm[ch:ch + 1], lay.rv[ch:ch + 1])
                for x, o, training, thr in views:
                    m = min(m, float(_cbr_fwd(x, one, training, o)[1][6].abs().min()) / thr)
                return m
            bad = [ch for ch in range(lay.W.shape[0]) if worst(ch, lay.W[ch]) < 1.0]
            if not bad:
                break
            nudged += _nudge(lay.W, bad, lambda ch, w: worst(ch, w) >= 1.0, gen)
    return nudged


def _condition_dg(inp, gen):
    nudged = 0
    C = inp["x_k"].shape[2]
    for _ in range(8):
        margins = [(dg_margin(inp, o), thr) for o, thr in _VIEWS]
        bad = sorted(set(int(ch) for m, thr in margins for ch in (m < thr).any(0).any(0).nonzero().flatten()))
        if not bad:
            break
        frozen = []                                   # per view: operands and the group statistics, frozen while one channel moves
        for o, thr in _VIEWS:
            v, (xk, xq, _, _, xhat, rstd_c, n, Cg) = _dg_forward(inp, o)
            ft = o.ft
            W = inp["W"].to(ft)
            y = (xhat / rstd_c)                                                  # y - mean
            frozen.append((o, thr, xk, xq, rstd_c, y, W))

        def ok(ch, wrow):
            B, S, _ = inp["x_k"].shape
            idx = inp["idx"]
            for o, thr, xk, xq, rstd_c, ym, W in frozen:
                w = wrow.to(o.ft)
                old = W[ch]
                dP = xk @ (_rd(w[:C], o) - _rd(old[:C], o))
                dQ = xq @ (_rd(w[C:] - w[:C], o) - _rd(old[C:] - old[:C], o))
                ych = ym[..., ch] + dP.view(B, S)[torch.arange(B)[:, None, None], idx] + dQ.view(B, -1, 1)
                v = F.leaky_relu(ych * rstd_c[..., ch] * inp["gamma"][ch].to(o.ft) + inp["beta"][ch].to(o.ft), SLOPE)
                if float(_margin(v[..., None], idx, inp.get("dup")).min()) < 1.1 * thr:
                    return False
            return True
        nudged += _nudge(inp["W"], bad, ok, gen, ncols=C)          # (a Wb column moves Q only: no lead changes)
    return nudged


@functools.lru_cache(maxsize=None)
def inputs(c):
    """-> the case's inputs on the CPU (fp32; seeded per case; conditioned), with 'nudged': the share of input values moved"""
    gen = torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()))
    inp = _raw_inputs(c, gen)
    n = _condition_dg(inp, gen) if c.node == "dg" else _condition_mlp(inp, c, gen)
    total = sum(t.numel() for t in _float_inputs(inp))
    inp["nudged"] = n / total
    return inp


def _float_inputs(inp):
    ts = [v for k, v in inp.items() if isinstance(v, torch.Tensor) and v.is_floating_point() and k not in ("dist", "xyz1", "xyz2", "coor", "coor_q")]
    for lay in inp.get("layers", ()):
        ts += list(lay)
    return ts


def conditioning(c):
    """-> (smallest |BatchNorm pre-activation| or arg-max lead in fp64, the same in the two rounding models, share nudged)"""
    inp = inputs(c)
    worst = []
    for o, _ in _VIEWS:
        if c.node == "dg":
            worst.append(float(dg_margin(inp, o).min()))
        else:
            m = float("inf")
            for training in (True, False):
                rows = _interp(inp, o)[0] if c.node == "fp" else inp["x"].to(o.ft)
                for sv in _mlp_forward(rows, inp["layers"], training, o)[1]:
                    m = min(m, float(sv[6].abs().min()))
            worst.append(m)
    return worst[0], min(worst[1:]), inp["nudged"]


def exact(c, training=True, inp=None):
    inp = inputs(c) if inp is None else inp
    return {"fp": fp_exact, "cbr": cbr_exact}[c.node](inp, training) if c.node != "dg" else dg_exact(inp)


def model(c, o, training=True, inp=None):
    inp = inputs(c) if inp is None else inp
    return {"fp": fp_model, "cbr": cbr_model}[c.node](inp, training, o) if c.node != "dg" else dg_model(inp, o)


def rounded(c, T, training=True, S=1.0, mut=None, inp=None):
    return model(c, Opt(T=T, S=S, mut=mut), training, inp)


def rounded_tiled(c, T, training=True, S=1.0, inp=None):
    return model(c, Opt(T=T, S=S, tiled=True), training, inp)


@functools.lru_cache(maxsize=None)
def exact_cached(c, training):
    return exact(c, training)


@functools.lru_cache(maxsize=None)
def references(c, T, training=True, S=1.0):
    """-> (exact outputs, mags, rounded(T) outputs at gradient scale S) of a case, built once and shared; do not modify"""
    ref, mag = exact_cached(c, training)
    return ref, mag, rounded(c, T, training, S=S)


def pow2_floor(n):
    """the gradient scale a 16-bit node picks for n rows when nothing else is announced: 2^floor(log2 n)"""
    return float(2 ** max(0, int(n).bit_length() - 1))


def rows(c):
    """the rows a case's node sees (its default gradient scale is pow2_floor of it)"""
    return c.shape[0] if c.node == "cbr" else c.shape[0] * c.shape[1] if c.node == "fp" else c.shape[1] * c.shape[3]
