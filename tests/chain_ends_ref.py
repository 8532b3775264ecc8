"""Shared by tests/test_chain_ends_ref_cpu.py and tests/test_chain_ends_gpu.py: the small fp32 kernels at the two ends of the text
chain when only the prompt trains (head_type 0) -- LayerNorm forward / backward and their split-K consumer forms (csrc/norm.hip),
ppt_rows_matmul_f32, ppt_head_logits, ppt_head_ce_bwd (csrc/head.hip), ppt_prompt_rows / ppt_prompt_rows_bwd (csrc/optim.hip) -- in
plain torch on the CPU (no ppt_amd import): the case table, the inputs, the fp64 references, the criterion, a correct fp32
stand-in in another summation order and the mutations that break it.

  CASES      one flat list; Case.note names the edge a case is for, family(case, output) the kernel a failure belongs to,
             branches(case) the dispatch branches it takes; _assert_coverage() fails when a kernel or branch has no case.
  inputs     every operand as plain fp32 values, seeded per case (torch.Generator on the CPU); place() puts one inside a NaN-filled
             (operands) or sentinel-filled (caller-owned outputs) buffer, 16 bytes in -- or 20, one float off, for the
             misalignment cases.
  reference  {output: Ref(exact fp64, E, R, bits)}.  tol = E + R; E what fp32 arithmetic may err (below), R the half ulp of a
             16-bit store (0 for fp32: its last rounding is inside E); bits, where the summation order is documented and
             fp32-sequential, the value that must come out bit for bit.
  standin    the same operation in fp32 in ANOTHER order (columns permuted, torch's blocked sums); `mutate` breaks it on purpose.
  check      worst |x - exact| / (cap E + R) per output; a result passes iff that is <= 1, nothing is NaN and the bits match.

The references follow the model's formulas: LayerNorm (ULIP_models.py:21-27), x = prompts + positional_embedding, ln_final on the
EOT rows, x @ text_projection (:210-222), pc_embed = feat @ pc_projection (:257), text / text.norm (:279), logits =
exp(logit_scale) pc_embed @ text^T (:281), CrossEntropyLoss(label_smoothing) with mean reduction (main_cls.py:52,196).

The bound E (u = 2^-24; first order, any summation order; nothing in it is measured except the two fast-math figures):
  sum of n terms    n u sum |t|              (n - 1 additions in any order, + 1 for a scale or division that follows)
  dot product       (K + 2) u (|a| . |w|)    (rows_matmul, the projection; times the carried factor alpha or exp(s))
  LayerNorm forward row r known within Er (u |r| for x + add, (S + 1) u sum |terms| for the split-K consumer):
        mean   Em = (D + 1) u mean|r| + mean(Er);  d = r - mean within e = Em + Er + u |d|
        var    Ev = mean(2 |d| e + e^2) + (D + 2) u var + u (var + eps)
        rstd   Ers = (var + eps - Ev)^-1/2 - rstd + 6 u rstd        (sqrt, division, and the eps argument's own rounding)
        y      Ey = |w| (e rstd + |d| Ers + e Ers) + 3 u |d rstd w| + u |y|
  LayerNorm backward with mean, rstd GIVEN (fp32 operands; Emu = Ers = 0) or the forward's own (the chained case: Em, Ers above):
        dy     Edy = S u sum_z |dy_z| for S > 1 slices, else 0;   g = dy w within Eg = |w| Edy + u |g|
        xhat   Exh = 2 u |xhat| + (Emu + Ex) rstd + |x - mu| Ers      (Ex: the summed row's own bound, chained case only)
        s1     mean(Eg) + (D + 1) u mean|g|;   s2: mean(Eg |xhat| + |g| Exh + u |g xhat|) + (D + 1) u mean|g xhat|
        dx     rstd (Eg + Es1 + |xhat| Es2 + |s2| Exh + 3 u (|g| + |s1| + |xhat s2|)) + |inner| Ers + u |r|, + u |dx0 + r| accumulated
        copy   the same E; R = half an ulp of the copy's format at |dx| + E
        dw     sum_rows (|dy| Exh + u |dy xhat|) + (M + 1) u sum_rows |dy xhat|;  db  (M + 1) u sum_rows |dy|
  head  pc = feat W within (F + 2) u |feat| |W|;  spc = exp(s) pc: + |spc| (expf(s) + u)
        dot = spc . t within sum (Espc |t|) + (E + 1) u sum |spc t|;  logits = dot / |t|: E / |t| + |logit| ((E + 1) u / 2 + 3 u)
        CE row: a_c = L_c - max;  se within se_rel = sum_c softmax_c (expf(a_c) + u |a_c| + u) + (C + 1) u;
                lse within Else = se_rel + logf(se) + 2 u |lse| + u |max|, + max_c EL_c from the logits' own error
                row loss within 2 max_c EL_c + Else + u (4 |lse| + 4 |L_y| + (C + 4) mean|L|);  loss: mean + (B + 2) u mean|row loss|
        dlogits = (p - target) / B, p = exp(L_c - lse): p (EL_c + max EL) + p (expf(L_c - lse) + u |L_c - lse| + Else + u) + 3 u (p + target)
        d text: dtn = dlogits^T spc, tn = t / |t| within |tn| ((E + 1) u / 2 + 3 u), proj = dtn . tn, (dtn - tn proj) / |t|: each
                product and sum as above
  expf(x), logf(x)  the fast __expf / __logf of the head kernels: |__expf(x) - e^x| <= (EXPF_A + EXPF_B |x|) u e^x + 2^-126 and
        |__logf(x) - ln x| <= (LOGF_A |ln x| + LOGF_B) u.  The ROCm device-library documents installed with the compiler give no error
        figure for either, so the figures are the a-priori ones of their lowering (one hardware exp2 / log2 at 1 ulp = 2 u of its
        result, one fp32 multiply by log2(e) resp. ln 2: x (1 + 1.5 u) log2(e) moves e^x by 1.5 u |x|) rounded up, and
        test_chain_ends_gpu.py MEASURES both on a dense grid through ops.head_loss against fp64 and fails if either is exceeded.
"""
import collections
import functools
import math
import zlib

import torch

U = 2.0 ** -24
FMT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
ROUND = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}            # half an ulp of a value in [1, 2)
_MINHALF = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
SENTINEL = {4: 0x5EA7C0DE, 2: 0x5EA7}                                        # finite in every format; by element size
EXPF_A, EXPF_B = 4.0, 2.0
LOGF_A, LOGF_B = 4.0, 1.0
SCALE = {"init": math.log(1 / 0.07), "max": math.log(100.0)}                 # logit_scale at its initial value and at its clamp

_FIELDS = dict(op="", M=0, D=0, y="f32", add="", xs="", mis="", stats=True, eps=1e-5, S=0, bias=False, hard=False, acc=False, copy="",
               prows=0, K=0, N=0, alpha=1.0, B=0, F=0, E=0, C=0, smooth=0.2, scale="init", labels="rand", close=False, W=0, max_rows=0, sc=1.0,
               note="")
Case = collections.namedtuple("Case", list(_FIELDS), defaults=list(_FIELDS.values()))
Ref = collections.namedtuple("Ref", "exact E R bits", defaults=(None,))
N_TOK, N_BASE = 5, 3                                                        # the synthetic prompt layouts: tokens, rows that stay base rows


def case_id(c):
    s = c.op
    for k, d in _FIELDS.items():
        v = getattr(c, k)
        if k in ("op", "note") or v == d:
            continue
        s += f"-{k}" if v is True else f"-{k}{v:g}" if isinstance(v, float) else f"-{k}{v}"
    return s


def _wide8(c):
    return c.D % 8 == 0 and c.D <= 512 and not c.mis


def _project8(c, K):
    return K <= 1536 and K % 32 == 0 and c.mis != "feat"


def family(c, output=None):
    """the kernel a failure of `output` of case c belongs to (the shapes choose: the host functions of csrc/norm.hip, head.hip)"""
    if c.op in ("ln_fwd", "ln_fwd_sum"):
        return "ln_fwd_vec8_kernel" + ("<SUM>" if c.op == "ln_fwd_sum" else "") if _wide8(c) else "ln_fwd_kernel"
    if c.op in ("ln_bwd", "ln_bwd_sum"):
        return "ln_bwd_dx8_kernel" + (f" (S = {c.S} slices)" if c.S else "") if _wide8(c) else "ln_bwd_kernel (dx only, waves = M)"
    if c.op == "ln_bwd_w":
        return "ln_bwd_w8_kernel" if _wide8(c) else "ln_bwd_kernel"
    if c.op == "ln_chain":
        return "ln_fwd_vec8_kernel" if output in ("y", "mean", "rstd") else "ln_bwd_dx8_kernel"
    if c.op == "matmul":
        return "head_project8_kernel (ppt_rows_matmul_f32)"
    if c.op == "head":
        if output in ("loss", "d_text"):
            return "head_ce_bwd_kernel"
        return ("head_project8_kernel" if _project8(c, c.F) else "head_project_kernel") + " + head_logits_kernel"
    return {"rows": "prompt_rows_kernel", "rows_bwd": "prompt_rows_bwd_kernel"}[c.op]


def _lnw_geometry(c):
    """(rows per wave, partial rows used, partial rows) of ppt_layernorm_bwd with weight gradients"""
    p = c.prows or max(256, min(4096, (c.M + 15) // 16))
    rpw = (c.M + p - 1) // p
    return rpw, (c.M + rpw - 1) // rpw, p


def branches(c):
    """the dispatch branches and edges case c reaches, as tags (the coverage assertion's vocabulary)"""
    t = set()
    if c.op in ("ln_fwd", "ln_fwd_sum"):
        k = "vec8" if _wide8(c) else "scalar"
        t |= {f"ln_fwd:{k}", f"ln_fwd:{k}:{c.y}", f"ln_fwd:{k}:D{c.D}", f"ln_fwd:M{c.M}", f"ln_fwd:eps{c.eps:g}", f"ln_fwd:stats{int(c.stats)}"}
        if c.mis:
            t.add(f"ln_fwd:scalar:D{c.D}:mis_{c.mis}")
        if c.op == "ln_fwd" and k == "vec8" and c.M > 8192:
            t.add("ln_fwd:vec8:rowloop")
        if c.add:
            t.add(f"ln_fwd:add_{c.add}")
        if c.xs:
            t.add(f"ln_fwd:xs_{c.xs}")
        if c.hard:
            t.add(f"ln_fwd:{k}:hard")
        if c.op == "ln_fwd_sum":
            t |= {f"ln_fwd_sum:S{c.S}", f"ln_fwd_sum:bias{int(c.bias)}", f"ln_fwd_sum:{c.y}"}
    elif c.op in ("ln_bwd", "ln_bwd_sum"):
        k = "dx8" if _wide8(c) else "scalar"
        t |= {f"ln_bwd:{k}", f"ln_bwd:{k}:D{c.D}", f"ln_bwd:{k}:acc{int(c.acc)}", f"ln_bwd:{k}:copy_{c.copy or 'none'}", f"ln_bwd:M{c.M}"}
        if k == "scalar":
            t.add("ln_bwd:scalar:" + ("mis_" + c.mis if c.mis else "D>512" if c.D > 512 else "D%8"))
        if c.op == "ln_bwd_sum":
            t |= {f"ln_bwd_sum:S{c.S}", f"ln_bwd_sum:acc{int(c.acc)}"}
    elif c.op == "ln_bwd_w":
        rpw, used, p = _lnw_geometry(c)
        k = "w8" if _wide8(c) else "scalar_w"
        t |= {f"ln_bwd:{k}", f"ln_bwd:{k}:prows{c.prows}", f"ln_bwd:{k}:" + ("rpw1" if rpw == 1 else "rpw>1")}
        if rpw > 1 and c.M % rpw:
            t.add(f"ln_bwd:{k}:ragged")
        if used < p:
            t.add(f"ln_bwd:{k}:memset_tail")
    elif c.op == "ln_chain":
        t.add("ln_chain")
    elif c.op in ("matmul", "head"):
        K, Bn, En = (c.K, c.M, c.N) if c.op == "matmul" else (c.F, c.B, c.E)
        who = c.op
        if _project8(c, K):
            fq = K // 8
            t.add(f"{who}:project8")
            t.add(f"{who}:project8:" + ("tail4_only" if fq < 16 else "loop16+tail4" if fq % 16 else "loop16_only"))
            if En % 64:
                t.add(f"{who}:project8:E%64")
            if K == 1536:
                t.add(f"{who}:project8:lds64k")
            if Bn % 8:
                t.add(f"{who}:project8:B{Bn}")
        else:
            t.add("head:fallback:" + ("mis_feat" if c.mis == "feat" else "F>1536" if K > 1536 else "F%32"))
        if c.op == "matmul":
            t.add(f"matmul:alpha{c.alpha:g}")
        else:
            t |= {f"ce:smooth{c.smooth:g}", f"ce:scale_{c.scale}", f"ce:labels_{c.labels}"}
            if c.C > 64:
                t.add("ce:C>64")
            if c.B == 4096:
                t.add("ce:B4096")
            if c.close and c.C > 64:
                t.add("ce:C>64:every_class_in_the_softmax")
    else:
        t |= {f"{c.op}:W{c.W}", f"{c.op}:max_rows{c.max_rows}"}
        if c.op == "rows_bwd":
            t |= {f"rows_bwd:scale{c.sc:g}", "rows_bwd:unused_token", "rows_bwd:full_list"}
            if c.max_rows % 8:
                t.add("rows_bwd:max_rows%8")
    return t


# ------------------------------------------------------------------------------------------------ placement (GPU test, and its CPU check)
def place(vals, misaligned=False, sentinel=False):
    """vals -> (flat buffer, window): the values as a contiguous window 4 elements (16 bytes) into a buffer of NaN (an operand: a
    read outside it poisons the result) or of the sentinel (a caller-owned output), 5 elements when misaligned; 16 more behind"""
    off = 5 if misaligned else 4
    buf = torch.empty(off + vals.numel() + 16, dtype=vals.dtype)
    if sentinel:
        bits(buf).fill_(SENTINEL[buf.element_size()])
    else:
        buf.fill_(float("nan"))
    win = buf[off:off + vals.numel()].view(vals.shape)
    win.copy_(vals)
    return buf, win


def window(buf, shape, misaligned=False):
    """the window place() made, inside `buf` or a copy of it on another device"""
    off = 5 if misaligned else 4
    return buf[off:off + math.prod(shape)].view(shape)


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def outside_same(buf, before, shape, misaligned=False):
    """every element of `buf` outside the window holds the bits it held in `before`"""
    inside = torch.zeros(buf.numel(), dtype=torch.bool)
    window(inside, shape, misaligned).fill_(True)
    return bool((bits(buf.cpu())[~inside] == bits(before.cpu())[~inside]).all())


# ------------------------------------------------------------------------------------------------ inputs
def _ln_rows(c, gen, M, D):
    x = 0.5 + 2.0 * torch.randn(M, D, generator=gen)
    if c.hard:                    # what the text tower feeds its LayerNorms: outlier channels and a large row mean
        x[:, ::37] *= 20.0
        x += 50.0 * (2.0 * torch.randint(0, 2, (M, 1), generator=gen) - 1.0)
    return x


def layout(c, gen):
    """a synthetic prompt layout -> (slot [rows] i32, rows_of [N_TOK, max_rows] i32): token 0 fills its list (no -1 terminator),
    token 1 is used by no row, the others take (max_rows + 1) // 2, max_rows - 1 and min(max_rows, 1) rows; N_BASE rows stay base
    rows; the rows are shuffled, each token's list ascending"""
    mr = c.max_rows
    counts = [mr, 0, (mr + 1) // 2, mr - 1, min(mr, 1)]
    ids = torch.tensor([t for t, n in enumerate(counts) for _ in range(n)] + [-1] * N_BASE, dtype=torch.int32)
    slot = ids[torch.randperm(ids.numel(), generator=gen)]
    rows_of = torch.full((N_TOK, mr), -1, dtype=torch.int32)
    for t in range(N_TOK):
        r = torch.nonzero(slot == t)[:, 0].to(torch.int32)
        rows_of[t, :r.numel()] = r
    return slot, rows_of


@functools.lru_cache(maxsize=8)
def inputs(c):
    """the operands of case c: a dict of CPU tensors (fp32 values; int32 / int64 indices), seeded by the case's id"""
    gen = torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()))
    rn = lambda *s: torch.randn(*s, generator=gen)
    I = {}
    M, D = c.M, c.D
    if c.op.startswith("ln"):
        I["w"], I["b"] = 1.0 + 0.3 * rn(D), 0.2 * rn(D)
    if c.op in ("ln_fwd", "ln_chain"):
        I["x"] = _ln_rows(c, gen, M, D)
        if c.add:
            I["add"] = 0.5 * rn({"full": M, "rows1": 1, "rows7": 7}[c.add], D)
    if c.op == "ln_fwd_sum":
        I["x"], I["parts"] = _ln_rows(c, gen, M, D), 0.5 * rn(c.S, M, D)
        if c.bias:
            I["bias"] = 0.5 * rn(D)
    if c.op in ("ln_bwd", "ln_bwd_sum", "ln_bwd_w", "ln_chain"):
        if c.op != "ln_chain":
            I["xs"] = _ln_rows(c, gen, M, D)
            st = ln_fwd64(I["xs"].double(), I["w"].double(), I["b"].double(), c.eps)
            I["mean"], I["rstd"] = st["mean"].float(), st["rstd"].float()         # the fp64 statistics rounded to fp32: operands
        I["dy"] = rn(c.S, M, D) if c.S else rn(M, D)
        I["dx0"] = rn(M, D)
    if c.op == "matmul":
        I["a"], I["w"] = rn(M, c.K), rn(c.K, c.N) / math.sqrt(c.K)
    if c.op == "head":
        I["feat"], I["w"], I["text"] = rn(c.B, c.F), rn(c.F, c.E) / math.sqrt(c.F), 0.3 * rn(c.C, c.E)
        if c.close:               # class prompts that resemble each other, as real ones do: every class keeps a share of the softmax
            I["text"] = 0.3 * rn(1, c.E) + 0.015 * rn(c.C, c.E)
        I["scale"] = torch.tensor([SCALE[c.scale]], dtype=torch.float32)
        I["labels"] = (torch.randint(0, c.C, (c.B,), generator=gen) if c.labels == "rand" else torch.full((c.B,), c.C // 2)).long()
    if c.op in ("rows", "rows_bwd"):
        I["slot"], I["rows_of"] = layout(c, gen)
        R = I["slot"].numel()
        if c.op == "rows":
            I["base"], I["pos"], I["tokens"] = rn(R, c.W), rn(R, c.W), rn(N_TOK, c.W)
        else:
            I["g"] = rn(R, c.W)
    return I


# ------------------------------------------------------------------------------------------------ fp64 references
def ln_fwd64(r, w, b, eps):
    mean = r.mean(1)
    d = r - mean[:, None]
    var = (d * d).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    return dict(y=d * rstd[:, None] * w + b, mean=mean, rstd=rstd)


def ln_bwd64(dy, x, w, mu, rs):
    g = dy * w
    xh = (x - mu[:, None]) * rs[:, None]
    s1, s2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    return dict(dx=rs[:, None] * (g - s1 - xh * s2), dw=(dy * xh).sum(0), db=dy.sum(0))


def head64(feat, w, text, s, labels, smooth):
    B, C = feat.shape[0], text.shape[0]
    spc = torch.exp(s) * (feat @ w)
    n = text.norm(dim=1, keepdim=True)
    tn = text / n
    logits = spc @ tn.t()
    lse = torch.logsumexp(logits, 1, keepdim=True)
    logp = logits - lse
    onehot = torch.zeros_like(logits).scatter_(1, labels[:, None], 1.0)
    rowloss = (1.0 - smooth) * -(logp * onehot).sum(1) + smooth * -logp.mean(1)
    dlogits = (torch.exp(logp) - ((1.0 - smooth) * onehot + smooth / C)) / B
    dtn = dlogits.t() @ spc
    d_text = (dtn - tn * (dtn * tn).sum(1, keepdim=True)) / n
    return dict(logits=logits, loss=rowloss.mean(), d_text=d_text)


def rows64(base, slot, tokens, pos):
    s = slot.long()
    return torch.where((s >= 0)[:, None], tokens[s.clamp_min(0)] + pos, base)


def rows_bwd64(g, rows_of, scale):
    r = rows_of.long()
    return scale * (g[r.clamp_min(0)] * (r >= 0)[:, :, None]).sum(1)


# ------------------------------------------------------------------------------------------------ the bounds
def _half_ulp(v, dt):
    return (ROUND[dt] * torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(1e-300))))).clamp_min(_MINHALF[dt])


def _ref(v, E, fmt="f32", bits_=None):
    dt = FMT[fmt]
    R = torch.zeros_like(v) if dt == torch.float32 else _half_ulp(v.abs() + E, dt)
    return Ref(v, E, R, bits_)


def expf_err(x):
    """relative error of __expf at x (docstring)"""
    return (EXPF_A + EXPF_B * x.abs()) * U


def logf_err(x):
    return (LOGF_A * torch.log(x).abs() + LOGF_B) * U


def _ln_fwd_bound(r, Er, w, b, eps):
    D = r.shape[1]
    k = lambda t: t.mean(1, keepdim=True)
    mean = k(r)
    Em = (D + 1) * U * k(r.abs()) + k(Er)
    d = r - mean
    e = Em + Er + U * d.abs()
    var = k(d * d)
    Ev = k(2 * d.abs() * e + e * e) + (D + 2) * U * var + U * (var + eps)
    t = var + eps
    rs = t.rsqrt()
    lo = t - Ev
    Ers = torch.where(lo > 0, lo.clamp_min(1e-300).rsqrt() - rs, torch.full_like(rs, float("inf"))) + 6 * U * rs
    y = d * rs * w + b
    Ey = w.abs() * (e * rs + d.abs() * Ers + e * Ers) + 3 * U * (d * rs * w).abs() + U * y.abs()
    return dict(y=y, Ey=Ey, mean=mean[:, 0], Em=(Em + U * mean.abs())[:, 0], rstd=rs[:, 0], Ers=Ers[:, 0])


def _ln_bwd_bound(dy, Edy, x, w, mu, rs, dx0, M_sum, Emu=None, Ers=None, Ex=0.0):
    """ln_bwd64's outputs with their bounds; mu, rs [M] as the kernel holds them within Emu, Ers (None: operands, exact), x within Ex"""
    D = x.shape[1]
    k = lambda t: t.mean(1, keepdim=True)
    mu, rs = mu[:, None], rs[:, None]
    Emu = torch.zeros_like(mu) if Emu is None else Emu[:, None]
    Ers = torch.zeros_like(rs) if Ers is None else Ers[:, None]
    g = dy * w
    Eg = w.abs() * Edy + U * g.abs()
    xc = x - mu
    xh = xc * rs
    Exh = 2 * U * xh.abs() + (Emu + Ex) * rs + xc.abs() * Ers
    s1, s2 = k(g), k(g * xh)
    Es1 = k(Eg) + (D + 1) * U * k(g.abs())
    Es2 = k(Eg * xh.abs() + g.abs() * Exh + U * (g * xh).abs()) + (D + 1) * U * k((g * xh).abs())
    inner = g - s1 - xh * s2
    Ein = Eg + Es1 + xh.abs() * Es2 + s2.abs() * Exh + 3 * U * (g.abs() + s1.abs() + (xh * s2).abs())
    r = rs * inner
    Edx = rs * Ein + inner.abs() * Ers + U * r.abs()
    dx = r
    if dx0 is not None:
        dx = dx0 + r
        Edx = Edx + U * dx.abs()
    t = dy * xh
    Edw = (dy.abs() * Exh + Edy * xh.abs() + U * t.abs()).sum(0) + (M_sum + 1) * U * t.abs().sum(0)
    Edb = Edy.sum(0) + (M_sum + 1) * U * dy.abs().sum(0)
    return dict(dx=dx, Edx=Edx, dw=t.sum(0), Edw=Edw, db=dy.sum(0), Edb=Edb)


def _seq32(terms):
    """fp32 sum of the tensors in list order"""
    acc = terms[0].clone()
    for t in terms[1:]:
        acc = acc + t
    return acc


def _fwd_row(c, I):
    """the row a LayerNorm forward case normalises: (fp64 value, its bound, the fp32-sequential value the kernel must hold)"""
    terms = [I["x"]]
    if c.op == "ln_fwd_sum":
        terms += ([I["bias"].expand_as(I["x"])] if c.bias else []) + list(I["parts"])
    elif c.add:
        a = I["add"]
        terms.append(a if c.add == "full" else a[torch.arange(c.M) % a.shape[0]])
    r = sum(t.double() for t in terms)
    Er = torch.zeros_like(r) if len(terms) == 1 else len(terms) * U * sum(t.double().abs() for t in terms)
    return r, Er, _seq32(terms)


def _head_bound(c, I):
    feat, w, text, s = (I[k].double() for k in ("feat", "w", "text", "scale"))
    labels, sm = I["labels"], c.smooth
    B, F = feat.shape
    C, E = text.shape
    es = torch.exp(s)
    pc = feat @ w
    spc = es * pc
    Espc = es * (F + 2) * U * (feat.abs() @ w.abs()) + spc.abs() * (expf_err(s) + U)
    n = text.norm(dim=1)
    nerr = (E + 1) * U / 2 + 3 * U
    tn = text / n[:, None]
    L = spc @ tn.t()
    EL = (Espc @ text.abs().t() + (E + 1) * U * (spc.abs() @ text.abs().t())) / n + L.abs() * nerr
    # cross entropy
    mx = L.amax(1, keepdim=True)
    a = L - mx
    ex = torch.exp(a)
    se = ex.sum(1, keepdim=True)
    lse = mx + torch.log(se)
    ELmax = EL.amax(1, keepdim=True)
    se_rel = (ex * (expf_err(a) + U * a.abs() + U)).sum(1, keepdim=True) / se + (C + 1) * U + 2.0 ** -126 * C
    Else = se_rel + logf_err(se) + 2 * U * lse.abs() + U * mx.abs()
    onehot = torch.zeros_like(L).scatter_(1, labels[:, None], 1.0)
    Ly = (L * onehot).sum(1, keepdim=True)
    rowloss = (1.0 - sm) * (lse - Ly) + sm * (lse - L.mean(1, keepdim=True))
    Erow = 2 * ELmax + Else + U * (4 * lse.abs() + 4 * Ly.abs() + (C + 4) * L.abs().mean(1, keepdim=True))
    loss = rowloss.mean()
    Eloss = Erow.mean() + (B + 2) * U * rowloss.abs().mean()
    q = L - lse
    p = torch.exp(q)
    tgt = (1.0 - sm) * onehot + sm / C
    dl = (p - tgt) / B
    Edl = (p * (EL + ELmax) + p * (expf_err(q) + U * q.abs() + Else + U) + 2.0 ** -126 + 3 * U * (p + tgt)) / B
    dtn = dl.t() @ spc
    Edtn = Edl.t() @ spc.abs() + dl.abs().t() @ Espc + (B + 1) * U * (dl.abs().t() @ spc.abs())
    Etn = tn.abs() * nerr
    proj = (dtn * tn).sum(1, keepdim=True)
    Eproj = (Edtn * tn.abs() + dtn.abs() * Etn).sum(1, keepdim=True) + (E + 2) * U * (dtn * tn).abs().sum(1, keepdim=True)
    out = (dtn - tn * proj) / n[:, None]
    Eout = (Edtn + tn.abs() * Eproj + proj.abs() * Etn + 3 * U * (dtn.abs() + (tn * proj).abs())) / n[:, None] + out.abs() * nerr
    return dict(logits=_ref(L, EL), loss=_ref(loss, Eloss), d_text=_ref(out, Eout))


def reference(c):
    """{output: Ref} of case c (module docstring)"""
    I = inputs(c)
    d = lambda k: I[k].double()
    if c.op in ("ln_fwd", "ln_fwd_sum", "ln_chain"):
        r, Er, r32 = _fwd_row(c, I)
        f = _ln_fwd_bound(r, Er, d("w"), d("b"), c.eps)
        out = dict(y=_ref(f["y"], f["Ey"], c.y))
        if c.stats:
            out["mean"], out["rstd"] = _ref(f["mean"], f["Em"]), _ref(f["rstd"], f["Ers"])
        if c.xs or c.op == "ln_fwd_sum":
            out["xs"] = _ref(r, Er, bits_=r32)
        if c.op != "ln_chain":
            return out
        # the backward on the forward's own statistics: dx against the EXACT statistics, their error inside the bound
        b = _ln_bwd_bound(d("dy"), torch.zeros_like(r), r, d("w"), f["mean"], f["rstd"], None, c.M, f["Em"], f["Ers"], Er)
        out["dx"], out["copy"] = _ref(b["dx"], b["Edx"]), _ref(b["dx"], b["Edx"], c.copy)
        return out
    if c.op in ("ln_bwd", "ln_bwd_sum", "ln_bwd_w"):
        dy = d("dy")
        Edy = torch.zeros_like(dy)
        if c.S:
            Edy = (c.S * U * dy.abs().sum(0)) if c.S > 1 else Edy[0]
            dy = dy.sum(0)
        b = _ln_bwd_bound(dy, Edy, d("xs"), d("w"), d("mean"), d("rstd"), d("dx0") if c.acc else None, c.M)
        out = dict(dx=_ref(b["dx"], b["Edx"]))
        if c.copy:
            out["copy"] = _ref(b["dx"], b["Edx"], c.copy)
        if c.op == "ln_bwd_w":
            out["dw"], out["db"] = _ref(b["dw"], b["Edw"]), _ref(b["db"], b["Edb"])
        return out
    if c.op == "matmul":
        a, w = d("a"), d("w")
        return dict(out=_ref(c.alpha * (a @ w), c.alpha * (c.K + 2) * U * (a.abs() @ w.abs())))
    if c.op == "head":
        return _head_bound(c, I)
    if c.op == "rows":
        v = rows64(d("base"), I["slot"], d("tokens"), d("pos"))
        return dict(out=_ref(v, U * v.abs(), bits_=rows64(I["base"], I["slot"], I["tokens"], I["pos"])))
    if c.op == "rows_bwd":
        g, ro = d("g"), I["rows_of"]
        n = (ro >= 0).sum(1)[:, None]
        return dict(out=_ref(rows_bwd64(g, ro, c.sc), (n + 1) * U * rows_bwd64(g.abs(), ro, c.sc), bits_=_rows_bwd32(I["g"], ro, c.sc)))
    raise ValueError(c.op)


def _rows_bwd32(g, rows_of, scale, first8=False, per_row=False):
    """the documented order in fp32: a token's rows added in list order onto zero, then one multiply by scale"""
    out = torch.zeros(rows_of.shape[0], g.shape[1], dtype=torch.float32)
    sc = torch.tensor(scale, dtype=torch.float32)
    for t in range(rows_of.shape[0]):
        for k, r in enumerate(rows_of[t].tolist()):
            if r < 0 or (first8 and k >= 8):
                break
            out[t] = (out[t] + g[r]) * sc if per_row else out[t] + g[r]
    return out if per_row else out * sc


# ------------------------------------------------------------------------------------------------ the stand-in and its mutations
MUTATIONS = ("ln_bwd_no_xhat_term", "ln_bwd_mean_over_512", "ln_bwd_accumulate_ignored", "sum_from_z1", "sum_twice", "ln_fwd_add_row_not_wrapped",
             "drop_k_eighth", "drop_k_tail16", "sample7_reads_neighbour", "columns_past_64_unwritten", "logits_norm_squared",
             "ce_eps_over_c_minus_1", "ce_softmax_first_64", "dtext_no_projection", "dtext_norm_once_too_few", "loss_mean_over_16",
             "rows_bwd_first_batch_only", "rows_bwd_scale_per_row")


@functools.lru_cache(maxsize=None)
def _perm(n):
    return torch.randperm(n, generator=torch.Generator().manual_seed(n))


def _sum32(t, dim, keepdim=False):
    """fp32 sum along dim in another order: the entries permuted, then torch's blocked (pairwise) sum"""
    return t.index_select(dim, _perm(t.shape[dim])).sum(dim, keepdim=keepdim)


def _mm32(a, w, mutate=None):
    """a [M, K] @ w [K, N] in fp32, K permuted; the project8 mutations act on the eight K ranges of its waves"""
    K = a.shape[1]
    a = a.clone()
    if mutate == "drop_k_eighth":
        a[:, K - K // 8:] = 0
    if mutate == "drop_k_tail16":
        fq = K // 8
        for q in range(8):
            a[:, q * fq + fq - fq % 16:(q + 1) * fq] = 0
    if mutate == "sample7_reads_neighbour":
        a[7::8] = a[6::8][:a[7::8].shape[0]]
    p = _perm(K)
    out = a[:, p] @ w[p]
    if mutate == "columns_past_64_unwritten":
        bits(out)[:, 64 * (out.shape[1] // 64):] = SENTINEL[4]
    return out


def _ln_fwd32(r, w, b, eps):
    D = r.shape[1]
    mean = _sum32(r, 1, True) / D
    dd = r - mean
    rstd = 1.0 / torch.sqrt(_sum32(dd * dd, 1, True) / D + torch.tensor(eps, dtype=torch.float32))
    return dd * rstd * w + b, mean[:, 0], rstd[:, 0]


def _ln_bwd32(dy, x, w, mu, rs, dx0, mutate):
    D = 512 if mutate == "ln_bwd_mean_over_512" else x.shape[1]
    g = dy * w
    xh = (x - mu[:, None]) * rs[:, None]
    s1, s2 = _sum32(g, 1, True) / D, _sum32(g * xh, 1, True) / D
    r = rs[:, None] * (g - s1 - (0 if mutate == "ln_bwd_no_xhat_term" else xh * s2))
    dx = r if dx0 is None or mutate == "ln_bwd_accumulate_ignored" else dx0 + r
    return dx, _sum32(dy * xh, 0), _sum32(dy, 0)


def standin(c, mutate=None):
    """{output: tensor in its stored format}: case c computed correctly in fp32 in another order, or broken by `mutate`"""
    I = inputs(c)
    if c.op in ("ln_fwd", "ln_fwd_sum", "ln_chain"):
        terms = [I["x"]]
        if c.op == "ln_fwd_sum":
            parts = list(I["parts"])
            parts = parts[1:] if mutate == "sum_from_z1" else parts + parts if mutate == "sum_twice" else parts
            terms += ([I["bias"].expand_as(I["x"])] if c.bias else []) + parts
        elif c.add:
            a = I["add"]
            idx = torch.arange(c.M).clamp_max(a.shape[0] - 1) if mutate == "ln_fwd_add_row_not_wrapped" else torch.arange(c.M) % a.shape[0]
            terms.append(a if c.add == "full" else a[idx])
        r = _seq32(terms)                                   # (the documented order: the summed row is checked bit for bit)
        y, mean, rstd = _ln_fwd32(r, I["w"], I["b"], c.eps)
        out = dict(y=y.to(FMT[c.y]))
        if c.stats:
            out["mean"], out["rstd"] = mean, rstd
        if c.xs or c.op == "ln_fwd_sum":
            out["xs"] = r
        if c.op == "ln_chain":
            dx, _, _ = _ln_bwd32(I["dy"], r, I["w"], mean, rstd, None, mutate)
            out["dx"], out["copy"] = dx, dx.to(FMT[c.copy])
        return out
    if c.op in ("ln_bwd", "ln_bwd_sum", "ln_bwd_w"):
        dy = I["dy"]
        if c.S:
            parts = list(dy)
            parts = parts[1:] if mutate == "sum_from_z1" else parts + parts if mutate == "sum_twice" else parts
            dy = _sum32(torch.stack(parts), 0) if parts else torch.zeros_like(I["xs"])
        dx, dw, db = _ln_bwd32(dy, I["xs"], I["w"], I["mean"], I["rstd"], I["dx0"] if c.acc else None, mutate)
        out = dict(dx=dx)
        if mutate == "ln_bwd_accumulate_ignored" and c.acc:
            out["dx"] = I["dx0"].clone()                     # (the caller's dx is left as it was; the copy is of the new term alone)
        if c.copy:
            out["copy"] = dx.to(FMT[c.copy])
        if c.op == "ln_bwd_w":
            out["dw"], out["db"] = dw, db
        return out
    if c.op == "matmul":
        return dict(out=_mm32(I["a"], I["w"], mutate) * torch.tensor(c.alpha, dtype=torch.float32))
    if c.op == "head":
        return _head32(c, I, mutate)
    if c.op == "rows":
        return dict(out=rows64(I["base"], I["slot"], I["tokens"], I["pos"]))
    if c.op == "rows_bwd":
        return dict(out=_rows_bwd32(I["g"], I["rows_of"], c.sc, mutate == "rows_bwd_first_batch_only", mutate == "rows_bwd_scale_per_row"))
    raise ValueError(c.op)


def _head32(c, I, mutate):
    feat, w, text, labels, sm = I["feat"], I["w"], I["text"], I["labels"], torch.tensor(c.smooth, dtype=torch.float32)
    B, C = c.B, c.C
    pm = mutate if mutate in ("drop_k_eighth", "drop_k_tail16", "sample7_reads_neighbour", "columns_past_64_unwritten") and _project8(c, c.F) else None
    spc = torch.exp(I["scale"]) * _mm32(feat, w, pm)
    nn = _sum32(text * text, 1)
    n = torch.sqrt(nn)
    logits = _mm32(spc, text.t().contiguous()) / (nn if mutate == "logits_norm_squared" else n)
    lg = logits[:, :64] if mutate == "ce_softmax_first_64" else logits
    mx = lg.amax(1, keepdim=True)
    lse = mx + torch.log(_sum32(torch.exp(lg - mx), 1, True))
    onehot = torch.zeros_like(logits).scatter_(1, labels[:, None], 1.0)
    ly = _sum32(logits * onehot, 1, True)
    rowloss = (1 - sm) * (lse - ly) + sm * (lse - _sum32(logits, 1, True) / C)
    loss = _sum32(rowloss[:16], 0)[0] / 16 if mutate == "loss_mean_over_16" else _sum32(rowloss, 0)[0] / B
    base = sm / (C - 1) if mutate == "ce_eps_over_c_minus_1" and C > 1 else sm / C
    dl = (torch.exp(logits - lse) - (base + (1 - sm) * onehot)) / B
    dtn = _mm32(dl.t().contiguous(), spc)
    tn = text / n[:, None]
    proj = 0 if mutate == "dtext_no_projection" else _sum32(dtn * tn, 1, True)
    d_text = dtn - tn * proj
    if mutate != "dtext_norm_once_too_few":
        d_text = d_text / n[:, None]
    return dict(logits=logits, loss=loss, d_text=d_text)


# ------------------------------------------------------------------------------------------------ the criterion
def worst(x, ref, cap=1.0):
    """-> max |x - exact| / (cap E + R); NaN, or an error where the tolerance is 0, counts as inf"""
    err = (x.double() - ref.exact).abs()
    tl = cap * ref.E + ref.R
    r = torch.where(tl > 0, err / tl.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())


def describe(c, name=None):
    return f"{case_id(c)} [{family(c, name)}] ({c.note})"


def check(c, result, errors=None, cap=1.0, what="CHAIN-ENDS"):
    """result {output: tensor} against reference(c) -> {output: ratio}; appends what fails to `errors`; prints the ratios.  The
    outputs with a documented order must also hold its bits (compared as values: -0 and +0 are the same row)."""
    ref, res = reference(c), {}
    assert set(result) == set(ref), (sorted(result), sorted(ref))
    for name, x in result.items():
        x = x.cpu()
        assert tuple(x.shape) == tuple(ref[name].exact.shape), (name, x.shape, ref[name].exact.shape)
        # (an output pinned to a documented order has no other order to be the half of: its rounding may use all of E)
        res[name] = worst(x, ref[name], 1.0 if ref[name].bits is not None else cap)
        if errors is not None and not res[name] <= 1.0:
            errors.append(f"{describe(c, name)} {name}: |x - exact| / ({cap:g} E + R) = {res[name]:.3g} > 1")
        if errors is not None and ref[name].bits is not None and not torch.equal(x, ref[name].bits):
            errors.append(f"{describe(c, name)} {name}: not the bits of the documented fp32 order "
                          f"({int((x != ref[name].bits).sum())} elements differ)")
    print(f"{what} {case_id(c)} " + " ".join(f"{k}={v:.3f}" for k, v in res.items()))
    return res


# ------------------------------------------------------------------------------------------------ the cases
VEC8_D, SCALAR_D = (8, 64, 136, 384, 504, 512), (4, 7, 100, 520, 1000, 1024)
HEAD_SHAPES = [
    (32, 768, 512, 40, "", "project8: the production shape"), (1, 32, 64, 1, "", "project8: smallest sizes"),
    (9, 96, 100, 3, "", "project8: F / 8 = 12, the 4-step tail only; E % 64 != 0"),
    (17, 160, 72, 65, "", "project8: the 16-step loop then the 4-step tail; C > 64"),
    (5, 1536, 64, 15, "", "project8: the 64 KiB LDS edge"), (3, 100, 64, 7, "", "fallback: F % 32 != 0"),
    (2, 2048, 128, 10, "", "fallback: F > 1536"), (4, 768, 512, 40, "feat", "fallback: feat one float off alignment"),
    (33, 8192, 64, 5, "", "fallback: large F"), (4096, 32, 64, 2, "", "ce_bwd: B at its limit"),
]
MATMUL_SHAPES = [(1, 32, 1, 1.0), (8, 32, 64, 1.0), (9, 96, 65, 1.0), (15, 160, 100, 1.0), (40, 512, 512, 1.0), (40, 512, 512, 4096.0),
                 (256, 1536, 70, 1.0), (17, 1024, 512, 2.0 ** -12)]


def _cases():
    cs = []
    ys, Ms = ("f32", "bf16", "f16"), (1, 3, 4, 5)
    adds, xss = ("", "full", "rows1", "rows7"), ("", "out", "inplace")
    # LayerNorm forward: every D of both kernels in every output format; M, add, write_xs, save_stats, eps and the input
    # distribution go round their values with the running index
    k = 0
    for D in VEC8_D + SCALAR_D:
        for y in ys:
            cs.append(Case("ln_fwd", M=Ms[k % 4], D=D, y=y, add=adds[(k // 3 + k) % 4], xs=xss[(k // 2) % 3], stats=k % 3 != 1,
                           eps=1e-6 if k % 5 == 2 else 1e-5, hard=k % 2 == 1, note="D x format grid"))
            k += 1
    for D, y in ((512, "bf16"), (384, "f16"), (1000, "f32"), (1024, "bf16")):
        cs.append(Case("ln_fwd", M=817, D=D, y=y, add="rows7" if D == 512 else "full", xs="inplace", hard=True,
                       note="the prompt chain's 817 rows, outlier channels and row offsets"))
    for y, xs in (("f32", "out"), ("bf16", ""), ("f16", "inplace")):
        cs.append(Case("ln_fwd", M=8200, D=8, y=y, add="rows7", xs=xs, hard=True, note="M > 8192: the row += nw loop of ln_fwd_vec8_kernel"))
    for i, (D, mis) in enumerate((D, m) for D in (384, 512) for m in ("x", "add", "xs")):
        cs.append(Case("ln_fwd", M=Ms[i % 4] if i else 817, D=D, y=ys[i % 3], add="full", xs="out", mis=mis, hard=i % 2 == 0,
                       note=f"{mis} one float off alignment: ln_fwd_kernel at a vec8 width"))
    for i, (S, bias) in enumerate((S, b) for S in (1, 3, 8) for b in (False, True)):
        cs.append(Case("ln_fwd_sum", M=(5, 817, 3, 4, 1, 817)[i], D=(512, 384, 8, 136, 504, 512)[i], y=ys[i % 3], S=S, bias=bias, stats=i % 2 == 0,
                       eps=1e-6 if i == 3 else 1e-5, hard=i in (1, 5), note="split-K consumer: x + bias + parts in slice order"))
    # LayerNorm backward, dx only: the D / M / alignment grid with accumulate and the operand copy going round
    copies = ("", "f16", "bf16", "f32")
    k = 0
    for D in VEC8_D + SCALAR_D:
        for acc in (False, True):
            cs.append(Case("ln_bwd", M=Ms[k % 4], D=D, acc=acc, copy=copies[(k // 2 + k) % 4], hard=k % 3 == 0, note="D x accumulate grid"))
            k += 1
    for D, cp, acc in ((512, "bf16", True), (384, "f16", False), (1000, "bf16", True), (512, "", False), (512, "f32", True), (1000, "f16", False),
                       (100, "f32", True), (100, "", False), (1024, "", True), (8, "bf16", False)):
        cs.append(Case("ln_bwd", M=817, D=D, acc=acc, copy=cp, hard=True, note="the prompt chain's 817 rows: more than one workgroup"))
    cs.append(Case("ln_bwd", M=8200, D=8, acc=True, copy="f16", note="the largest launch of the file"))
    for i, (D, mis) in enumerate((D, m) for D in (384, 512) for m in ("dy", "xs", "dx")):
        cs.append(Case("ln_bwd", M=(817, 5, 3, 4, 1, 817)[i], D=D, acc=i % 2 == 0, copy=copies[i % 4], mis=mis, hard=True,
                       note=f"{mis} one float off alignment: the scalar waves = M path at a dx8 width"))
    for i, (S, acc) in enumerate((S, a) for S in (1, 4, 8) for a in (True, False)):
        cs.append(Case("ln_bwd_sum", M=(817, 5, 3, 817, 1, 4)[i], D=(512, 384, 8, 512, 504, 136)[i], S=S, acc=acc, copy=copies[(i + 1) % 4], hard=i % 2 == 0,
                       note="dy as S split-K slices"))
    cs.append(Case("ln_chain", M=817, D=512, y="bf16", add="rows7", xs="out", copy="bf16", hard=True,
                   note="forward then backward on the forward's own mean / rstd"))
    # with weight gradients
    for M in (1, 5, 300, 301):
        for D in (384, 1000):
            for p in (1, 64, 0):
                cs.append(Case("ln_bwd_w", M=M, D=D, prows=p, acc=(M + p) % 2 == 1, copy="bf16" if p == 64 else "", hard=M == 300,
                               note="(rows per wave, partial rows used, partial rows) = " + str(_lnw_geometry(Case(M=M, prows=p)))))
    for M, K, N, alpha in MATMUL_SHAPES:
        cs.append(Case("matmul", M=M, K=K, N=N, alpha=alpha, note="ppt_rows_matmul_f32"))
    for B, F, E, C, mis, note in HEAD_SHAPES:
        for sm in (0.0, 0.2):
            for sc in ("init", "max"):
                cs.append(Case("head", B=B, F=F, E=E, C=C, mis=mis, smooth=sm, scale=sc, note=note))
    cs.append(Case("head", B=32, F=768, E=512, C=40, labels="same", note="every label equal"))
    cs.append(Case("head", B=17, F=160, E=72, C=65, labels="same", smooth=0.0, scale="max", note="every label equal, C > 64"))
    for B, F, E, C, sm in ((17, 160, 72, 65, 0.2), (17, 160, 72, 65, 0.0), (40, 64, 64, 130, 0.2)):
        cs.append(Case("head", B=B, F=F, E=E, C=C, smooth=sm, close=True,
                       note="C > 64 with similar class prompts: the second and third pass of the lane loops carry weight in every row"))
    for i, mr in enumerate((1, 7, 8, 9, 40, 55)):
        for W in (4, 512, 516):
            cs.append(Case("rows_bwd", W=W, max_rows=mr, sc=2.0 ** -12 if (i + W // 4) % 2 else 1.0, note="synthetic layout: a full list, an unused token"))
        cs.append(Case("rows", W=(4, 512, 516)[i % 3], max_rows=mr, note="slots mixed with base rows"))
    return cs


CASES = _cases()
assert len({case_id(c) for c in CASES}) == len(CASES)
BY_ID = {case_id(c): c for c in CASES}

REQUIRED = (
    {f"ln_fwd:vec8:D{D}" for D in VEC8_D} | {f"ln_fwd:scalar:D{D}" for D in SCALAR_D}
    | {f"ln_fwd:{k}:{y}" for k in ("vec8", "scalar") for y in FMT} | {f"ln_fwd:scalar:D{D}:mis_{m}" for D in (384, 512) for m in ("x", "add", "xs")}
    | {f"ln_fwd:M{M}" for M in (1, 3, 4, 5, 817, 8200)} | {"ln_fwd:vec8:rowloop", "ln_fwd:add_full", "ln_fwd:add_rows1", "ln_fwd:add_rows7",
                                                           "ln_fwd:xs_out", "ln_fwd:xs_inplace", "ln_fwd:stats0", "ln_fwd:stats1", "ln_fwd:eps1e-05",
                                                           "ln_fwd:eps1e-06", "ln_fwd:vec8:hard", "ln_fwd:scalar:hard"}
    | {f"ln_fwd_sum:S{S}" for S in (1, 3, 8)} | {"ln_fwd_sum:bias0", "ln_fwd_sum:bias1"} | {f"ln_fwd_sum:{y}" for y in FMT}
    | {f"ln_bwd:dx8:D{D}" for D in VEC8_D} | {f"ln_bwd:scalar:D{D}" for D in SCALAR_D}
    | {f"ln_bwd:{k}:{o}" for k in ("dx8", "scalar") for o in ("acc0", "acc1", "copy_none", "copy_f16", "copy_bf16", "copy_f32")}
    | {f"ln_bwd:scalar:{w}" for w in ("D%8", "D>512", "mis_dy", "mis_xs", "mis_dx")} | {f"ln_bwd:M{M}" for M in (1, 3, 4, 5, 817, 8200)}
    | {f"ln_bwd_sum:S{S}" for S in (1, 4, 8)} | {"ln_bwd_sum:acc0", "ln_bwd_sum:acc1", "ln_chain"}
    | {f"ln_bwd:{k}:{o}" for k in ("w8", "scalar_w") for o in ("prows1", "prows64", "prows0", "rpw1", "rpw>1", "ragged", "memset_tail")}
    | {"matmul:project8:tail4_only", "matmul:project8:loop16+tail4", "matmul:project8:loop16_only", "matmul:project8:E%64",
       "matmul:project8:lds64k", "matmul:project8:B1", "matmul:project8:B9", "matmul:project8:B17", "matmul:alpha4096", "matmul:alpha0.000244141"}
    | {"head:project8:tail4_only", "head:project8:loop16+tail4", "head:project8:loop16_only", "head:project8:E%64", "head:project8:lds64k",
       "head:project8:B1", "head:project8:B9", "head:project8:B17", "head:fallback:F%32", "head:fallback:F>1536", "head:fallback:mis_feat",
       "ce:C>64", "ce:C>64:every_class_in_the_softmax", "ce:B4096", "ce:smooth0", "ce:smooth0.2", "ce:scale_init", "ce:scale_max", "ce:labels_same"}
    | {f"{op}:W{W}" for op in ("rows", "rows_bwd") for W in (4, 512, 516)} | {f"{op}:max_rows{m}" for op in ("rows", "rows_bwd") for m in (1, 7, 8, 9, 40, 55)}
    | {"rows_bwd:scale1", "rows_bwd:scale0.000244141", "rows_bwd:unused_token", "rows_bwd:full_list", "rows_bwd:max_rows%8"})
FAMILIES = {"ln_fwd_vec8_kernel", "ln_fwd_vec8_kernel<SUM>", "ln_fwd_kernel", "ln_bwd_dx8_kernel", "ln_bwd_kernel (dx only, waves = M)",
            "ln_bwd_w8_kernel", "ln_bwd_kernel", "head_project8_kernel (ppt_rows_matmul_f32)", "head_project8_kernel + head_logits_kernel",
            "head_project_kernel + head_logits_kernel", "head_ce_bwd_kernel", "prompt_rows_kernel", "prompt_rows_bwd_kernel"}


def _assert_coverage():
    have = set().union(*(branches(c) for c in CASES))
    assert REQUIRED <= have, sorted(REQUIRED - have)
    fams = {family(c, o) for c in CASES for o in (None, "loss")}
    assert FAMILIES <= fams, sorted(FAMILIES - fams)
    assert any(family(c).startswith("ln_bwd_dx8_kernel (S") for c in CASES)


_assert_coverage()

# the cases each mutation must fail on (at least two each; test_chain_ends_ref_cpu.py)
_ids = lambda pred: [case_id(c) for c in CASES if pred(c)]
MUTANT_CASES = {
    "ln_bwd_no_xhat_term": _ids(lambda c: c.op in ("ln_bwd", "ln_bwd_sum", "ln_chain") and c.M == 817),
    "ln_bwd_mean_over_512": _ids(lambda c: c.op == "ln_bwd" and c.M == 817 and c.D != 512),
    "ln_bwd_accumulate_ignored": _ids(lambda c: c.op in ("ln_bwd", "ln_bwd_sum") and c.acc and c.M == 817),
    "sum_from_z1": _ids(lambda c: c.op in ("ln_fwd_sum", "ln_bwd_sum") and c.S > 1),
    "sum_twice": _ids(lambda c: c.op in ("ln_fwd_sum", "ln_bwd_sum")),
    "ln_fwd_add_row_not_wrapped": _ids(lambda c: c.op == "ln_fwd" and c.add in ("rows1", "rows7") and c.M > 7),
    "drop_k_eighth": _ids(lambda c: c.op == "matmul" or (c.op == "head" and _project8(c, c.F) and c.smooth == 0.2 and c.scale == "init")),
    "drop_k_tail16": _ids(lambda c: (c.op == "matmul" and (c.K // 8) % 16) or (c.op == "head" and (c.F // 8) % 16 and _project8(c, c.F))),
    "sample7_reads_neighbour": _ids(lambda c: (c.op == "matmul" and c.M >= 8) or (c.op == "head" and c.B >= 8 and _project8(c, c.F) and c.labels == "rand")),
    "columns_past_64_unwritten": _ids(lambda c: (c.op == "matmul" and c.N % 64) or (c.op == "head" and c.E % 64 and _project8(c, c.F))),
    "logits_norm_squared": _ids(lambda c: c.op == "head" and c.B in (32, 9, 33)),
    "ce_eps_over_c_minus_1": _ids(lambda c: c.op == "head" and c.smooth > 0 and c.C > 1 and c.B in (32, 17, 3) and not c.close),
    "ce_softmax_first_64": _ids(lambda c: c.op == "head" and c.C > 64 and c.close),
    "dtext_no_projection": _ids(lambda c: c.op == "head" and c.C > 1 and c.B in (32, 9, 2)),
    "dtext_norm_once_too_few": _ids(lambda c: c.op == "head" and c.C > 1 and c.B in (32, 5, 4096)),
    "loss_mean_over_16": _ids(lambda c: c.op == "head" and c.B > 16 and c.F < 8192 and c.labels == "rand"),
    "rows_bwd_first_batch_only": _ids(lambda c: c.op == "rows_bwd" and c.max_rows > 8),
    "rows_bwd_scale_per_row": _ids(lambda c: c.op == "rows_bwd" and c.sc != 1.0 and c.max_rows > 1),
}
assert set(MUTANT_CASES) == set(MUTATIONS) and all(len(v) >= 2 for v in MUTANT_CASES.values()), {k: len(v) for k, v in MUTANT_CASES.items()}
