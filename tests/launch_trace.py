"""Launch traces of ppt_amd.engine functions, recorded without a GPU (helper module, not collected as a test).

A Recorder stands in for ppt_amd.ops while an engine function runs: every launch wrapper the function reaches is replaced by a fake
that allocates CPU tensors of the wrapper's result shape, dtype and aliasing and writes ONE LINE per call --

    op(name=argument, ...) -> result

The arguments are bound to the signature of the real wrapper and written by parameter name in the signature's order, without those
that are at their default (and gemm's out2_pre without an out2, which ops.gemm does not read): a call says the same whether an
argument went by position or by keyword, or whether a default was spelled out.  A call the real wrapper would not accept raises.
A tensor is written as a label numbered by the first appearance of its storage, its storage offset if not zero, its shape, its
strides if not contiguous, and its dtype: `t7[24,512]f32`, `t7+1024[22,512]f32`.  The same buffer keeps its label wherever it
comes back, so in-place against fresh and view against copy show in the text.  ATen calls between the launches (torch.empty,
index_select, cat ...) run for real on the CPU and are not recorded.  A wrapper without a fake raises.

trace_vit_block(case) / trace_text_tower(case) build zero-filled parameters of the real shapes and names, a fresh WeightCache, set
the engine's switches as module attributes (every switch to its documented default, then the case's), run the function and restore
everything.  tests/golden/make_golden_traces.py records the traces of a grid of cases; tests/test_launch_trace_cpu.py holds the
engine to them.
"""
import contextlib
import inspect

import torch

from ppt_amd import engine
from ppt_amd import ops as real_ops

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
_NAMES = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16", torch.uint8: "u8", torch.int64: "i64",
          torch.int32: "i32"}
HALF = real_ops.HALF
F32 = torch.float32

# the documented defaults -- set explicitly, so that a trace does not depend on the environment
DEFAULTS = dict(FUSED_MLP=True, FUSED_PROJ=True, ROWGEMM_MIN_ROWS=16000, LNLIN_MAX_ROWS=24576,
                BLOCK_PATH={"qkv": "auto", "proj": "fused", "mlp": "fused"},
                TEXT_FUSE_LN=False, TEXT_SPLITK=True, TEXT_MLP_PAIR=True, TEXT_MLP_PAIR_LN=True, TEXT_MLP_PAIR_LAST=True,
                TEXT_MLP_PAIR_SPLIT=True, TEXT_LIN_SPLIT=True)
SPLIT16_POW2 = (0, 4)


def _empty(shape, dtype):
    return torch.empty(tuple(shape), dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fakes: result shape, dtype and aliasing of the wrappers in ppt_amd/ops.py
# ---------------------------------------------------------------------------------------------------------------------------------
def _stats(M, on):
    return (_empty((M,), F32), _empty((M,), F32)) if on else (None, None)


def layernorm_fwd(x, w, b, y_dtype, add=None, add_rows=0, write_xs=None, save_stats=False, eps=1e-5):
    assert x.dtype == F32
    return (_empty(x.shape, y_dtype),) + _stats(x.numel() // x.shape[-1], save_stats)


def layernorm_fwd_sum(x, bias, parts, w, b, y_dtype, write_xs, save_stats=False, eps=1e-5):
    assert x.dtype == F32 and parts.dtype == F32 and write_xs.dtype == F32 and parts.numel() == parts.shape[0] * x.numel()
    return (_empty(x.shape, y_dtype),) + _stats(x.numel() // x.shape[-1], save_stats)


def layernorm_bwd(dy, xs, w, mean, rstd, dx=None, accumulate=False, want_wgrad=False, partial_rows=None, copy_dtype=None):
    assert dy.dtype == F32 and xs.dtype == F32
    dx = torch.empty_like(xs) if dx is None else dx
    D = xs.shape[-1]
    dw, db = (_empty((D,), F32), _empty((D,), F32)) if want_wgrad else (None, None)
    return (dx, dw, db, _empty(xs.shape, copy_dtype)) if copy_dtype is not None else (dx, dw, db)


def layernorm_bwd_sum(dy_parts, xs, w, mean, rstd, dx, accumulate=True, copy_dtype=None):
    assert dy_parts.dtype == F32 and xs.dtype == F32 and dy_parts.numel() == dy_parts.shape[0] * xs.numel()
    return dx, (_empty(xs.shape, copy_dtype) if copy_dtype is not None else None)


def gemm(A, B, *, out=None, out_dtype=None, M=None, want_out=True, **kw):
    assert A.shape[1] == B.shape[1] and A.dtype == B.dtype and A.stride(1) == 1 and B.stride(1) == 1
    if out is None and want_out:
        out = _empty((A.shape[0] if M is None else M, B.shape[0]), out_dtype or B.dtype)
    return out


def gemm_splitk(A, B, S):
    assert A.shape[1] == B.shape[1] and A.dtype == B.dtype and (A.shape[1] // S) * S == A.shape[1] and (A.shape[1] // S) % 64 == 0
    return _empty((S, A.shape[0], B.shape[0]), F32)


def rowgemm(A, W, *, ln=None, out=None, residual=None, **kw):
    assert W.shape[1] == A.shape[1] and W.dtype in HALF and W.is_contiguous() and A.is_contiguous()
    assert A.dtype == (F32 if ln is not None else W.dtype)
    if out is None:
        out = _empty((A.shape[0], W.shape[0]), F32 if residual is not None else W.dtype)
    assert out.dtype == (F32 if residual is not None else W.dtype) and out.is_contiguous()
    return out


def rows_matmul(a, w_kn, alpha=1.0):
    K = a.shape[1]
    if K > 1536 or K % 32 or w_kn.shape[0] != K:
        return None
    return _empty((a.shape[0], w_kn.shape[1]), F32)


def lnlin_retile(w):
    assert w.dtype in HALF and w.shape[1] == 384 and w.shape[0] % 384 == 0
    return torch.empty_like(w)


def lnlin(x, wt, ln, *, bias=None, ln_eps=1e-5, out=None):
    assert x.dtype == F32 and x.shape[1] == 384 and wt.dtype in HALF
    return _empty((x.shape[0], wt.shape[0]), wt.dtype) if out is None else out


def vit_mlp_retile(w1, w2, variant=None):
    assert w1.dtype in HALF and w2.dtype == w1.dtype and tuple(w1.shape) == (1536, 384) and tuple(w2.shape) == (384, 1536)
    return torch.empty_like(w1), torch.empty_like(w2)


def vit_proj_retile(wp):
    assert wp.dtype in HALF and tuple(wp.shape) == (384, 384)
    return torch.empty_like(wp)


def vit_mlp(x, w1, b1, w2, b2, ln, *, out=None, proj=None, **kw):
    assert x.dtype == F32 and x.is_contiguous() and x.shape[1] == 384 and w1.dtype in HALF and w2.dtype == w1.dtype
    if proj is not None:
        assert proj[0].dtype == w1.dtype and proj[1].dtype == w1.dtype and proj[0].shape == x.shape and proj[0].is_contiguous()
    return x if out is None else out


def _attention_fwd(qkv, n_seq, T, P, H, want_lse):
    rows = real_ops.prefix_rows(n_seq, T, P)
    assert qkv.shape[0] == rows and qkv.shape[1] == 3 * H * 64
    return _empty((rows, H * 64), qkv.dtype), (_empty((rows, H) if P else (n_seq, H, T), F32) if want_lse else None)


def attention_fwd(qkv, Bt, T, H, scale, causal, want_lse=True):
    return _attention_fwd(qkv, Bt, T, 0, H, want_lse)


def attention_prefix_fwd(qkv, C, T, P, H, scale, want_lse=True):
    return _attention_fwd(qkv, C, T, P, H, want_lse)


def attention_bwd(qkv, out, dout, lse, Bt, T, H, scale, causal):
    assert out.dtype == qkv.dtype and dout.dtype == qkv.dtype and lse is not None
    return torch.empty_like(qkv)


def attention_prefix_bwd(qkv, out, dout, lse, C, T, P, H, scale):
    assert out.dtype == qkv.dtype and dout.dtype == qkv.dtype and lse is not None
    return torch.empty_like(qkv)


def text_lin_retile16(w):
    assert w.dtype in HALF and w.dim() == 2
    wt = _empty((w.shape[0] * w.shape[1] * 2,), torch.uint8)
    wt.ppt_shape, wt.ppt_dtype = tuple(w.shape), w.dtype
    return wt


def text_lin_retile_split(w, b_pow2=None):
    assert w.dtype == F32 and w.dim() == 2
    wt = _empty((w.shape[0] * w.shape[1] * 4,), torch.uint8)
    wt.ppt_shape, wt.ppt_dtype = tuple(w.shape), F32
    return wt


def _text_lin(a, wt, bias, residual, out, out_dtype):
    N, K = wt.ppt_shape
    assert a.dtype == wt.ppt_dtype and a.dim() == 2 and a.shape[1] == K
    if K > 512:
        assert bias is None and residual is None and out is None and out_dtype in (None, F32)
        return _empty((K // 512, a.shape[0], N), F32)
    return _empty((a.shape[0], N), out_dtype or a.dtype) if out is None else out


def text_lin16(a, wt, *, bias=None, residual=None, out=None, out_dtype=None):
    return _text_lin(a, wt, bias, residual, out, out_dtype)


def text_lin_split(a, wt, *, bias=None, residual=None, out=None, a_pow2=None):
    return _text_lin(a, wt, bias, residual, out, None)


def text_mlp_retile(w1, w2, b_pow2=None):
    assert w2.dtype == w1.dtype and tuple(w1.shape) == (2048, 512) and tuple(w2.shape) == (512, 2048)
    if w1.dtype != F32:
        return torch.empty_like(w1), torch.empty_like(w2)
    return _empty((2048 * 512 * 4,), torch.uint8), _empty((2048 * 512 * 4,), torch.uint8)


def text_mlp_pair(a, w1t, w2t, *, bias=None, pre=None, backward=False, a_pow2=None, ln=None, ln_eps=1e-5, save_stats=False):
    t = F32 if w1t.dtype == torch.uint8 else w1t.dtype
    M = a.shape[0]
    assert a.shape[1] == 512 and a.dtype == (F32 if ln is not None else t) and not (ln is not None and backward)
    assert pre is None or (pre.dtype == t and tuple(pre.shape) == (M, 2048))
    parts = _empty((8, M, 512), F32)
    return (parts,) + _stats(M, save_stats) if ln is not None else parts


def convert(src, dst_dtype, scale=1.0):
    return src if (src.dtype == dst_dtype and scale == 1.0) else _empty(src.shape, dst_dtype)


def transpose(src, dst_dtype=None, pad_to=1):
    R, C = src.shape
    return _empty((C, (R + pad_to - 1) // pad_to * pad_to), dst_dtype or src.dtype)


FAKES = {f.__name__: f for f in (
    layernorm_fwd, layernorm_fwd_sum, layernorm_bwd, layernorm_bwd_sum, gemm, gemm_splitk, rowgemm, rows_matmul, lnlin, lnlin_retile,
    vit_mlp, vit_mlp_retile, vit_proj_retile, attention_fwd, attention_bwd, attention_prefix_fwd, attention_prefix_bwd,
    text_lin16, text_lin_split, text_lin_retile16, text_lin_retile_split, text_mlp_pair, text_mlp_retile, convert, transpose)}
# arguments the wrapper reads only when another one is given: {op: {argument: the one it rides on}}
RIDES_ON = {"gemm": {"out2_pre": "out2"}}
# constants and pure helpers of the real module
PASS = ("HALF", "ROWGEMM_K", "VIT_MLP_VARIANT", "prefix_rows", "ACT_NONE", "ACT_GELU", "ACT_QUICKGELU", "A_AFFINE_RELU", "A_CONV1")


def _is_default(v, default):
    return v is default or (not isinstance(v, torch.Tensor) and type(v) is type(default) and v == default)


class Recorder:
    """Stands in for ppt_amd.ops (see the module docstring).  `lines` is the trace so far."""

    SPLIT16_POW2 = SPLIT16_POW2

    def __init__(self, split16=False):
        self._split16 = bool(split16)
        self._labels = {}
        self._alive = []            # every tensor seen: a freed buffer's storage could come back under another label
        self.lines = []

    def split16_enabled(self):
        return self._split16

    def __getattr__(self, name):
        if name in PASS:
            return getattr(real_ops, name)
        fake = FAKES.get(name)
        if fake is None:
            raise AssertionError(f"ppt_amd.engine reached ops.{name}, which tests/launch_trace.py has no fake for")

        sig = inspect.signature(getattr(real_ops, name))

        def call(*args, **kw):
            given = sig.bind(*args, **kw).arguments
            rides = RIDES_ON.get(name, {})
            text = ", ".join(f"{k}={self.render(v)}" for k, v in given.items()
                             if not _is_default(v, sig.parameters[k].default) and not (k in rides and given.get(rides[k]) is None))
            out = fake(*args, **kw)
            self.lines.append(f"{name}({text}) -> {self.render(out)}")
            return out
        return call

    def render(self, v):
        if isinstance(v, torch.Tensor):
            self._alive.append(v)
            key = v.untyped_storage()._cdata
            label = self._labels.setdefault(key, f"t{len(self._labels)}")
            off = f"+{v.storage_offset()}" if v.storage_offset() else ""
            strides = "" if v.is_contiguous() else "{" + ",".join(str(s) for s in v.stride()) + "}"
            return f"{label}{off}[{','.join(str(s) for s in v.shape)}]{strides}{_NAMES.get(v.dtype, str(v.dtype))}"
        if isinstance(v, (tuple, list)):
            return "(" + ", ".join(self.render(e) for e in v) + ")"
        if isinstance(v, dict):
            return "{" + ", ".join(f"{k}={self.render(v[k])}" for k in sorted(v)) + "}"
        if isinstance(v, torch.dtype):
            return _NAMES.get(v, str(v))
        if isinstance(v, engine.WeightCache):
            return f"WeightCache({_NAMES[v.dtype]})"
        if v is None or isinstance(v, (bool, int, float, str)):
            return repr(v)
        raise AssertionError(f"launch trace: no rendering for {type(v).__name__}")

    def text(self):
        return "\n".join(self.lines) + "\n"


@contextlib.contextmanager
def recording(case):
    """engine.ops replaced by a Recorder, the switches and STAGE_DTYPE set as the case says; everything restored afterwards."""
    rec = Recorder(case.get("split16", False))
    switches = dict(DEFAULTS, **case.get("switches", {}))
    switches["BLOCK_PATH"] = dict(switches["BLOCK_PATH"])
    old = {k: getattr(engine, k) for k in switches}
    old.update(ops=engine.ops, STAGE_DTYPE=engine.STAGE_DTYPE, _F32_CACHES=engine._F32_CACHES)
    try:
        for k, v in switches.items():
            setattr(engine, k, v)
        engine.ops = rec
        engine.STAGE_DTYPE = {k: DTYPES[v] for k, v in case.get("stage", {}).items()}
        engine._F32_CACHES = {}
        yield rec
    finally:
        for k, v in old.items():
            setattr(engine, k, v)


def _zeros(*shape, dtype=F32):
    return torch.zeros(shape, dtype=dtype)


def trace_vit_block(case):
    """case: B, dtype, save, pos_in_x, add_pos_out, dp, fc1 (+ switches) -> the trace text of one vit_block_forward call
    (D = 384, 6 heads, Tn = 129, qkv 1152 wide)."""
    D, heads, Tn, B, hid = 384, 6, 129, case["B"], case["fc1"]
    p = "blocks.blocks.3."
    shapes = {"norm1.weight": (D,), "norm1.bias": (D,), "attn.qkv.weight": (3 * D, D), "attn.proj.weight": (D, D),
              "attn.proj.bias": (D,), "norm2.weight": (D,), "norm2.bias": (D,), "mlp.fc1.weight": (hid, D), "mlp.fc1.bias": (hid,),
              "mlp.fc2.weight": (D, hid), "mlp.fc2.bias": (D,)}
    sd = {p + k: _zeros(*s) for k, s in shapes.items()}
    x, pos = _zeros(B * Tn, D), _zeros(B * Tn, D)
    dp1, dp2 = (_zeros(B), _zeros(B)) if case["dp"] else (None, None)
    save = {} if case["save"] else None
    with recording(case) as rec:
        rec.render(x), rec.render(pos)                     # (the inputs are t0 and t1 in every trace)
        out = engine.vit_block_forward(sd, p, engine.WeightCache(DTYPES[case["dtype"]]), x, pos, B, Tn, heads, dp1, dp2, save=save,
                                       pos_in_x=case["pos_in_x"], add_pos_out=case["add_pos_out"])
        rec.lines.append("return " + rec.render(out))
        if save is not None:
            rec.lines.append("save " + rec.render(save))
        return rec.text()


def trace_text_tower(case):
    """case: dtype, split16, C, Lfull, eff_len, prefix, rows_in, layers, save, c_fc, grad_scale (+ stage, switches) -> the trace
    text of text_tower_forward and, where the case saves, of text_tower_backward on what it saved (Wd = 512, 8 heads)."""
    Wd, heads, C, Lfull, layers, hid = 512, 8, case["C"], case["Lfull"], case["layers"], case["c_fc"]
    sd = {"positional_embedding": _zeros(Lfull, Wd), "ln_final.weight": _zeros(Wd), "ln_final.bias": _zeros(Wd),
          "text_projection": _zeros(Wd, Wd)}
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        shapes = {"ln_1.weight": (Wd,), "ln_1.bias": (Wd,), "attn.in_proj_weight": (3 * Wd, Wd), "attn.in_proj_bias": (3 * Wd,),
                  "attn.out_proj.weight": (Wd, Wd), "attn.out_proj.bias": (Wd,), "ln_2.weight": (Wd,), "ln_2.bias": (Wd,),
                  "mlp.c_fc.weight": (hid, Wd), "mlp.c_fc.bias": (hid,), "mlp.c_proj.weight": (Wd, hid), "mlp.c_proj.bias": (Wd,)}
        sd.update({p + k: _zeros(*s) for k, s in shapes.items()})
    L = Lfull if case["eff_len"] is None else min(Lfull, case["eff_len"])
    P = case["prefix"]
    eot = (L - 1 - torch.arange(C) % (L - P)).to(torch.int64)                # every EOT at or behind the shared prefix
    prompts = rows_in = None
    if case["rows_in"]:
        P_eff = P if (0 < P < L and C > 1) else 0
        rows_in = (_zeros(real_ops.prefix_rows(C, L, P_eff) if P_eff else C * L, Wd), C, Lfull)
    else:
        prompts = _zeros(C, Lfull, Wd)
    with recording(case) as rec:
        rec.render(rows_in[0] if case["rows_in"] else prompts)
        wc = engine.WeightCache(DTYPES[case["dtype"]])
        out, saved = engine.text_tower_forward(sd, wc, prompts, eot, heads, layers, case["save"], eff_len=case["eff_len"], prefix=P,
                                               rows_in=rows_in)
        rec.lines.append("return " + rec.render(out))
        if case["save"]:
            # (the keys alone: the backward below shows which buffer it takes for each of them)
            rec.lines.append("saved " + " ".join(sorted(saved)) + " | layer: " + " ".join(sorted(saved["layers"][-1])))
            rec.lines.append("== backward")
            dout = _zeros(C, Wd)
            rec.render(dout)
            g = engine.text_tower_backward(sd, wc, saved, dout, grad_scale=case["grad_scale"])
            rec.lines.append("return " + rec.render(g))
        return rec.text()


TRACERS = {"vit_block": trace_vit_block, "text_tower": trace_text_tower}


# ---------------------------------------------------------------------------------------------------------------------------------
# which kernel ran: a trace reduced to its op names (weight conversions and re-tilings dropped), for the coverage check of the grid
# ---------------------------------------------------------------------------------------------------------------------------------
def signature(text):
    tags = []
    for line in text.splitlines():
        name = line.split("(", 1)[0]
        if "(" not in line or " -> " not in line:
            if line == "== backward":
                tags.append("|")
            continue
        if name in ("convert", "transpose") or name.endswith("_retile") or "_retile" in name:
            continue
        if name == "gemm_splitk":
            name += line.split(" -> ")[0].rsplit("S=", 1)[1].rstrip(")")
        for mark, tag in (("ln=(", ":ln"), ("proj=(", ":proj"), ("out2=t", ":out2"), ("backward=True", ":bwd")):
            if mark in line:
                name += tag
        tags.append(name)
    return " ".join(tags) + " "
