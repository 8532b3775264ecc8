"""GPU: ppt_gemm and ppt_gemm256 (csrc/gemm.hip, csrc/gemm256.hip) through ppt_amd.ops.gemm, every tile loop, epilogue tier and
dispatch edge, in bf16, fp16 and fp32, against the fp64 reference and the a-priori bound of tests/gemm_ref.py.

Every case checks every output elementwise -- |kernel - fp64| <= tol, nothing NaN, nothing left out --, that everything OUTSIDE
the output windows (padding columns, rows behind M, gaps between batch slices, the bytes in front of a misaligned view) still
holds the sentinel, and that a second call returns the same bits.  Operands are windows in NaN-filled buffers, so an unmasked
read poisons the result.  The shapes choose the kernel and the tier (gemm_ref.CASES says which edge each case is for;
gemm_ref.family names the kernel in a failure); no switch is set, split=False is passed so a leaked split16 mode cannot change a
case.  The measured figures are printed (pytest -s) as output=ratio@slice.row.column: profiles/gemm_tests.md holds them.
"""
import ctypes

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ppt_amd import ops as _ops
    assert (_ops.A_PLAIN, _ops.A_AFFINE_RELU, _ops.A_CONV1) == (R.A_PLAIN, R.A_AFFINE_RELU, R.A_CONV1)
    assert (_ops.ACT_NONE, _ops.ACT_RELU, _ops.ACT_GELU, _ops.ACT_QUICKGELU) == (R.ACT_NONE, R.ACT_RELU, R.ACT_GELU, R.ACT_QUICKGELU)
    return _ops


def _dev(x):
    return None if x is None else x.cuda()


class Launch:
    """one case's operands on the device; call() launches into FRESH sentinel-filled output buffers and returns them"""

    def __init__(self, c, fmt):
        self.c, self.I = c, R.inputs(c, fmt)
        I = self.I
        self.slots = {k: getattr(I, k) for k in ("A", "B", "bias", "group", "row_scale", "res", "res2", "dact") if getattr(I, k) is not None}
        self.bufs = {k: s.buf.cuda() for k, s in self.slots.items()}
        self.flat = {k: _dev(getattr(I, k)) for k in ("a_scale", "a_shift", "pts", "w1", "b1")}

    def v(self, name):
        return R.view(self.slots[name], self.bufs[name], z=0) if name in self.slots else None

    def call(self, ops, core="case"):
        c, I = self.c, self.I
        outs = self.last = {k: s.buf.cuda() for k, s in I.outs.items()}
        o = lambda k: R.view(I.outs[k], outs[k], z=0) if k in outs else None
        assert self.v("B").data_ptr() % 16 == 0 and (c.a_mode == R.A_CONV1 or self.v("A").data_ptr() % 16 == 0)
        if c.c != "none":
            assert o("C").data_ptr() % 16 == (c.c_off * outs["C"].element_size()) % 16
        if c.bias:
            assert self.v("bias").data_ptr() % 16 == (c.bias_off * 4) % 16
        if c.group_rows:
            assert self.v("group").data_ptr() % 16 == (c.group_off * 4) % 16
        ops.gemm(self.v("A"), self.v("B"), out=o("C"), want_out=c.c != "none", bias=self.v("bias"), act=c.act, dact_pre=self.v("dact"),
                 group_add=self.v("group"), group_rows=c.group_rows, row_scale=self.v("row_scale"), row_scale_rows=c.rs_rows,
                 residual=self.v("res"), residual2=self.v("res2"), out2=o("out2"), out2_pre=c.out2_pre,
                 col_stats=(o("col_sum"), o("col_sqsum")) if c.stats else None, pool_max=o("pool_max"), pool_min=o("pool_min"),
                 pool_rows=c.pool_rows, batch=c.batch, strideA=I.A.zs if I.A is not None else 0, strideB=I.B.zs if c.strideB else 0,
                 strideC=I.outs["C"].zs if c.c != "none" else 0, a_mode=c.a_mode, a_scale=self.flat["a_scale"], a_shift=self.flat["a_shift"],
                 pts=self.flat["pts"], w1=self.flat["w1"], b1=self.flat["b1"], core=(c.core or None) if core == "case" else core, split=False)
        torch.cuda.synchronize()
        return {k: b.cpu() for k, b in outs.items()}


def _windows(I, bufs):
    return {k: R.view(I.outs[k], b).clone() for k, b in bufs.items()}


@pytest.mark.parametrize("run", R.RUNS, ids=R.run_id)
def test_gemm_against_fp64(ops, run):
    c, fmt = run
    L = Launch(c, fmt)
    I = L.I
    tag = f"{R.case_id(c)} {fmt} [{R.family(c, fmt)}, {c.tier}] ({c.note})"
    if c.expect == "raise":
        # statistics / pools on a launch that only the scalar tier would take: it has no code for them -- refused, nothing written
        with pytest.raises(RuntimeError):
            L.call(ops)
        torch.cuda.synchronize()
        for k, b in L.last.items():
            assert R.untouched(I.outs[k], b), f"{tag} {k}: written by a refused launch"
        return
    first = L.call(ops)
    second = L.call(ops)
    errors = []
    for k, b in first.items():
        if not torch.equal(R.bits(b), R.bits(second[k])):
            errors.append(f"{tag} {k}: a second call returned other bits")
        if not R.outside_intact(I.outs[k], b):
            errors.append(f"{tag} {k}: written outside its [{I.outs[k].rows}, {I.outs[k].cols}] window (ld {I.outs[k].ld}, offset {I.outs[k].off})")
        if k != "C" and R.any_sentinel_inside(I.outs[k], b):
            errors.append(f"{tag} {k}: returned with the sentinel still in it")
    R.check(c, fmt, _windows(I, first), errors, what="GEMM-GPU")
    if c.core == "256":
        # the macro-tile core against the tile loops on the same launch: the same bits (both walk K in ascending 16-wide MFMA steps
        # into fp32 accumulators and share the epilogue arithmetic)
        from ppt_amd import _lib
        _lib.lib().ppt_set_gemm256(0)
        try:
            loops = L.call(ops, core=None)
        finally:
            _lib.lib().ppt_set_gemm256(-1)
        for k, b in first.items():
            if not torch.equal(R.bits(b), R.bits(loops[k])):
                d = (R.view(I.outs[k], b).double() - R.view(I.outs[k], loops[k]).double()).abs().max()
                errors.append(f"{tag} {k}: ppt_gemm256 and the tile loops differ (max |difference| {float(d):.3g})")
    assert not errors, "\n".join(errors)


# ------------------------------------------------------------------------------------------------ J. refusals
def _raw(ops, fields, entry="ppt_gemm"):
    from ppt_amd import _lib
    p = _lib.GemmParams()
    for k, v in fields.items():
        setattr(p, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    _lib.check(getattr(_lib.lib(), entry)(ctypes.byref(p), ops._stream()), entry)


def _sent(shape, dt):
    t = torch.empty(shape, dtype=dt, device="cuda")
    R.bits(t).fill_(R._sentinel(dt))
    return t


def _base(fmt, M=70, N=72, K=64, cdt=None):
    """a valid plain launch as raw ppt_gemm_params fields + its tensors; every output sentinel-filled"""
    dt = R.FMT[fmt]
    code = {"f32": 0, "bf16": 1, "f16": 2}
    cdt = cdt or dt
    t = dict(A=torch.randn(M, K + 8, device="cuda").to(dt), B=torch.randn(N, K + 8, device="cuda").to(dt), C=_sent((M, N), cdt),
             C2=_sent((M, N), cdt), cs=_sent(((M + 31) // 32, N), torch.float32), cq=_sent(((M + 31) // 32, N), torch.float32),
             pmax=_sent(((M + 15) // 16, N), cdt), pmin=_sent(((M + 15) // 16, N), cdt), f=torch.randn(max(M, N, K) * N, device="cuda"),
             pts=torch.randn(M, 3, device="cuda"))
    f = dict(A=t["A"], lda=K + 8, B=t["B"], ldb=K + 8, C=t["C"], ldc=N, M=M, N=N, K=K, dtype=code[fmt],
             c_dtype=code[{v: k for k, v in R.FMT.items()}[cdt]], batch=1)
    return f, t, code


def _refusals():
    """(id, format, function(base fields, tensors, codes) -> (fields, entry))"""
    r = []
    add = lambda name, fn, fmts=("bf16", "f16", "f32"), **kw: r.extend((f"{name}-{fmt}", fmt, fn, kw) for fmt in fmts)
    h = ("bf16", "f16")
    add("K-not-a-chunk", lambda f, t, c: (dict(f, K=f["K"] - 2), "ppt_gemm"))
    add("lda-not-a-chunk", lambda f, t, c: (dict(f, lda=f["lda"] - 2), "ppt_gemm"))
    add("ldb-not-a-chunk", lambda f, t, c: (dict(f, ldb=f["ldb"] - 2), "ppt_gemm"))
    add("A-misaligned", lambda f, t, c: (dict(f, A=t["A"].data_ptr() + 8), "ppt_gemm"))
    add("B-misaligned", lambda f, t, c: (dict(f, B=t["B"].data_ptr() + 8), "ppt_gemm"))
    add("dtype-unknown", lambda f, t, c: (dict(f, dtype=3), "ppt_gemm"), ("bf16",))
    other = lambda f, c: c["f16"] if f["dtype"] == c["bf16"] else c["bf16"]
    add("C-other-16-bit-format", lambda f, t, c: (dict(f, c_dtype=other(f, c)), "ppt_gemm"), h)
    add("out2-other-16-bit-format", lambda f, t, c: (dict(f, C2=t["C2"], ldc2=f["N"], c2_dtype=other(f, c)), "ppt_gemm"), h)
    add("pool-other-16-bit-format", lambda f, t, c: (dict(f, pool_max=t["pmax"], pool_rows=16, pool_dtype=other(f, c)), "ppt_gemm"), h)
    add("statistics-N-not-8", lambda f, t, c: (dict(f, N=f["N"] - 4, col_sum=t["cs"], col_sqsum=t["cq"]), "ppt_gemm"))
    add("pool-rows-48", lambda f, t, c: (dict(f, pool_max=t["pmax"], pool_rows=48, pool_dtype=f["c_dtype"]), "ppt_gemm"))
    add("pool-min-without-max", lambda f, t, c: (dict(f, pool_min=t["pmin"], pool_rows=16, pool_dtype=f["c_dtype"]), "ppt_gemm"))
    add("prologue-K-1032", lambda f, t, c: (dict(f, a_mode=R.A_AFFINE_RELU, a_scale=t["f"], a_shift=t["f"]), "ppt_gemm"), K=1032)
    add("conv1-without-w1", lambda f, t, c: (dict(f, a_mode=R.A_CONV1, pts=t["pts"], b1=t["f"]), "ppt_gemm"))
    add("affine-without-scale", lambda f, t, c: (dict(f, a_mode=R.A_AFFINE_RELU, a_shift=t["f"]), "ppt_gemm"))
    M_ = 16
    for what, fn in (("residual", lambda f, t: dict(residual=t["f"], ld_res=f["N"])), ("group", lambda f, t: dict(group_add=t["f"], group_rows=32)),
                     ("statistics", lambda f, t: dict(col_sum=t["cs"], col_sqsum=t["cq"])),
                     ("pool", lambda f, t: dict(pool_max=t["pmax"], pool_rows=16, pool_dtype=f["c_dtype"]))):
        add(f"batched-{what}", lambda f, t, c, fn=fn: (dict(f, M=M_, batch=2, strideA=M_ * f["lda"], strideC=M_ * f["N"], **fn(f, t)), "ppt_gemm"))
    add("group-rows-0", lambda f, t, c: (dict(f, group_add=t["f"], group_rows=0), "ppt_gemm"))
    add("row-scale-rows-0", lambda f, t, c: (dict(f, row_scale=t["f"], row_scale_rows=0), "ppt_gemm"))
    add("core256-pool", lambda f, t, c: (dict(f, pool_max=t["pmax"], pool_rows=16, pool_dtype=f["c_dtype"]), "ppt_gemm256"), h)
    add("core256-K-32", lambda f, t, c: (f, "ppt_gemm256"), h, K=32)
    add("core256-K-72", lambda f, t, c: (f, "ppt_gemm256"), h, K=72)
    add("core256-statistics-with-bias", lambda f, t, c: (dict(f, bias=t["f"], col_sum=t["cs"], col_sqsum=t["cq"]), "ppt_gemm256"), h, N=256)
    add("core256-statistics-narrow-tile", lambda f, t, c: (dict(f, group_add=t["f"], group_rows=32, col_sum=t["cs"], col_sqsum=t["cq"]),
                                                           "ppt_gemm256"), h, N=128)
    add("core256-fp32-operands", lambda f, t, c: (f, "ppt_gemm256"), ("f32",))
    return r


REFUSALS = _refusals()


@pytest.mark.parametrize("name,fmt,fn,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_gemm_refuses(ops, name, fmt, fn, kw):
    f, t, code = _base(fmt, **kw)
    _raw(ops, f)                                             # the base launch is valid: what is refused below is the one change
    torch.cuda.synchronize()
    R.bits(t["C"]).fill_(R._sentinel(t["C"].dtype))
    fields, entry = fn(f, t, code)
    with pytest.raises(RuntimeError):
        _raw(ops, fields, entry)
    torch.cuda.synchronize()
    for k in ("C", "C2", "cs", "cq", "pmax", "pmin"):
        assert bool((R.bits(t[k].cpu()) == R._sentinel(t[k].dtype)).all()), f"{name}: {k} was written by a refused launch"


# ------------------------------------------------------------------------------------------------ the callers of statistics launches
def test_aligned16_copies_only_what_is_misaligned(ops):
    flat = torch.randn(64, device="cuda")
    assert ops.aligned16(None) is None and ops.aligned16(flat) is flat and ops.aligned16(flat[4:36]).data_ptr() == flat[4:36].data_ptr()
    v = flat[1:33]
    a = ops.aligned16(v)
    assert v.data_ptr() % 16 == 4 and a.data_ptr() % 16 == 0 and torch.equal(a, v)


@pytest.mark.parametrize("prec", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
def test_conv_bn_relu_takes_a_bias_view_of_a_flat_buffer(ops, prec):
    """autograd._conv_bn_relu_fwd hands a state-dict bias to a statistics launch with an fp32 C: as a view at element 1 of a flat
    parameter buffer it made the launch scalar, which left the (uninitialised) statistics as they were; now the caller passes an
    aligned copy -- the same bits as with a bias that was aligned to begin with"""
    from ppt_amd import autograd as AG
    M, K, N = 96, 16, 40
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(M, K, generator=gen).cuda().to(prec)
    w = (torch.randn(N, K, generator=gen) / 4).cuda()
    flat = torch.randn(N + 1, generator=gen).cuda()
    res = []
    for b in (flat[1:].clone(), flat[1:]):
        bn = torch.nn.BatchNorm1d(N).cuda()
        h, saved = AG._conv_bn_relu_fwd(x, w, b, bn, True, prec, prec)
        torch.cuda.synchronize()
        res.append((h, saved[2], bn.running_mean.clone(), bn.running_var.clone()))
    assert res[0][0].data_ptr() != res[1][0].data_ptr() and flat[1:].data_ptr() % 16 == 4
    for a, b in zip(*res):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    y = x.double() @ w.to(prec).double().T + flat[1:].double()
    ref = torch.relu((y - y.mean(0)) / torch.sqrt(y.var(0, unbiased=False) + 1e-5))
    # (guards against both runs being wrong alike: twice the 16-bit store's half ulp at the largest value, 1e-4 of it in fp32)
    assert (res[1][0].double() - ref).abs().max() <= (2.0 ** -7 if prec != torch.float32 else 1e-4) * max(1.0, float(ref.abs().max()))
