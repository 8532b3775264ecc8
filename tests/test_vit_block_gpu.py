"""GPU: the three launches of a frozen PointBERT block -- ppt_lnlin (csrc/lnlin.hip), ppt_rowgemm_bf16 (csrc/rowgemm.hip) and
ppt_vit_mlp_bf16 / ppt_vit_mlp3_bf16 (csrc/mlp_fused.hip, csrc/mlp_fused3.hip) -- through ppt_amd.ops, against the fp64 reference and
the two-tier criterion of tests/vit_block_ref.py (tests/test_vit_block_ref_cpu.py pins that criterion without a GPU).

Every (case, format): the hard bound on every element, the sharp bound per row within floor(M / 20) exceptions, nothing NaN, nothing
outside the output windows touched (operands are windows in NaN-filled buffers, outputs windows in sentinel-filled ones), a second
call bit-identical, in place equal to out of place bit for bit.  As exact equalities besides: a result does not depend on
workgroups= / walkers= / persistent_occupancy, and rows computed alone equal the same rows inside the batch.  Then the refusals of
the three host functions.  Chunk geometries are reached through workgroups= (vit_block_ref.geometry restates the host's
arithmetic; the device's CU count goes into it where the case leaves the grid to the host).  Figures are printed (pytest -s):
profiles/vit_block_tests.md holds them.
"""
import contextlib
import ctypes
import time

import pytest
import torch

import vit_block_ref as V

pytestmark = pytest.mark.gpu
_TIMES = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ppt_amd import ops as _ops
    assert (_ops.ACT_NONE, _ops.ACT_GELU, _ops.ACT_QUICKGELU) == (V.ACT_NONE, V.ACT_GELU, V.ACT_QUICKGELU)
    yield _ops
    if _TIMES:
        slow = max(_TIMES, key=_TIMES.get)
        print(f"\nVIT-GPU-TIME total {sum(_TIMES.values()):.1f} s over {len(_TIMES)} tests; slowest {slow}: {_TIMES[slow]:.2f} s")


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    _TIMES[request.node.name] = time.perf_counter() - t0


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


_SLOTS = ("x", "A", "bias", "gam", "bet", "rs", "res", "res2", "b1", "b2", "pa", "pb", "prs")


class Launch:
    """one case's operands on the device as windows of their NaN-filled buffers; call() launches into FRESH output buffers (the
    sentinel-filled ones, or for an in-place case a fresh copy of the NaN-padded operand) and returns them on the CPU"""

    def __init__(self, ops, c, fmt):
        self.ops, self.c, self.I = ops, c, V.inputs(c, fmt)
        I = self.I
        self.slots = {k: getattr(I, k) for k in _SLOTS if getattr(I, k) is not None}
        self.bufs = {k: s.buf.cuda() for k, s in self.slots.items()}
        self.t = {k: (V.mat if k in ("x", "A", "res", "res2", "pa") else V.vec)(s, self.bufs[k]) for k, s in self.slots.items()}
        if c.kernel == "mlp":
            self.t["W1t"], self.t["W2t"] = ops.vit_mlp_retile(I.W1.cuda(), I.W2.cuda(), variant=c.variant)
            if c.proj:
                self.t["Wpt"] = ops.vit_proj_retile(I.Wp.cuda())
        elif c.kernel == "lnlin":
            self.t["Wt"] = ops.lnlin_retile(I.W.cuda())
        else:
            self.t["W"] = I.W.cuda()
        for k, v in self.t.items():
            assert v.data_ptr() % 16 == 0 and v.is_contiguous(), k
        self.inplace_slot = self.slots["x" if c.kernel == "mlp" else "res"] if c.inplace else None

    def call(self, inplace=None, **kw):
        """-> ({output: its whole buffer on the CPU}, {output: slot}); inplace=False runs an in-place case out of place"""
        c, I = self.c, self.I
        inplace = c.inplace if inplace is None else inplace
        slots = dict(I.outs)
        t = dict(self.t)
        if inplace:
            name = "x" if c.kernel == "mlp" else "res"
            buf = self.slots[name].buf.cuda()
            t[name] = V.mat(self.slots[name], buf)
            slots[V.out_name(c)] = self.slots[name]
            bufs = {V.out_name(c): buf}
            o = {V.out_name(c): t[name]}
        else:
            if c.inplace:
                slots[V.out_name(c)] = V._slot_out(torch.float32, 1, c.M, c.N if c.kernel != "mlp" else V.D, c.N if c.kernel != "mlp" else V.D, 16)
            bufs = {k: s.buf.cuda() for k, s in slots.items()}
            o = {k: V.mat(s, bufs[k]) for k, s in slots.items()}
        launch(self.ops, c, t, o, **kw)
        torch.cuda.synchronize()
        return {k: b.cpu() for k, b in bufs.items()}, slots


def launch(ops, c, t, o, workgroups=None, walkers=None, occupancy=None):
    """one launch of case c on the tensors t into the outputs o, through ppt_amd.ops"""
    g = t.get
    occupancy = c.occupancy if occupancy is None else occupancy
    with ops.persistent_occupancy(occupancy) if occupancy < 100 else contextlib.nullcontext():
        if c.kernel == "lnlin":
            ops.lnlin(t["x"], t["Wt"], (t["gam"], t["bet"]), bias=g("bias"), ln_eps=V.EPS, out=o["C"])
        elif c.kernel == "mlp":
            proj = (t["pa"], t["Wpt"], g("pb"), g("prs"), c.prs_rows) if c.proj else None
            ops.vit_mlp(t["x"], t["W1t"], t["b1"], t["W2t"], t["b2"], (t["gam"], t["bet"]), out=o["out"], ln_eps=V.EPS, row_scale=g("rs"),
                        row_scale_rows=c.rs_rows, residual2=g("res2"), workgroups=c.workgroups if workgroups is None else workgroups, proj=proj)
        elif c.form == "res":
            ops.rowgemm(t["A"], t["W"], bias=g("bias"), out=o["C"], residual=t["res"], residual2=g("res2"), row_scale=g("rs"),
                        row_scale_rows=c.rs_rows, walkers=c.walkers if walkers is None else walkers)
        else:
            ln = c.form == "ln"
            ops.rowgemm(t["x"] if ln else t["A"], t["W"], ln=(t["gam"], t["bet"]) if ln else None, ln_eps=V.EPS,
                        ln_stats=(o["mean"][0], o["rstd"][0]) if c.ln_stats else None, bias=g("bias"), act=c.act, out=o["C"], out2=o.get("out2"),
                        walkers=c.walkers if walkers is None else walkers)


def _windows(slots, bufs):
    return {k: V.mat(slots[k], b).clone() for k, b in bufs.items()}


def _outside_same(slot, buf, original):
    """an in-place output: everything outside the window still holds the operand buffer's (NaN) bits"""
    inside = torch.zeros(buf.numel(), dtype=torch.bool)
    V.view(slot, inside).fill_(True)
    return bool((V.bits(buf)[~inside] == V.bits(original)[~inside]).all())


@pytest.mark.parametrize("run", V.RUNS, ids=V.run_id)
def test_vit_block_against_fp64(ops, cus, run):
    c, fmt = run
    L = Launch(ops, c, fmt)
    tag = V.describe(c, fmt, cus)
    first, slots = L.call()
    second, _ = L.call()
    errors = []
    for k, b in first.items():
        if not torch.equal(V.bits(b), V.bits(second[k])):
            errors.append(f"{tag} {k}: a second call returned other bits")
        if c.inplace and k == V.out_name(c):
            if not _outside_same(slots[k], b, L.inplace_slot.buf):
                errors.append(f"{tag} {k}: written outside its window (in place)")
        else:
            if not V.outside_intact(slots[k], b):
                errors.append(f"{tag} {k}: written outside its [{slots[k].rows}, {slots[k].cols}] window")
            if V.any_sentinel_inside(slots[k], b):        # (no value within the bound is the sentinel: the CPU test asserts it)
                errors.append(f"{tag} {k}: returned with the sentinel still in it")
    win = _windows(slots, first)
    for gelu in ("poly", "erf") if V.uses_gelu(c) else ("poly",):
        V.check(c, fmt, win, errors, what="VIT-GPU", gelu=gelu, cus=cus)
    if c.inplace:
        apart, aslots = L.call(inplace=False)
        k = V.out_name(c)
        if not torch.equal(V.bits(V.mat(aslots[k], apart[k]).contiguous()), V.bits(win[k].contiguous())):
            errors.append(f"{tag} {k}: in place and out of place differ")
        if not V.outside_intact(aslots[k], apart[k]):
            errors.append(f"{tag} {k}: written outside its window (out of place)")
    assert not errors, "\n".join(errors)


def test_the_table_reaches_the_chunk_geometries_on_this_device(cus):
    cov = V.coverage(cus)
    assert {1, 15, 16, 17, 32, 48, 64, 65, 79, 80} <= cov["rows_per_chunk"], (cus, cov["rows_per_chunk"])
    assert cov["occupancy"] == {(160, 80), (513, 74)}, (cus, cov["occupancy"])
    assert {1, 2, 3} <= cov["chunks_per_workgroup"] and cov["last_one_row"] and cov["last_block_shorter"] and cov["second_division"]


# ------------------------------------------------------------------------------------------------ exact equalities
def _ids(pairs):
    return [V.run_id(p) for p in pairs]


_FULL = dict(rs_rows=13, zeros=True, res2=True, proj="wbs", prs_rows=11)
_GRID_RUNS = [(c, f) for c in V.CASES for f in V.FMTS if c.kernel == "mlp" and c.M == 331 and c.workgroups == 2 and not c.inplace
              and (c.proj, c.rs_rows, c.res2) in (("", 0, False), ("wbs", 13, True))] + \
             [(c, "bf16" if i % 2 else "f16") for i, c in enumerate(c for c in V.CASES if c.kernel == "rowgemm" and c.M == 787 and not c.inplace)]


@pytest.mark.parametrize("run", _GRID_RUNS, ids=_ids(_GRID_RUNS))
def test_result_does_not_depend_on_the_grid(ops, cus, run):
    """which workgroup takes a chunk / a row tile, and how many rows a chunk has, changes nothing a row computes"""
    c, fmt = run
    L = Launch(ops, c, fmt)
    base, slots = L.call()
    if c.kernel == "mlp":
        others = [dict(workgroups=1), dict(workgroups=3), dict(workgroups=0), dict(workgroups=0, occupancy=50), dict(workgroups=7)]
    else:
        others = [dict(walkers=0), dict(walkers=16), dict(walkers=0, occupancy=50), dict(walkers=0, occupancy=10)]
    for kw in others:
        got, _ = L.call(**kw)
        for k, b in base.items():
            assert torch.equal(V.bits(b), V.bits(got[k])), f"{V.describe(c, fmt, cus)} {k}: differs with {kw}"


_SUB_RUNS = [(c, f) for c in V.CASES for f in V.FMTS if not c.inplace and c.family == "unit" and (
    (c.kernel == "mlp" and c.M == 331 and c.workgroups == 2 and (c.proj, c.rs_rows, c.res2) in (("", 0, False), ("wbs", 13, True)))
    or (c.kernel == "lnlin" and c.M == 577) or (c.kernel == "rowgemm" and c.M == 787))]


@pytest.mark.parametrize("run", _SUB_RUNS, ids=_ids(_SUB_RUNS))
def test_rows_alone_equal_rows_in_the_batch(ops, cus, run):
    """rows [r0, r1) as a launch of their own (other chunk geometry, other tiles) return the bits they have inside the batch;
    r0 is a multiple of both sample sizes so that the per-sample factors line up"""
    c, fmt = run
    L = Launch(ops, c, fmt)
    base, slots = L.call()
    win = _windows(slots, base)
    r0 = 143 if c.kernel == "mlp" else 37 * 4                     # lcm(13, 11); a multiple of the residual form's 37
    r1 = min(c.M, r0 + 101)
    t = dict(L.t)
    for k in ("x", "A", "res", "res2", "pa"):
        if k in t:
            t[k] = t[k][r0:r1].clone()
    if "rs" in t:
        t["rs"] = t["rs"][r0 // c.rs_rows:].clone()
    if "prs" in t:
        t["prs"] = t["prs"][r0 // c.prs_rows:].clone()
    o = {k: torch.zeros((r1 - r0, w.shape[1]), dtype=w.dtype, device="cuda") for k, w in win.items() if k not in ("mean", "rstd")}
    for k in ("mean", "rstd"):
        if k in win:
            o[k] = torch.zeros((1, r1 - r0), dtype=torch.float32, device="cuda")
    launch(ops, c._replace(M=r1 - r0), t, o, workgroups=0 if c.kernel == "mlp" else None, walkers=0 if c.kernel == "rowgemm" else None)
    torch.cuda.synchronize()
    for k, w in win.items():
        want = w[:, r0:r1] if k in ("mean", "rstd") else w[r0:r1]
        assert torch.equal(V.bits(o[k].cpu()), V.bits(want.contiguous())), f"{V.describe(c, fmt, cus)} {k}: rows {r0}..{r1} alone differ"


# ------------------------------------------------------------------------------------------------ refusals
def _sent(shape, dt):
    t = torch.empty(shape, dtype=dt, device="cuda")
    V.bits(t).fill_(V._sentinel(dt))
    return t


def _base(kernel):
    """a valid launch as raw parameter-struct fields + its tensors (bf16); every output sentinel-filled"""
    from ppt_amd import _lib
    M, h = 40, torch.bfloat16
    r = lambda *s: torch.randn(*s, device="cuda")
    if kernel == "lnlin":
        t = dict(x=r(M, 384), W=r(768, 384).to(h), C=_sent((M, 768), h), g=r(384), b=r(768))
        f = dict(x=t["x"], W=t["W"], C=t["C"], ln_w=t["g"], ln_b=t["g"], ln_eps=1e-5, bias=t["b"], M=M, N=768, K=384, dtype=_lib.PPT_BF16)
        return _lib.LnLinParams, ["ppt_lnlin"], f, t, ["C"]
    if kernel == "mlp":
        t = dict(x=r(M, 384), out=_sent((M, 384), torch.float32), W1=r(1536, 384).to(h), W2=r(384, 1536).to(h), g=r(384), b1=r(1536), rs=r(M),
                 r2=r(M, 384), pa=r(M, 384).to(h), wp=r(384, 384).to(h))
        f = dict(x=t["x"], out=t["out"], W1=t["W1"], W2=t["W2"], ln_w=t["g"], ln_b=t["g"], ln_eps=1e-5, b1=t["b1"], b2=t["g"], M=M, D=384,
                 hidden=1536, dtype=_lib.PPT_BF16)
        return _lib.VitMlpParams, ["ppt_vit_mlp_bf16", "ppt_vit_mlp3_bf16"], f, t, ["out"]
    t = dict(A=r(M, 384).to(h), W=r(392, 384).to(h), C=_sent((M, 392), h), c2=_sent((M, 392), h), res=_sent((M, 392), torch.float32), g=r(512),
             rs=r(M), st=_sent((M,), torch.float32))
    f = dict(A=t["A"], W=t["W"], C=t["C"], M=M, N=392, K=384, dtype=_lib.PPT_BF16)
    return _lib.RowGemmParams, ["ppt_rowgemm_bf16"], f, t, ["C", "c2", "res", "st"]


def _raw(ops, struct, entry, fields):
    from ppt_amd import _lib
    p = struct()
    for k, v in fields.items():
        setattr(p, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return getattr(_lib.lib(), entry)(ctypes.byref(p), ops._stream())


@pytest.mark.parametrize("kernel,name,change,code", V.REFUSALS, ids=[f"{r[0]}-{r[1]}" for r in V.REFUSALS])
def test_vit_block_refuses(ops, kernel, name, change, code):
    struct, entries, f, t, outs = _base(kernel)
    for entry in entries:
        assert _raw(ops, struct, entry, f) == 0, f"{entry}: the base launch is valid"
        torch.cuda.synchronize()
        for k in outs:
            V.bits(t[k]).fill_(V._sentinel(t[k].dtype))
        g = dict(f)
        for k, v in change.items():
            if not isinstance(v, tuple):
                g[k] = v
            elif v[0] == "null":
                g[k] = None
            elif v[0] == "off":
                g[k] = f[k].data_ptr() + v[1]
            elif v[0] == "buf":
                g[k] = t[v[1]]
            else:
                g[k] = t[v[1]].data_ptr() + v[2]
        assert _raw(ops, struct, entry, g) == code, f"{entry} {name}"
        torch.cuda.synchronize()
        for k in outs:
            assert bool((V.bits(t[k].cpu()) == V._sentinel(t[k].dtype)).all()), f"{entry} {name}: {k} was written by a refused launch"
