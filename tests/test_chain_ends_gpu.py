"""GPU: the small fp32 kernels at the two ends of the prompt chain -- ppt_layernorm_fwd / _fwd_sum / _bwd / _bwd_sum (csrc/norm.hip),
ppt_rows_matmul_f32, ppt_head_logits, ppt_head_ce_bwd (csrc/head.hip), ppt_prompt_rows / ppt_prompt_rows_bwd (csrc/optim.hip) --
through ppt_amd.ops, against the fp64 references and the derived bound of tests/chain_ends_ref.py (tests/test_chain_ends_ref_cpu.py
pins that criterion without a GPU).

Every case: every output elementwise inside tol = E + R with no element excepted, nothing NaN, the documented fp32 orders bit for
bit, every operand a window of a NaN-filled buffer, every caller-owned output (dx, write_xs) a window of a sentinel-filled one that
is untouched outside the window, a second call from fresh buffers bit-identical.  Then the refusals, and the two fast-math figures
of the bound (__expf, __logf) measured through ops.head_loss on dense grids.  Ratios are printed (pytest -s):
profiles/chain_ends_tests.md holds them.
"""
import collections
import time

import pytest
import torch

import chain_ends_ref as R

pytestmark = pytest.mark.gpu
_WORST = collections.defaultdict(float)
_TIMES = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ppt_amd import ops as _ops
    yield _ops
    for k in sorted(_WORST):
        print(f"\nCHAIN-ENDS-GPU worst ratio {k}: {_WORST[k]:.3f}", end="")
    if _TIMES:
        slow = max(_TIMES, key=_TIMES.get)
        print(f"\nCHAIN-ENDS-GPU-TIME total {sum(_TIMES.values()):.1f} s over {len(_TIMES)} tests; slowest {slow}: {_TIMES[slow]:.2f} s")


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    _TIMES[request.node.name] = time.perf_counter() - t0


class Launch:
    """the operands of one launch on the device: each a window of its NaN-filled buffer, caller-owned outputs windows of
    sentinel-filled ones; intact() compares everything outside those windows with what it held before the launch"""

    def __init__(self):
        self.owned = []

    def operand(self, vals, mis=False):
        buf, _ = R.place(vals, mis)
        win = R.window(buf.cuda(), vals.shape, mis)
        assert win.is_contiguous() and win.data_ptr() % 16 == (4 if mis else 0)
        return win

    def output(self, shape, mis=False, fill=None):
        """a caller-owned fp32 output window (holding `fill`, the tensor an accumulating launch adds to, else the sentinel)"""
        buf, _ = R.place(torch.zeros(shape), mis, sentinel=True)
        if fill is None:
            R.bits(buf).fill_(R.SENTINEL[4])
        else:
            R.window(buf, shape, mis).copy_(fill)
        dbuf = buf.cuda()
        self.owned.append((dbuf, buf, tuple(shape), mis))
        return R.window(dbuf, shape, mis)

    def inplace(self, vals, mis=False):
        """an operand the launch overwrites (write_xs = x): its NaN surroundings must stay"""
        buf, _ = R.place(vals, mis)
        dbuf = buf.cuda()
        self.owned.append((dbuf, buf, tuple(vals.shape), mis))
        return R.window(dbuf, vals.shape, mis)

    def intact(self):
        return all(R.outside_same(d, b, s, m) for d, b, s, m in self.owned)


def run(ops, c):
    """one launch of case c through ppt_amd.ops from fresh buffers -> ({output: CPU tensor}, surroundings intact)"""
    I, L = R.inputs(c), Launch()
    op, out = L.operand, {}
    cpdt = R.FMT[c.copy] if c.copy else None
    if c.op in ("ln_fwd", "ln_chain"):
        x = L.inplace(I["x"]) if c.xs == "inplace" else op(I["x"], c.mis == "x")
        xs = x if c.xs == "inplace" else L.output(I["x"].shape, c.mis == "xs") if c.xs else None
        add = op(I["add"], c.mis == "add") if c.add else None
        w, b = op(I["w"]), op(I["b"])
        y, mean, rstd = ops.layernorm_fwd(x, w, b, R.FMT[c.y], add=add, add_rows=0 if c.add in ("", "full") else I["add"].shape[0],
                                          write_xs=xs, save_stats=c.stats, eps=c.eps)
        out["y"] = y
        if c.stats:
            out["mean"], out["rstd"] = mean, rstd
        if c.xs:
            out["xs"] = xs
        if c.op == "ln_chain":
            dx = L.output(I["x"].shape)
            got = ops.layernorm_bwd(op(I["dy"]), xs, w, mean, rstd, dx=dx, accumulate=False, want_wgrad=False, copy_dtype=cpdt)
            assert got[0] is dx and got[1] is None and got[2] is None
            out["dx"], out["copy"] = dx, got[3]
    elif c.op == "ln_fwd_sum":
        xs = L.output(I["x"].shape)
        y, mean, rstd = ops.layernorm_fwd_sum(op(I["x"]), op(I["bias"]) if c.bias else None, op(I["parts"]), op(I["w"]), op(I["b"]), R.FMT[c.y],
                                              xs, save_stats=c.stats, eps=c.eps)
        out["y"], out["xs"] = y, xs
        if c.stats:
            out["mean"], out["rstd"] = mean, rstd
    elif c.op in ("ln_bwd", "ln_bwd_sum", "ln_bwd_w"):
        dx = L.output(I["xs"].shape, c.mis == "dx", I["dx0"] if c.acc else None)
        dy, xs, w, mean, rstd = op(I["dy"], c.mis == "dy"), op(I["xs"], c.mis == "xs"), op(I["w"]), op(I["mean"]), op(I["rstd"])
        if c.op == "ln_bwd_sum":
            got, cp = ops.layernorm_bwd_sum(dy, xs, w, mean, rstd, dx, accumulate=c.acc, copy_dtype=cpdt)
        else:
            res = ops.layernorm_bwd(dy, xs, w, mean, rstd, dx=dx, accumulate=c.acc, want_wgrad=c.op == "ln_bwd_w",
                                    partial_rows=(c.prows or None) if c.op == "ln_bwd_w" else None, copy_dtype=cpdt)
            got, cp = res[0], res[3] if c.copy else None
            if c.op == "ln_bwd_w":
                out["dw"], out["db"] = res[1], res[2]
            else:
                assert res[1] is None and res[2] is None
        assert got is dx
        out["dx"] = dx
        if c.copy:
            out["copy"] = cp
    elif c.op == "matmul":
        out["out"] = ops.rows_matmul(op(I["a"]), op(I["w"]), alpha=c.alpha)
    elif c.op == "head":
        loss, logits, d_text = ops.head_loss(op(I["feat"], c.mis == "feat"), op(I["w"]), op(I["text"]), op(I["scale"]), I["labels"].cuda(), c.smooth)
        out.update(loss=loss, logits=logits, d_text=d_text)
    elif c.op == "rows":
        out["out"] = ops.prompt_rows(op(I["base"]), I["slot"].cuda(), op(I["tokens"]), op(I["pos"]))
    elif c.op == "rows_bwd":
        out["out"] = ops.prompt_rows_bwd(op(I["g"]), I["rows_of"].cuda(), R.N_TOK, scale=c.sc)
    else:
        raise AssertionError(c.op)
    torch.cuda.synchronize()
    return {k: v.cpu().clone() for k, v in out.items()}, L.intact()


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_chain_ends_against_fp64(ops, case):
    c, errors = case, []
    got, intact = run(ops, c)
    res = R.check(c, got, errors, what="CHAIN-ENDS-GPU")
    for name, v in res.items():
        k = f"{R.family(c, name)} {name}"
        _WORST[k] = max(_WORST[k], v)
    for name, x in got.items():
        if bool(torch.isnan(x.float()).any()):
            errors.append(f"{R.describe(c, name)} {name}: NaN in the result")
    if not intact:
        errors.append(f"{R.describe(c)}: a caller-owned buffer was written outside its window")
    if c.copy == "f32" and not torch.equal(got["copy"], got["dx"]):
        errors.append(f"{R.describe(c, 'copy')}: the fp32 copy is not dx")
    again, _ = run(ops, c)
    for name, x in got.items():
        if not torch.equal(R.bits(x.reshape(-1)), R.bits(again[name].reshape(-1))):
            errors.append(f"{R.describe(c, name)} {name}: a second call returned other bits")
    assert not errors, "\n".join(errors)


def test_rows_matmul_refusals(ops):
    g = torch.Generator().manual_seed(3)
    for M, K, N in ((8, 48, 64), (8, 1568, 64), (4, 2048, 8)):          # K % 32 != 0, K > 1536: not covered
        assert ops.rows_matmul(torch.randn(M, K, generator=g).cuda(), torch.randn(K, N, generator=g).cuda()) is None
    assert ops.rows_matmul(torch.randn(8, 64, generator=g).cuda(), torch.randn(32, 8, generator=g).cuda()) is None      # w is not [K, N]
    L = Launch()
    a, w = L.operand(torch.randn(9, 64, generator=g), True), L.operand(torch.randn(64, 16, generator=g))
    with pytest.raises(RuntimeError):                                     # a one float off alignment: refused, nothing launched
        ops.rows_matmul(a, w)
    with pytest.raises(RuntimeError):
        ops.rows_matmul(L.operand(torch.randn(9, 64, generator=g)), w, alpha=0.0)
    torch.cuda.synchronize()


def test_head_refusals(ops):
    g = torch.Generator().manual_seed(4)
    rn = lambda *s: torch.randn(*s, generator=g).cuda()
    s = torch.tensor([R.SCALE["init"]]).cuda()
    for B, F in ((2, 8224), (4097, 32)):
        with pytest.raises(RuntimeError):
            ops.head_loss(rn(B, F), rn(F, 64), rn(3, 64), s, torch.zeros(B, dtype=torch.long).cuda(), 0.2)
    torch.cuda.synchronize()


class UnitHead:
    """head_loss on feat = e_0, W[0, :] = row, text = the first C unit vectors: logits[0, c] = __expf(s) * row[c] with every sum and
    the normalisation exact; label 0, no smoothing.  The operands stay on the device; only s and the row change."""

    def __init__(self, ops, C):
        feat = torch.zeros(1, 32); feat[0, 0] = 1.0
        self.ops, self.C = ops, C
        self.feat, self.w, self.text = feat.cuda(), torch.zeros(32, 64).cuda(), torch.eye(C, 64).cuda()
        self.label = torch.zeros(1, dtype=torch.long).cuda()

    def __call__(self, s, row):
        """s: a 1-element device tensor; row: [C] device tensor -> (logits [C], loss) on the device"""
        self.w[0, :self.C] = row
        loss, logits, _ = self.ops.head_loss(self.feat, self.w, self.text, s, self.label, 0.0)
        return logits[0], loss


def test_fast_math_figures(ops):
    """the two figures chain_ends_ref's bound takes for __expf and __logf hold on dense grids, measured against fp64"""
    # __expf(s): the logit of the unit problem IS the kernel's __expf(s)
    xs = torch.cat([torch.linspace(-110.0, 6.0, 1451), torch.tensor([-700.0, -300.0, R.SCALE["init"], R.SCALE["max"]])]).float()
    head, xd, one = UnitHead(ops, 1), xs.cuda(), torch.ones(1).cuda()
    got = torch.stack([head(xd[i:i + 1], one)[0][0] for i in range(xs.numel())]).cpu().double()
    ex = torch.exp(xs.double())
    err = (got - ex).abs()
    ratio = err / (R.expf_err(xs.double()) * ex + 2.0 ** -126)
    normal = ex > 2.0 ** -120
    rel = (err / (R.U * ex))[normal]
    print(f"\nCHAIN-ENDS-GPU __expf: worst |err| / bound {float(ratio.max()):.3f} at x = {float(xs[ratio.argmax()]):.4f}; worst relative error "
          f"{float(rel.max()):.2f} u at x = {float(xs[normal][rel.argmax()]):.4f}; over [2.5, 4.7] {float(rel[(xs[normal] > 2.5) & (xs[normal] < 4.7)].max()):.2f} u; "
          f"worst (relative error / u - {R.EXPF_A:g}) / |x| = {float(((rel - R.EXPF_A) / xs[normal].abs().clamp_min(1e-3).double()).max()):.3f}")
    assert not torch.isnan(got).any() and float(ratio.max()) <= 1.0
    # __logf(se): logits (0, -x, 0, ..., 0) with label 0 and no smoothing give loss = __logf(se), se = (C - 1) + __expf(-x) within
    # what the bound already allots to se
    worst, worst_raw, at, zero = 0.0, 0.0, None, torch.zeros(1).cuda()
    for C in (2, 3, 5, 9, 17, 33, 64):
        head = UnitHead(ops, C)
        grid = torch.linspace(0.0, 24.0, 97)
        rows = torch.zeros(grid.numel(), C); rows[:, 1] = -grid
        rows = rows.cuda()
        res = [head(zero, rows[i]) for i in range(grid.numel())]
        lgs, losses = torch.stack([r[0] for r in res]).cpu().double(), torch.stack([r[1] for r in res]).cpu().double()
        for x, Lg, loss in zip(grid.tolist(), lgs, losses):
            a = Lg - Lg.max()
            se = torch.exp(a).sum()
            se_rel = (torch.exp(a) * (R.expf_err(a) + R.U)).sum() / se + R.U
            e = abs(float(loss) - float(Lg.max() + torch.log(se) - Lg[0]))
            r = e / float(R.logf_err(se) + se_rel)
            if r > worst:
                worst, at = r, (C, x)
            worst_raw = max(worst_raw, e / R.U)
    print(f"CHAIN-ENDS-GPU __logf: worst |err| / (logf figure + the sum's share) {worst:.3f} at (C, x) = {at}; worst |err| {worst_raw:.2f} u")
    assert worst <= 1.0
