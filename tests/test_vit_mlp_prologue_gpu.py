"""GPU: the prologue of ppt_vit_mlp3_bf16 (csrc/mlp_fused3.hip) -- the proj operand image filled by LDS-DMA, the DropPath factors
loaded without a branch, the constants' pieces -- through ppt_amd.ops.vit_mlp at D = 384, hidden = 1536, against the fp64 reference
and the two-tier criterion of tests/vit_block_ref.py (the bounds tests/test_vit_block_gpu.py holds this kernel to; none is set here).

  ragged image   proj on, M rows in one workgroup's chunks: `a`, x and pos are the leading M rows of buffers whose further rows are
                 NaN.  The result is finite and within the bounds, equal BIT FOR BIT to the same call with those rows zero (no row
                 at or past M reaches the image or an accumulator that is stored), and the output buffer past row M - 1 is untouched.
  factors        row_scale x proj_row_scale, each absent or with an exact zero, two samples of 81 rows: against the reference, and
                 an absent factor equals a tensor of ones bit for bit.
  chunk walk     more chunks than workgroups (workgroups = 2 over 407 rows: three chunks each) equals the default grid bit for bit:
                 the second chunk's DMA into the image does not overrun the first chunk's readers.
"""
import functools

import pytest
import torch

import vit_block_ref as V

pytestmark = pytest.mark.gpu
GUARD = 96                      # rows behind the operands: more than one chunk (80)
SENTINEL = -12345.0
_FULL = dict(rs_rows=13, zeros=True, res2=True, proj="wbs", prs_rows=11)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ppt_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _case(M, workgroups, **kw):
    return V.Case("mlp", M, V.D, V.D, variant=3, workgroups=workgroups, **kw)


class Operands:
    """a case's operands on the device; x, a and pos as the leading M rows of buffers with GUARD rows of `guard` behind them"""

    def __init__(self, ops, c, fmt, guard=float("nan")):
        I = V.inputs(c, fmt)
        self.c, self.M = c, c.M
        vec = lambda s: None if s is None else V.vec(s).clone().cuda()
        self.gam, self.bet, self.b1, self.b2, self.pb = vec(I.gam), vec(I.bet), vec(I.b1), vec(I.b2), vec(I.pb)
        self.rs, self.prs = vec(I.rs), vec(I.prs)
        self.W1t, self.W2t = ops.vit_mlp_retile(I.W1.cuda(), I.W2.cuda(), variant=3)
        self.Wpt = ops.vit_proj_retile(I.Wp.cuda()) if c.proj else None
        self.x, self.pa, self.res2 = self.rows(I.x, guard), self.rows(I.pa, guard), self.rows(I.res2, guard)

    def rows(self, slot, guard):
        if slot is None:
            return None
        v = V.mat(slot)
        buf = torch.full((self.M + GUARD, v.shape[1]), guard, dtype=v.dtype)
        buf[:self.M] = v
        return buf.cuda()

    def call(self, ops, workgroups=None, rs="own", prs="own"):
        """-> the whole output buffer (M + GUARD rows, SENTINEL behind row M - 1) on the CPU"""
        c, M = self.c, self.M
        out = torch.full((M + GUARD, V.D), SENTINEL, dtype=torch.float32, device="cuda")
        rs = self.rs if isinstance(rs, str) else rs
        prs = self.prs if isinstance(prs, str) else prs
        proj = (self.pa[:M], self.Wpt, self.pb, prs, c.prs_rows if c.prs_rows else 81) if c.proj else None
        ops.vit_mlp(self.x[:M], self.W1t, self.b1, self.W2t, self.b2, (self.gam, self.bet), out=out[:M], ln_eps=V.EPS, row_scale=rs,
                    row_scale_rows=c.rs_rows if c.rs_rows else 81, residual2=None if self.res2 is None else self.res2[:M],
                    workgroups=c.workgroups if workgroups is None else workgroups, proj=proj)
        torch.cuda.synchronize()
        return out.cpu()


def _against_reference(c, fmt, out, cus, errors):
    for gelu in ("poly", "erf"):
        V.check(c, fmt, {"out": out[:c.M]}, errors, what="VIT-PROLOGUE", gelu=gelu, cus=cus)


def _untouched(out, M):
    return bool((out[M:] == SENTINEL).all())


@pytest.mark.parametrize("fmt", V.FMTS)
@pytest.mark.parametrize("M", (1, 15, 79, 80, 81, 97, 161))
def test_ragged_image(ops, cus, M, fmt):
    c = _case(M, 1, **_FULL)                       # one workgroup: chunks of 1, 15, 79, 80, 41 + 40, 49 + 48, 54 + 54 + 53 rows
    errors = []
    out = Operands(ops, c, fmt).call(ops)
    if not torch.isfinite(out[:M]).all():
        errors.append(f"{V.describe(c, fmt, cus)}: a row of the result is not finite (NaN rows behind the operands were read)")
    _against_reference(c, fmt, out, cus, errors)
    if not _untouched(out, M):
        errors.append(f"{V.describe(c, fmt, cus)}: the output buffer was written at or past row {M}")
    zero = Operands(ops, c, fmt, guard=0.0).call(ops)
    if not torch.equal(V.bits(out[:M].contiguous()), V.bits(zero[:M].contiguous())):
        errors.append(f"{V.describe(c, fmt, cus)}: the result depends on the rows behind the operands")
    assert not errors, "\n".join(errors)


@functools.lru_cache(maxsize=None)
def _factor_case(rs, prs):
    """M = 2 x 81 rows in one workgroup (chunks of 54: the second one holds the sample boundary inside a row block).  The factors
    come from vit_block_ref.inputs (seeded by the case's fields); `walkers`, which no mlp case reads, is varied until each factor
    tensor holds an exact zero AND a non-zero value."""
    for salt in range(1, 200):
        c = _case(162, 1, walkers=salt, res2=True, zeros=True, rs_rows=81 if rs else 0, proj="wbs" if prs else "wb", prs_rows=81 if prs else 0)
        I = V.inputs(c, "f16")
        mixed = lambda s: s is None or (bool((V.vec(s) == 0).any()) and bool((V.vec(s) != 0).any()))
        if mixed(I.rs) and mixed(I.prs) and mixed(V.inputs(c, "bf16").rs) and mixed(V.inputs(c, "bf16").prs):
            return c
    raise AssertionError("no factor set with a zero and a non-zero value")


@pytest.mark.parametrize("fmt", V.FMTS)
@pytest.mark.parametrize("prs", (False, True), ids=("proj_row_scale-None", "proj_row_scale"))
@pytest.mark.parametrize("rs", (False, True), ids=("row_scale-None", "row_scale"))
def test_factors(ops, cus, rs, prs, fmt):
    c = _factor_case(rs, prs)
    L = Operands(ops, c, fmt)
    assert (L.rs is not None) == rs and (L.prs is not None) == prs
    errors = []
    out = L.call(ops)
    _against_reference(c, fmt, out, cus, errors)
    if not _untouched(out, c.M):
        errors.append(f"{V.describe(c, fmt, cus)}: the output buffer was written at or past row {c.M}")
    if not (rs and prs):                           # an absent factor is a factor of one
        ones = torch.ones(2, device="cuda")
        same = L.call(ops, rs=L.rs if rs else ones, prs=L.prs if prs else ones)
        if not torch.equal(V.bits(out.contiguous()), V.bits(same.contiguous())):
            errors.append(f"{V.describe(c, fmt, cus)}: an absent factor and a factor of ones give different bits")
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("fmt", V.FMTS)
def test_chunk_walk(ops, cus, fmt):
    M = 5 * 80 + 7
    c = _case(M, 2, **_FULL)
    n_chunks, _, _, per_wg = V.case_geometry(c, cus)
    assert n_chunks > 2 and per_wg >= 2, "more chunks than workgroups"
    L = Operands(ops, c, fmt)
    errors = []
    walked = L.call(ops)
    _against_reference(c, fmt, walked, cus, errors)
    default = L.call(ops, workgroups=0)
    if not torch.equal(V.bits(walked.contiguous()), V.bits(default.contiguous())):
        errors.append(f"{V.describe(c, fmt, cus)}: two workgroups walking {n_chunks} chunks and the default grid give different bits")
    assert not errors, "\n".join(errors)
