"""GPU: the 16-bit attention kernels (csrc/attention_mfma.hip, and csrc/attention.hip for unaligned pointers), both operand
formats, through ppt_amd.ops, against the fp64 reference and the rounding model of tests/attn_ref.py.

Every case checks out, dq, dk, dv per (row, head) of 64 values -- ||kernel - fp64|| <= 2 (||model - fp64|| + floor), attn_ref.row_ratio
-- the LSE against its fp32-accumulation bound (attn_ref.lse_check), and that a second call returns the same bits.  The shapes
choose the kernel (attn_ref.CASES says which edge each one is for; attn_ref.family names the kernels in a failure); no switch of
the launchers is set.  The measured figures are printed (pytest -s) as part=ratio@row.head: profiles/r12_attention_tests.md holds them.
"""
import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu
CASE_IDS = [R.case_id(c) for c in R.CASES]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ppt_amd import ops as _ops
    return _ops


def _run(ops, c, qkv, dout):
    """forward + backward of one case -> (out, lse, dqkv) on the device"""
    if c.P:
        out, lse = ops.attention_prefix_fwd(qkv, c.n, c.T, c.P, c.H, R.SCALE)
        return out, lse, ops.attention_prefix_bwd(qkv, out, dout, lse, c.n, c.T, c.P, c.H, R.SCALE)
    out, lse = ops.attention_fwd(qkv, c.n, c.T, c.H, R.SCALE, c.causal)
    return out, lse, ops.attention_bwd(qkv, out, dout, lse, c.n, c.T, c.H, R.SCALE, c.causal)


def _unaligned(t):
    """a contiguous copy of t that starts 8 bytes into its buffer"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[4:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 8
    return v


def _check(c, dtype, what, fam, out, lse, dqkv, ref, model, errors):
    tag = f"{R.case_id(c)} {R.dtype_name(dtype)} [{what}: {fam}]"
    res = R.ratios(c.H, out, dqkv, model, ref, dtype)
    rel, i, err, tol = R.lse_check(lse, ref)
    print(f"ATTN-GPU {R.case_id(c)} {R.dtype_name(dtype)} {what} " + " ".join(f"{k}={v[0]:.3f}@{v[1][0]}.{v[1][1]}" for k, v in res.items())
          + f" lse_err={err:.2e} lse_bound={tol:.2e}")
    for part, (ratio, where) in res.items():
        if not ratio <= R.CAP:
            errors.append(f"{tag} {part}: ratio {ratio:.3f} > {R.CAP} at (row, head) {where}")
    if not rel <= 1.0:
        errors.append(f"{tag} lse: |err| {err:.3e} > bound {tol:.3e} at flat index {i} of {tuple(lse.shape)}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_name)
@pytest.mark.parametrize("c", R.CASES, ids=CASE_IDS)
def test_attention_16bit_against_fp64(ops, c, dtype):
    qkv_c, dout_c = R.inputs(c, dtype)
    ref, model = R.references(c, dtype)
    qkv, dout = qkv_c.cuda(), dout_c.cuda()
    assert qkv.data_ptr() % 16 == 0 and dout.data_ptr() % 16 == 0
    out, lse, dqkv = _run(ops, c, qkv, dout)
    out2, lse2, dqkv2 = _run(ops, c, qkv, dout)
    torch.cuda.synchronize()
    errors = []
    for name, a, b in (("out", out, out2), ("lse", lse, lse2), ("dqkv", dqkv, dqkv2)):
        if not torch.equal(a.view(torch.int16 if a.dtype != torch.float32 else torch.int32), b.view(torch.int16 if b.dtype != torch.float32 else torch.int32)):
            errors.append(f"{R.case_id(c)} {R.dtype_name(dtype)} [{R.family(c)}] {name}: a second call returned other bits")
    out, lse, dqkv = out.cpu(), lse.cpu(), dqkv.cpu()
    if c.group != "fallback":
        _check(c, dtype, "kernels", R.family(c), out, lse, dqkv, ref, model, errors)
    else:
        # the table's shape through the MFMA kernels (aligned, above) and through the fallbacks: both against the same model, and
        # the fallbacks' distance from the aligned result under the same cap
        _check(c, dtype, "aligned", R.family(c._replace(group="plain")), out, lse, dqkv, ref, model, errors)
        uq = _unaligned(qkv)
        out_u, lse_u, dqkv_u = (t.cpu() for t in _run(ops, c, uq, dout))
        assert torch.equal(uq, qkv)
        _check(c, dtype, "unaligned", R.family(c), out_u, lse_u, dqkv_u, ref, model, errors)
        shifted = R.ratios(c.H, ref.out + (out_u.double() - out.double()), ref.dqkv + (dqkv_u.double() - dqkv.double()), model, ref, dtype)
        print(f"ATTN-GPU {R.case_id(c)} {R.dtype_name(dtype)} unaligned-vs-aligned " + " ".join(f"{k}={v[0]:.3f}@{v[1][0]}.{v[1][1]}" for k, v in shifted.items()))
        for part, (ratio, where) in shifted.items():
            if not ratio <= R.CAP:
                errors.append(f"{R.case_id(c)} {R.dtype_name(dtype)} [{R.family(c)}] {part}: unaligned - aligned, ratio {ratio:.3f} > {R.CAP} "
                              f"at (row, head) {where}")
    assert not errors, "\n".join(errors)
