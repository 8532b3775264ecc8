"""CPU: the criterion of tests/attn_ref.py checked without a GPU, on the cases and inputs of tests/test_attention_gpu.py.

A correct result in another summation order (rounded_tiled) must pass with room to spare -- maximum ratio <= 1.0, half the cap --
and every model broken on purpose (attn_ref.MUTATIONS) must fail, with a ratio above the cap in at least one part.

One mutation the criterion CANNOT see as stated, and why: `delta_unrounded` (delta = rowsum(out * dout) from the fp32 out instead
of the stored 16-bit out).  That model is CLOSER to fp64 than the rounding model, not further, so taken as x its ratio is below
1; the test below pins that down (the figures are printed: pytest -s) instead of dropping the mutation.  The error of delta's
input is what row_ratio's `sens` term is made of.
"""
import pytest
import torch

import attn_ref as R

CASE_IDS = [R.case_id(c) for c in R.CASES]
BY_ID = {R.case_id(c): c for c in R.CASES}


def _args(c, dtype):
    qkv, dout = R.inputs(c, dtype)
    return qkv, dout, c.n, c.T, c.P, c.H, R.SCALE, c.causal


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_name)
@pytest.mark.parametrize("c", R.CASES, ids=CASE_IDS)
def test_tiled_model_passes_at_half_the_cap(c, dtype):
    ref, model = R.references(c, dtype)
    til = R.rounded_tiled(*_args(c, dtype), dtype)
    res = R.ratios(c.H, til.out, til.dqkv, model, ref, dtype)
    print(f"ATTN-REF tiled {R.case_id(c)} {R.dtype_name(dtype)} " + " ".join(f"{k}={v[0]:.3f}" for k, v in res.items()))
    for part, (ratio, where) in res.items():
        assert ratio <= R.CAP / 2, f"{R.case_id(c)} {R.dtype_name(dtype)} {part}: ratio {ratio:.3f} at (row, head) {where}"
    for name, lse in (("rounded", model.lse), ("rounded_tiled", til.lse)):
        rel, i, err, tol = R.lse_check(lse, ref)
        assert rel <= 1.0, f"{R.case_id(c)} {R.dtype_name(dtype)} {name} lse: |err| {err:.3e} > bound {tol:.3e} at flat index {i}"


def test_t1_output_is_v_exactly():
    """T = 1: out = v and both errors are 0 -- the floor's 2^-23 ||ref|| term keeps the ratio defined (0, not 0 / 0)"""
    c = BY_ID["plain-n3-T1-H2-full"]
    for dtype in R.DTYPES:
        ref, model = R.references(c, dtype)
        qkv, _ = R.inputs(c, dtype)
        assert torch.equal(model.out, qkv[:, 2 * c.H * R.HD:].float())
        assert R.row_ratio(model.out, model.out, ref.out)[0] == 0.0


# (mutation, case, dtype): each on shapes where it can act
F16, BF16 = torch.float16, torch.bfloat16
MUTANTS = [
    ("mask_wide", "plain-n3-T77-H8-causal", F16), ("mask_wide", "plain-n2-T300-H4-causal-gain3", BF16),
    ("mask_wide", "prefix-n5-T37-P17-H8-causal", BF16),
    ("drop_last_key", "plain-n7-T65-H2-full", F16), ("drop_last_key", "plain-n2-T63-H3-causal", BF16),
    ("drop_last_key", "plain-n2-T513-H6-full", F16),
    ("cross_prompt", "prefix-n5-T37-P17-H8-causal", F16), ("cross_prompt", "prefix-n3-T150-P130-H2-causal", BF16),
    ("cross_prompt", "prefix-n3-T77-P76-H2-causal", F16),
    ("bf16_inside", "plain-n3-T77-H8-causal", F16), ("bf16_inside", "plain-n3-T200-H2-full", F16),
    ("bf16_inside", "plain-n1-T513-H8-full-gain2", F16), ("bf16_inside", "prefix-n40-T77-P17-H8-causal", F16),
    ("fold_missing_copy", "prefix-n5-T37-P17-H8-causal", F16), ("fold_missing_copy", "prefix-n40-T77-P17-H8-causal", BF16),
    ("fold_missing_copy", "prefix-n6-T20-P1-H2-causal", BF16),
]


@pytest.mark.parametrize("mutation,cid,dtype", MUTANTS, ids=[f"{m}-{c}-{R.dtype_name(d)}" for m, c, d in MUTANTS])
def test_mutated_model_fails(mutation, cid, dtype):
    c = BY_ID[cid]
    ref, model = R.references(c, dtype)
    bad = R.rounded(*_args(c, dtype), dtype, mutate=mutation)
    res = R.ratios(c.H, bad.out, bad.dqkv, model, ref, dtype)
    print(f"ATTN-REF mutant {mutation} {cid} {R.dtype_name(dtype)} " + " ".join(f"{k}={v[0]:.1f}" for k, v in res.items()))
    assert max(v[0] for v in res.values()) > R.CAP, res


@pytest.mark.parametrize("cid,dtype", [("plain-n3-T77-H8-causal", F16), ("plain-n2-T300-H4-causal-gain3", BF16)])
def test_delta_from_the_unrounded_out_is_not_visible(cid, dtype):
    """(module docstring) the mutant sits closer to fp64 than the model in dQ and dK and equals it elsewhere"""
    c = BY_ID[cid]
    ref, model = R.references(c, dtype)
    bad = R.rounded(*_args(c, dtype), dtype, mutate="delta_unrounded")
    res = R.ratios(c.H, bad.out, bad.dqkv, model, ref, dtype)
    print(f"ATTN-REF mutant delta_unrounded {cid} {R.dtype_name(dtype)} " + " ".join(f"{k}={v[0]:.3f}" for k, v in res.items()))
    n = c.H * R.HD
    assert torch.equal(bad.out, model.out) and torch.equal(bad.dqkv[:, 2 * n:], model.dqkv[:, 2 * n:])
    assert not torch.equal(bad.dqkv[:, :2 * n], model.dqkv[:, :2 * n])
    err = lambda t: float((t.dqkv[:, :2 * n].double() - ref.dqkv[:, :2 * n]).norm())
    assert err(bad) < err(model) and max(v[0] for v in res.values()) <= R.CAP
