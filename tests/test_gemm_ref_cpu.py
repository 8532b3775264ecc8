"""CPU: the criterion of tests/gemm_ref.py checked without a GPU, on the cases and inputs of tests/test_gemm_gpu.py.

A correct launch in another summation order (gemm_ref.standin) must sit at <= tol / 2 in EVERY output of every case and format
-- C, out2, both statistics arrays, both pools; the half is asked of the arithmetic's share E of tol = E + R, gemm_ref.worst
says why --, every launch broken on purpose (gemm_ref.MUTATIONS) must exceed tol on the
cases chosen for it (at least two each, where it can act), and the two approximations whose stated bounds the tolerance leans
on (csrc/ppt_act.h: gelu_poly 2e-4, erf_fast 1.5e-7) meet them on a dense grid.  The figures are printed (pytest -s);
profiles/gemm_tests.md holds them.
"""
import pytest
import torch

import gemm_ref as R

BY_ID = {R.case_id(c): c for c in R.CASES}


@pytest.mark.parametrize("run", R.RUNS, ids=R.run_id)
def test_standin_passes_at_half_the_tolerance(run):
    c, fmt = run
    errors = []
    R.check(c, fmt, R.standin(c, fmt), errors, cap=0.5, what="GEMM-REF standin")
    assert not errors, "\n".join(errors)


def test_inputs_are_windows_in_poisoned_buffers():
    """what the GPU test relies on: NaN around every operand window, the sentinel in and around every output window"""
    c = next(c for c in R.CASES if c.res and c.group_rows and len(c.fmts) == 3)
    for fmt in c.fmts:
        I = R.inputs(c, fmt)
        for s in (I.A, I.B, I.res, I.group):
            inside = torch.zeros(s.buf.numel(), dtype=torch.bool)
            R.view(s, inside).fill_(True)
            assert torch.isnan(s.buf[~inside]).all() and (~inside).sum() >= s.off + s.ld and not torch.isnan(R.view(s)).any()
        for s in I.outs.values():
            assert R.untouched(s, s.buf) and R.outside_intact(s, s.buf) and R.any_sentinel_inside(s, s.buf)
            R.view(s).zero_()
            ok = R.outside_intact(s, s.buf) and not R.any_sentinel_inside(s, s.buf) and not R.untouched(s, s.buf)
            R.bits(s.buf).fill_(R._sentinel(s.buf.dtype))
            assert ok


def _pick(pred, n=3, fmts=None):
    return [(R.case_id(c), f) for c in R.CASES if pred(c) for f in c.fmts if fmts is None or f in fmts][:n]


# mutation -> the (case, format) runs it must fail on: shapes and operands on which it can act
MUTANTS = {
    "drop_k_last": _pick(lambda c: c.group == "A" and c.K in (8, 72), 4) + _pick(lambda c: c.group == "A" and c.K == 2048, 3),
    "drop_slab": _pick(lambda c: c.group == "A" and c.K in (128, 200), 4),
    "double_surplus": _pick(lambda c: c.group == "A" and c.K in (64, 136, 256), 5),
    "bias_next_col": _pick(lambda c: c.group == "D" and c.bias and c.act and not c.out2, 4),
    "group_neighbour": _pick(lambda c: c.group_rows == 16 and c.expect == "ok", 4),
    "row_scale_next": _pick(lambda c: c.group == "D" and c.rs_rows in (1, 7) and not c.out2, 4),
    "res_ldc": _pick(lambda c: c.group == "D" and c.res and not c.dact and not c.ldc_pad and c.c != "none", 4),
    "act_before_bias": _pick(lambda c: c.group == "D" and c.bias and c.act and not c.out2 and not c.dact, 4),
    "out2_wrong_side": _pick(lambda c: c.group == "D" and c.out2 != "", 6),
    "stats_after_act": _pick(lambda c: c.group == "E" and c.stats and c.act, 4),
    "pool_beyond_m": _pick(lambda c: c.group == "E" and c.pool and c.pool_min and not c.stats and c.M % (c.pool_rows or 32), 6),
    "stale_last_row": _pick(lambda c: c.group == "B" and c.M > 1, 3) + _pick(lambda c: c.group == "G", 2),
    "bf16_in_f16": _pick(lambda c: c.group in ("C", "G", "H") and c.c == "16", 4, ("f16",)),
}


def test_every_mutation_has_cases():
    assert set(MUTANTS) == set(R.MUTATIONS)
    for m, runs in MUTANTS.items():
        assert len({cid for cid, _ in runs}) >= 2, m


@pytest.mark.parametrize("mutation,cid,fmt", [(m, cid, f) for m, runs in MUTANTS.items() for cid, f in runs],
                         ids=lambda v: v if isinstance(v, str) else None)
def test_mutated_launch_fails(mutation, cid, fmt):
    c = BY_ID[cid]
    res = R.check(c, fmt, R.standin(c, fmt, mutate=mutation), what=f"GEMM-REF mutant {mutation}")
    assert max(res.values()) > 1.0, res


def test_activation_approximations_meet_their_stated_bounds():
    """csrc/ppt_act.h: |gelu_poly - GELU| <= 2e-4 and |erf_fast - erf| <= 1.5e-7 on [-12, 12] in steps of 1e-4.  gelu_poly holds
    its bound in fp32 arithmetic, as the kernels run it.  erf_fast's 1.5e-7 is the approximation's own error (Abramowitz &
    Stegun 7.1.26), met in fp64 arithmetic; evaluated in fp32 its five fused steps and the final 1 - p t exp(-x^2) add rounding
    of values near 1: that part must stay inside the 8 u which gemm_ref's derivative term D budgets beside the 1.5e-7."""
    x32 = (torch.arange(-120000, 120001, dtype=torch.float64) * 1e-4).float()
    x = x32.double()
    gelu = 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))
    e_gelu = float((R.gelu_poly(x32).double() - gelu).abs().max())
    e_gelu64 = float((R.gelu_poly(x) - gelu).abs().max())
    e_erf64 = float((R.erf_fast(x) - torch.erf(x)).abs().max())
    e_erf32 = float((R.erf_fast(x32).double() - torch.erf(x)).abs().max())
    print(f"GEMM-REF gelu_poly max error fp32 {e_gelu:.3e} fp64 {e_gelu64:.3e} (stated {R.GELU_POLY_BOUND:g}), "
          f"erf_fast fp64 {e_erf64:.3e} (stated {R.ERF_FAST_BOUND:g}) fp32 {e_erf32:.3e} (budget {R.ERF_FAST_BOUND + 8 * R.U:.3e})")
    assert e_gelu <= R.GELU_POLY_BOUND and e_gelu64 <= R.GELU_POLY_BOUND
    assert e_erf64 <= R.ERF_FAST_BOUND and e_erf32 <= R.ERF_FAST_BOUND + 8 * R.U
