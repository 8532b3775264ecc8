"""CPU: the criterion of tests/vit_block_ref.py (what tests/test_vit_block_gpu.py holds ppt_lnlin, ppt_rowgemm_bf16 and the two
fused MLP kernels to) is pinned here without a GPU: a correct computation in fp32 in another summation order (the stand-in) meets
the hard bound everywhere and the sharp bound within HALF its exception budget (none at all for M < 20); each way these kernels
can break (MUTATIONS) puts more rows over the sharp bound than it allows, on at least two cases; the case table reaches the chunk
geometries it claims; the restated polynomials meet what their sources state.  Figures are printed (pytest -s):
profiles/vit_block_tests.md holds them.
"""
import math

import pytest
import torch

import vit_block_ref as V


@pytest.mark.parametrize("run", V.RUNS, ids=V.run_id)
def test_standin_meets_both_tiers(run):
    c, fmt = run
    res = V.standin(c, fmt)
    errors = []
    for gelu in ("poly", "erf") if V.uses_gelu(c) else ("poly",):
        for name, r in V.reference(c, fmt, gelu).items():
            assert torch.isfinite(r.exact).all() and torch.isfinite(r.hard).all() and torch.isfinite(r.sharp).all(), (name, "a tolerance is not finite")
            assert (r.sharp <= r.hard * (1 + 1e-12)).all(), name
            # no value a kernel may return is the sentinel: the GPU test may take a sentinel inside a window for "never written"
            # (an in-place output has no sentinel-filled buffer: it lies in its operand's)
            slot = V.inputs(c, fmt).outs.get(name)
            assert slot is None or ((r.exact - _sentinel_value(slot.buf.dtype)).abs() > r.hard).all(), (name, "the sentinel is a possible value")
        for name, v in V.check(c, fmt, res, errors, what="VIT-STANDIN", gelu=gelu).items():
            budget = 0 if c.M < 20 else V.cap(c.M) // 2
            if v.over > budget:
                errors.append(f"{V.describe(c, fmt)} {name} [{gelu}]: the stand-in needs {v.over} exceptions, {budget} is half the budget")
    assert not errors, "\n".join(errors)


def _sentinel_value(dt):
    """the sentinel of an output buffer of type dt, as the number its bits spell"""
    return float(torch.tensor([V._sentinel(dt)], dtype=torch.int32 if dt == torch.float32 else torch.int16).view(dt)[0])


def _pick(pred, fmt):
    return [(c, fmt) for c in V.CASES if pred(c)][0]


def _mlp(M, variant, **kw):
    base = dict(V._FIELDS, kernel="mlp", M=M, variant=variant, **kw)
    return lambda c: all(getattr(c, k) == v for k, v in base.items() if k not in ("note", "workgroups", "N", "K"))


def _is(kernel, **kw):
    return lambda c: c.kernel == kernel and all(getattr(c, k) == v for k, v in kw.items())


FULL = dict(rs_rows=13, zeros=True, res2=True, proj="wbs", prs_rows=11)
# mutation -> the (case, format) pairs chosen for it
MUTATION_RUNS = {
    "drop_k_fc1": [_pick(_mlp(331, 2), "bf16"), _pick(_mlp(331, 3), "f16")],
    "drop_k_fc2": [_pick(_mlp(331, 2), "f16"), _pick(_mlp(331, 3), "bf16"), _pick(_mlp(331, 3, proj="w"), "bf16")],
    "drop_k_proj": [_pick(_mlp(331, 2, proj="w"), "bf16"), _pick(_mlp(331, 3, proj="w"), "f16"), _pick(_mlp(331, 3, proj="wb"), "bf16")],
    "drop_k_rowblock": [_pick(_mlp(331, 2), "bf16"), _pick(_mlp(331, 3), "bf16"), _pick(_mlp(331, 2, proj="w"), "bf16"),
                        _pick(_is("lnlin", M=577, N=384), "f16"),
                        _pick(_is("rowgemm", M=787, form="16", K=384), "bf16"), _pick(_is("rowgemm", M=787, form="res", K=384), "f16")],
    "ring_slip": [_pick(_mlp(331, 2), "bf16"), _pick(_mlp(331, 3), "f16"), _pick(_is("lnlin", M=65, N=384), "bf16")],
    "bias_next16": [_pick(_mlp(331, 2), "bf16"), _pick(_mlp(331, 3), "bf16"), _pick(_is("lnlin", M=513, N=1152, bias=True), "bf16"),
                    _pick(_is("rowgemm", M=787, form="res", K=384), "bf16")],
    "rs_chunk_first": [_pick(_mlp(331, 2, rs_rows=37, zeros=True), "bf16"), _pick(_mlp(331, 3, rs_rows=37, zeros=True), "bf16"),
                       _pick(_mlp(331, 3, rs_rows=37), "f16"), _pick(_is("rowgemm", M=787, form="res", K=384), "bf16")],
    "rs_swapped": [_pick(_mlp(331, 2, proj="wbs", prs_rows=37, rs_rows=56, zeros=True), "bf16"),
                   _pick(_mlp(331, 3, proj="wbs", prs_rows=37, rs_rows=56, zeros=True), "f16")],
    "res2_prev_row": [_pick(_mlp(331, 2, res2=True), "bf16"), _pick(_mlp(331, 3, res2=True), "f16"),
                      _pick(_is("rowgemm", M=787, form="res", K=384), "bf16")],
    "ragged_dup": [_pick(_mlp(9, 2, **FULL), "bf16"), _pick(_mlp(9, 3, **FULL), "f16"), _pick(_is("lnlin", M=19, family="outlier"), "bf16"),
                   _pick(_is("rowgemm", M=19, family="outlier"), "f16")],
    "slice_neighbour": [_pick(_is("lnlin", M=513, N=1152, bias=True), "bf16"), _pick(_is("lnlin", M=33, N=768, bias=False), "f16")],
    "var_single_pass": [_pick(_is("lnlin", M=19, family="const"), "bf16"), _pick(_is("rowgemm", M=19, family="const"), "f16"),
                        _pick(_is("lnlin", M=70, family="const"), "f16"), _pick(_is("rowgemm", M=70, family="const"), "bf16")],
    "eps_outside": [_pick(_mlp(19, 3, family="const", rs_rows=7), "f16"), _pick(_is("lnlin", M=70, family="const"), "f16"),
                    _pick(_is("rowgemm", M=19, family="const"), "bf16"), _pick(_is("rowgemm", M=70, family="const"), "bf16")],
    "bf16_in_f16": [_pick(_is("lnlin", M=65, N=384), "f16"), _pick(_is("rowgemm", M=65, form="16", act=V.ACT_NONE, bias=True), "f16"),
                    _pick(_is("rowgemm", M=65, form="ln", K=512, act=V.ACT_QUICKGELU, out2=True), "f16")],
    "exact_gelu": [_pick(_is("rowgemm", M=70, form="16", family="bias", out2=False), "f16"),
                   _pick(_is("rowgemm", M=70, form="16", family="bias", out2=True), "f16"),
                   _pick(_is("rowgemm", M=70, form="16", family="bias", out2=False), "bf16")],
    "no_clamp": [_pick(_mlp(19, 3, family="wide", rs_rows=7), "bf16"), _pick(_mlp(81, 3, family="wide", **FULL), "f16")],
}


def test_every_mutation_has_its_cases():
    assert set(MUTATION_RUNS) == set(V.MUTATIONS)
    assert all(len(v) >= 2 for v in MUTATION_RUNS.values())


@pytest.mark.parametrize("mutation", V.MUTATIONS)
def test_mutation_exceeds_the_sharp_criterion(mutation):
    """more rows over the sharp bound than the cap allows, on every case chosen for the mutation; whether the hard bound alone
    would have caught it is printed: that column is the argument for the sharp tier"""
    missed = []
    for c, fmt in MUTATION_RUNS[mutation]:
        res = V.check(c, fmt, V.standin(c, fmt, mutation), None, what=f"VIT-MUTATION {mutation}")
        sharp = any(v.over > V.cap(c.M) for v in res.values())
        hard = any(not v.hard <= 1.0 for v in res.values())
        print(f"MUTATION {mutation} {V.case_id(c)} {fmt}: sharp {'CAUGHT' if sharp else 'missed'}, hard alone {'caught' if hard else 'MISSED'}; "
              + " ".join(f"{k}: hard {v.hard:.3g} sharp {v.sharp:.3g} rows over {v.over}/{V.cap(c.M)}" for k, v in res.items()))
        if not sharp:
            missed.append(f"{mutation} on {V.case_id(c)} {fmt}")
    assert not missed, missed


def test_the_table_reaches_the_chunk_geometries_it_claims():
    for cus in (256, 304, 80):
        cov = V.coverage(cus)
        assert {1, 15, 16, 17, 32, 48, 64, 65, 79, 80} <= cov["rows_per_chunk"], cov["rows_per_chunk"]
        assert cov["last_one_row"] and cov["last_block_shorter"] and cov["second_division"]
        assert {1, 2, 3} <= cov["chunks_per_workgroup"]
        assert cov["occupancy"] == {(160, 80), (513, 74)}, cov["occupancy"]
        assert cov["boundary_in_block"] and cov["boundary_at_chunk"] and cov["boundary_in_ragged"] and cov["zeros"]
    assert V.geometry(81, 1, 256) == (2, 41, 40, 2) and V.geometry(331, 2, 256) == (6, 56, 51, 3) and V.geometry(9, 4, 256) == (3, 3, 3, 1)
    # the shapes the existing tests use, on a 256-CU part: what the issue counted
    assert {V.geometry(M, 0, 256)[1] for M in (16416, 32832, 513, 1000, 77, 83)} == {65, 3, 4, 1}
    ks = {c.kernel for c in V.CASES}
    assert ks == {"mlp", "lnlin", "rowgemm"}
    ln = [c for c in V.CASES if c.kernel == "lnlin"]
    assert {c.M for c in ln} >= {1, 31, 32, 33, 63, 64, 65, 512, 513, 577} and {c.N for c in ln} == {384, 768, 1152}
    rg = [c for c in V.CASES if c.kernel == "rowgemm"]
    assert {(c.M, c.N, bool(c.bias)) for c in ln} >= {(M, N, b) for M in (1, 31, 32, 33, 63, 64, 65, 512, 513, 577) for N in (384, 768, 1152)
                                                       for b in (False, True)}
    assert {(c.K, c.N) for c in rg if c.form == "16"} >= {(384, 8), (384, 384), (384, 392), (384, 200), (512, 8), (512, 256), (512, 264)}
    assert {(c.M, c.N, c.K) for c in rg if c.form == "16"} >= {(M, N, K) for M in (1, 31, 32, 33, 65) for K, Ns in ((384, (8, 384, 392, 200)), (512, (8, 256, 264)))
                                                               for N in Ns}
    assert {c.N for c in rg if c.form == "res"} >= {4, 388, 516} and {c.M for c in rg} >= {1, 31, 32, 33, 65}
    tiles = (787 + 31) // 32
    assert any(c.walkers == 8 and c.M == 787 for c in rg) and 3 * 8 < tiles < 4 * 8


def test_wide_family_reaches_the_polynomials_tails():
    for c in V.CASES:
        if c.family != "wide":
            continue
        for fmt in V.FMTS:
            I = V.inputs(c, fmt)
            if c.kernel == "mlp":
                h = torch.nn.functional.layer_norm(V.mat(I.x), (384,), V.vec(I.gam), V.vec(I.bet))
                pre = h @ I.W1.float().t() + V.vec(I.b1)
            elif c.form == "16":
                pre = V.mat(I.A).float() @ I.W.float().t() + V.vec(I.bias)
            else:
                continue
            frac = float((pre.abs() > 4).float().mean())
            assert frac >= 0.1, (V.case_id(c), frac)
            assert float(pre.abs().max()) > 10.0


def test_windows_are_poisoned():
    for cid, fmt in (("mlp", "bf16"), ("lnlin", "f16"), ("rowgemm", "bf16")):
        c = [c for c in V.CASES if c.kernel == cid and (c.rs_rows or cid == "lnlin") and not c.inplace][0]
        I = V.inputs(c, fmt)
        for name in ("x", "A", "bias", "gam", "bet", "rs", "res", "res2", "b1", "b2", "pa", "pb", "prs"):
            s = getattr(I, name)
            if s is None:
                continue
            inside = torch.zeros(s.buf.numel(), dtype=torch.bool)
            V.view(s, inside).fill_(True)
            assert torch.isfinite(s.buf[inside].float()).all() and torch.isnan(s.buf[~inside].float()).all(), name
            assert s.off >= 16 and s.buf.numel() >= s.off + (s.rows + 1) * s.ld and (s.off * s.buf.element_size()) % 16 == 0, name
        for name, s in I.outs.items():
            assert V.untouched(s, s.buf) and s.buf.numel() >= s.off + (s.rows + 1) * s.ld, name
            assert (s.off * s.buf.element_size()) % 16 == 0


def test_gelu_polynomials_meet_what_their_sources_state():
    x64 = torch.linspace(-12, 12, 2_400_001, dtype=torch.float64)
    ex = V.gelu_exact(x64)
    # beyond the clamp the erf factor is the constant 4 P(16): what CLAMP3 and the source state (1 - erf(4 / sqrt 2) = 6.3e-5 and
    # the polynomial's own error at 4 on top of it)
    gap = 1.0 - float(V._erf_factor(torch.tensor(4.0, dtype=torch.float64)))
    print(f"GELU clamp: 1 - 4 P(16) = {gap:.4e}")
    assert 6.3e-5 < gap <= V.CLAMP3
    for prec in (torch.float64, torch.float32):
        x = x64.to(prec)
        e3 = (V.gelu_poly3(x).double() - ex).abs()
        e2 = (V.gelu_poly(x).double() - ex).abs()
        inside = x64.abs() <= 4
        beyond = float((e3[~inside] / x64[~inside].abs()).max())
        print(f"GELU {prec}: gelu_poly max |error| {float(e2.max()):.3e}; gelu_poly3 inside |x| <= 4: {float(e3[inside].max()):.3e}, "
              f"beyond: max |error| / |x| {beyond:.3e} (the source states {V.CLAMP3 / 2:.3e})")
        assert float(e2.max()) <= V.GELU_POLY_BOUND and float(e3[inside].max()) <= V.GELU_POLY_BOUND
        assert (e3[~inside] <= x64[~inside].abs() * V.CLAMP3 / 2 + (1e-6 if prec == torch.float32 else 0.0)).all()
        assert (e3 <= V.approx_term(x64, 3) + (1e-6 if prec == torch.float32 else 0.0)).all()
    # the slope the bound's Lipschitz factor stands for (between the jump points of gelu_poly)
    for f, lo, hi in ((V.gelu_poly3, -12, 12), (V.gelu_poly, -3.999, 3.999)):
        g = torch.linspace(lo, hi, 1_000_001, dtype=torch.float64)
        slope = float(((f(g)[1:] - f(g)[:-1]) / (g[1:] - g[:-1])).abs().max())
        print(f"GELU slope {f.__name__}: {slope:.4f}")
        assert slope <= V.GELU_LIP
    # the fp32 evaluation stays inside the term the bound carries for it
    x = x64.float()
    for f in (V.gelu_poly3, V.gelu_poly):
        d = (f(x).double() - f(x.double())).abs()
        assert (d <= V._poly32(x.double()) + V.U * f(x.double()).abs()).all()


def test_dropped_rows_collapse_to_the_residual_adds():
    """a row whose DropPath factor is exactly 0: the MLP branch contributes nothing, the sharp tolerance is the residual's own"""
    seen = 0
    for c in V.CASES:
        if c.kernel != "mlp" or not c.zeros or c.family != "unit":
            continue
        I = V.inputs(c, "bf16")
        s = V.vec(I.rs)[torch.arange(c.M) // c.rs_rows]
        dead = s == 0
        if c.proj and I.prs is not None:
            dead &= V.vec(I.prs)[torch.arange(c.M) // c.prs_rows] == 0
        if not dead.any():
            continue
        r = V.reference(c, "bf16")["out"]
        x = V.mat(I.x).double()[dead]
        want = x + (V.mat(I.res2).double()[dead] if c.res2 else 0.0)
        assert torch.equal(r.exact[dead], want), V.case_id(c)
        # (x + 0 * proj, + 0 * branch, + residual2: at most three roundings of values no larger than |x| + |out|, and the store's)
        adds = 3 * V.U * (want.abs() + x.abs()) + V._store(want, torch.zeros_like(want), torch.float32) * 2
        assert (r.sharp[dead] <= adds).all(), V.case_id(c)
        live = r.sharp[~dead].median() if (~dead).any() else float("nan")
        seen += 1
        if seen <= 3:
            print(f"DROPPED {V.case_id(c)}: {int(dead.sum())} rows; sharp tolerance max {float(r.sharp[dead].max()):.3e} against a median of {float(live):.3e} on live rows")
    assert seen >= 4


def test_the_bound_grows_on_a_nearly_constant_row():
    c = [c for c in V.CASES if c.kernel == "rowgemm" and c.family == "const" and c.M == 19][0]
    r = V.reference(c, "bf16")
    rel = r["rstd"].hard[0] / r["rstd"].exact[0]
    i = torch.arange(c.M)
    near, plain = rel[i % 8 == 3], rel[(i % 8 != 3) & (i % 8 != 5) & (i != 1)]
    print(f"RSTD relative bound: nearly constant rows {float(near.min()):.3e} .. {float(near.max()):.3e}, ordinary rows {float(plain.max()):.3e}")
    assert float(near.min()) > 100 * float(plain.max()) and math.isfinite(float(near.max()))
    assert float(r["C"].hard[i % 8 == 3].median()) > 10 * float(r["C"].hard[(i % 8 == 0)].median())
