"""CPU: the references, bounds and mutations of tests/stream_ref.py checked without a GPU, on the cases of
tests/test_stream_kernels_gpu.py.

  * every fp64 reference agrees to 1e-12 (relative to the largest value) with an independent formulation in other torch ops:
    per-group index_select + torch.var, F.batch_norm + F.max_pool1d, F.conv1d, nn.BatchNorm1d, max_k relu(bn(y_k)), a Python
    loop for torch.max's NaN / first-maximum rule;
  * an fp32 model of each kernel in ANOTHER summation order (rows reversed, serial over chunks of 7) stays within bound / SPARE:
    a quarter of the bound where the bound counts a summation, the bound itself where it is one final rounding (stream_ref's
    docstring says why no model can do better there).  An element-wise kernel has no order to change: its model takes the
    kernel's own roundings (each fmaf evaluated in fp64 and cast once).  The largest ratio per case is printed;
  * every mutation in stream_ref.MUTATIONS breaks the criterion on the case named next to it.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import stream_ref as R

F32, BF16, F16 = R.F32, R.BF16, R.F16


def _same(a, b, what, tol=1e-12):
    err = (a.double() - b.double()).abs().max().item()
    assert err <= tol * max(1.0, b.double().abs().max().item()), f"{what}: {err:.3e}"


def _sum7(t):
    """fp32 sum over dim 0 in another order: rows reversed, chunks of 7 summed and folded serially"""
    t = t.flip(0)
    acc = torch.zeros(t.shape[1:], dtype=t.dtype)
    for r0 in range(0, t.shape[0], 7):
        acc = acc + t[r0:r0 + 7].sum(0)
    return acc


def _report(name, worst, spare):
    print(f"MODEL {name}: largest error / bound {worst:.3f} (must be <= 1/{spare})")
    assert worst <= 1.0 / spare, name


# --------------------------------------------------------------------------------------------------------- group_anchor_stats
def _gas_groups(case, x, idx, anchor):
    B, Nsrc, S, K, D = case
    for b in range(B):
        for s in range(S):
            rows = torch.index_select(x, 0, b * Nsrc + idx[b, s])
            yield b, s, rows - x[b * Nsrc + anchor[b, s]]


@pytest.mark.parametrize("case", R.GAS_CASES, ids=str)
def test_group_anchor_stats_reference(case):
    x, idx, anchor = R.gas_inputs(case, F32)
    st, _ = R.gas_exact(case, x, idx, anchor)
    other, allv = torch.zeros_like(st), [[] for _ in range(case[0])]
    for b, s, d in _gas_groups(case, x.double(), idx, anchor):
        n = d.numel()
        other[b, s, 0] = d.mean() * n
        other[b, s, 1] = (d.var(unbiased=False) + d.mean() ** 2) * n
        allv[b].append(d.reshape(-1))
    _same(st, other, "stats")
    r = R.gas_rstd_exact(case, x, idx, anchor)
    _same(r, torch.stack([1.0 / (torch.var(torch.cat(v), unbiased=True).sqrt() + 1e-5) for v in allv]), "1 / (std + eps)")
    _same(R.rstd_from_stats(st, float(case[2] * case[3] * case[4])), r, "the same from the statistics")
    # the planted edges are there: rows 0 and Nsrc - 1 of the last cloud, a duplicate, an anchor inside and one outside its group
    B, Nsrc = case[0], case[1]
    assert 0 in idx[B - 1].reshape(-1).tolist() and Nsrc - 1 in idx[B - 1].reshape(-1).tolist()
    assert anchor[B - 1, 0] in idx[B - 1, 0].tolist()
    assert any(anchor[0, s] not in idx[0, s].tolist() for s in range(case[2]))
    assert len(set(idx[B - 1].reshape(-1).tolist())) < idx[B - 1].numel()


def test_group_anchor_stats_model_in_another_order():
    worst = worst_r = 0.0
    for case in R.GAS_CASES:
        for dtype in (F32, BF16):
            x, idx, anchor = R.gas_inputs(case, dtype)
            st, bound = R.gas_exact(case, x, idx, anchor)
            model = torch.zeros(st.shape, dtype=F32)
            for b, s, d in _gas_groups(case, x.float(), idx, anchor):
                d = d.t().reshape(-1, 1)                                    # channel-major instead of neighbour-major
                model[b, s, 0], model[b, s, 1] = _sum7(d)[0], _sum7(d * d)[0]
            worst = max(worst, R.ratio(model, st, bound))
            n = float(case[2] * case[3] * case[4])
            worst_r = max(worst_r, R.ratio(R.rstd_from_stats(model, n).float(), R.gas_rstd_exact(case, x, idx, anchor),
                                           R.rstd_bound(st, n, bound)))
    _report("group_anchor_stats", worst, 4)
    _report("group_anchor_stats -> cloud_rstd", worst_r, 4)


@pytest.mark.parametrize("S", R.RSTD_S)
def test_cloud_rstd_reference_and_model(S):
    st, n = R.rstd_inputs(S)
    r = R.rstd_from_stats(st, n)
    # the formulation: unbiased variance from the moments, var = (E x^2 - (E x)^2) n / (n - 1)
    m1, m2 = st.double()[..., 0].sum(1) / n, st.double()[..., 1].sum(1) / n
    other = 1.0 / (((m2 - m1 * m1) * n / (n - 1.0)).clamp_min(0).sqrt() + 1e-5)
    assert ((r - other).abs() <= 1e-12 * other.abs()).all(), "r, every cloud relative to its own value"
    want0 = torch.tensor(1.0 / 1e-5, dtype=torch.float64).float()
    assert r[1].float() == want0 and r[2].float() == want0, "a cloud of equal values: variance exactly 0"
    model = R.rstd_from_stats(st.flip(1), n).float()
    _report(f"cloud_rstd S {S}", R.ratio(model, r, R.rstd_bound(st, n)), 1)


# ------------------------------------------------------------------------------------------------------------ bn_res_act_rows
def test_bn_res_act_rows_cases_reach_every_instantiation():
    reached = {c[0].split("-")[0] for c in R.BRA_CASES}
    assert reached == set(R.BRA_INSTANTIATIONS)
    assert any(c[6] and c[1][1] % 8 == 0 for c in R.BRA_CASES)              # the alignment fallback with C % 8 == 0


@pytest.mark.parametrize("cid", [c[0] for c in R.BRA_CASES])
def test_bn_res_act_rows_reference_and_model(cid):
    case = R.BRA_BY_ID[cid]
    _, (M, C, pool), xd, rd, yd, aff, _ = case
    x, res, sc, sh, rs, rh = R.bra_inputs(case)
    ref, bound = R.bra_exact(case, x, res, sc, sh, rs, rh)
    zeros, ones = torch.zeros(C, dtype=torch.float64), torch.full((C,), 1.0 - 1e-5, dtype=torch.float64)   # var + eps = 1
    t = F.batch_norm(x.double(), zeros, ones, sc.double(), sh.double(), False, 0.0, 1e-5)
    rr = torch.relu(F.batch_norm(res.double(), zeros, ones, rs.double(), rh.double(), False, 0.0, 1e-5)) if aff else res.double()
    other = F.max_pool1d(torch.relu(t + rr).t()[None], pool)[0].t()
    _same(ref, other, "y")
    assert (ref[0, 1] == 0).all() and (ref > 0).any(), "the all-negative group gives exactly 0"
    # the kernel's roundings: each fmaf evaluated in fp64 and cast once, their sum one fp32 addition
    t32 = (sc.double() * x.double() + sh.double()).float()
    rr32 = torch.relu((rs.double() * res.double() + rh.double()).float()) if aff else res.float()
    model = torch.relu(t32 + rr32).view(M // pool, pool, C).amax(1).to(yd)
    _report("bn_res_act_rows " + cid, R.ratio(model, ref, bound, yd), 1)


# ------------------------------------------------------------------------------------------------------------------ gather_add
def _chan(ps, pm, counts):
    n, mean, m2 = 0.0, None, None
    for s, q, c in zip(ps.double(), pm.double(), counts):
        if mean is None:
            n, mean, m2 = float(c), s / c, q
            continue
        d, tot = s / c - mean, n + c
        mean, m2, n = mean + d * (c / tot), m2 + q + d * d * (n * c / tot), tot
    return mean, m2 / n


@pytest.mark.parametrize("case", R.GA_CASES, ids=str)
def test_gather_add_reference_and_model(case):
    B, Nsrc, S, K, C = case
    P, Q, idx = R.ga_inputs(case)
    (ps, pm), (bs, bm), v = R.ga_exact(case, P, Q, idx)
    M = B * S * K
    rows = torch.stack([P[(m // (S * K)) * Nsrc + idx.reshape(-1)[m]].double() + Q[m // K].double() for m in range(M)])
    _same(v, rows, "rows")
    counts = [n for _, n in R._chunks(M, R.GA_CHUNK)]
    assert counts[-1] == (M % 32 or 32)
    for p, (r0, n) in enumerate(R._chunks(M, R.GA_CHUNK)):
        _same(ps[p], rows[r0:r0 + n].mean(0) * n, "chunk sum")
        _same(pm[p], torch.var(rows[r0:r0 + n], 0, unbiased=False) * n, "chunk M2")
    mean, var = R.moments_exact(v)
    cm, cv = _chan(ps, pm, counts)
    _same(mean, cm, "Chan's merge of the exact partials is the mean")
    _same(var, cv, "... and the biased variance")
    assert torch.equal(R.ga_y(case, P, Q, idx, BF16).float(), rows.float().to(BF16).float())
    # fp32 model, rows of a chunk reversed, chunks of 7
    p32, q32 = R._ga_rows(case, P, Q, idx)
    y32 = p32 + q32
    ms, mm = [], []
    for r0, n in R._chunks(M, R.GA_CHUNK):
        c = y32[r0:r0 + n]
        s = _sum7(c)
        ms.append(s)
        mm.append(_sum7((c - s / n) ** 2))
    ms, mm = torch.stack(ms), torch.stack(mm)
    _report(f"gather_add {case} partial sums", R.ratio(ms, ps, bs), 4)
    _report(f"gather_add {case} partial M2", R.ratio(mm, pm, bm), 4)
    fm, fv = _chan(ms, mm, counts)
    fm, fv = fm.float(), fv.float()
    frstd = 1.0 / torch.sqrt(fv + torch.tensor(R.BN_EPS, dtype=F32))
    bmean, bvar, brstd = R.finalize_bound((ps, pm), (bs, bm), M, R.GA_CHUNK)
    worst = max(R.ratio(fm, mean, bmean), R.ratio(fv, var, bvar), R.ratio(frstd, 1.0 / (var + R.BN_EPS).sqrt(), brstd))
    _report(f"gather_add {case} -> bn_finalize", worst, 4)


# ----------------------------------------------------------------------------------------------------------------- pool_finish
@pytest.mark.parametrize("case", R.PF_CASES, ids=lambda c: f"{R.dtype_name(c[0])}-{R.dtype_name(c[1])}-fold{c[2]}")
def test_pool_finish_reference_and_model(case):
    pd, od, fold = case
    pmax, pmin, sc, sh = R.pf_inputs(case)
    ref, bound = R.pf_exact(case, pmax, pmin, sc, sh)
    scd, shd = sc.double(), sh.double()
    cand = torch.where(scd >= 0, torch.relu(scd * pmax.double() + shd), torch.relu(scd * pmin.double() + shd))   # max_k relu(bn(y_k))
    _same(ref, cand.view(R.PF_G, fold, R.PF_C).amax(1), "out")
    assert (sc == 0).any() and (sc < 0).any() and (sc > 0).any() and torch.equal(ref[:, 0], torch.full((R.PF_G,), 0.25, dtype=torch.float64))
    sel = torch.where(sc >= 0, pmax.float().view(R.PF_G, fold, R.PF_C).amax(1), pmin.float().view(R.PF_G, fold, R.PF_C).amin(1))
    model = torch.relu((sc.double() * sel.double() + sh.double()).float()).to(od)          # one fmaf: fp64, cast once
    _report(f"pool_finish {R.dtype_name(pd)} -> {R.dtype_name(od)} fold {fold}", R.ratio(model, ref, bound, od), 1)


# ----------------------------------------------------------------------------------------------------------------- conv1_stats
@pytest.mark.parametrize("case", R.C1_CASES, ids=str)
def test_conv1_stats_reference_and_model(case):
    M, C = case
    pts, w1, b1 = R.c1_inputs(case)
    (ps, pm), (bs, bm), y = R.c1_exact(case, pts, w1, b1)
    conv = F.conv1d(pts.double().t()[None], w1.double()[:, :, None], b1.double())[0].t()
    _same(y, conv, "y")
    chunks = R._chunks(M, R.C1_CHUNK)
    for p, (r0, n) in enumerate(chunks):
        _same(ps[p], conv[r0:r0 + n].mean(0) * n, "chunk sum")
        _same(pm[p], torch.var(conv[r0:r0 + n], 0, unbiased=False) * n, "chunk M2")
    g = torch.Generator().manual_seed(M + C)
    gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), 1.0 + torch.rand(C, generator=g)
    sc, sh, nrm, nrv = R.bn_affine_exact(y, gamma, beta, rm, rv, R.BN_MOM)
    bn = torch.nn.BatchNorm1d(C, eps=R.BN_EPS, momentum=R.BN_MOM).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
        out = bn(y)
    _same(sc * y + sh, out, "scale * y + shift is BatchNorm1d")
    _same(nrm, bn.running_mean, "running mean")
    _same(nrv, bn.running_var, "running variance")
    # model: fp64 in another order, cast once; the finalize in fp32 from fp64 Chan merges
    ms = torch.stack([y[r0:r0 + n].flip(0).sum(0) for r0, n in chunks]).float()
    mm = torch.stack([((y[r0:r0 + n] - y[r0:r0 + n].mean(0)) ** 2).flip(0).sum(0) for r0, n in chunks]).float()
    _report(f"conv1_stats {case} partials", max(R.ratio(ms, ps, bs), R.ratio(mm, pm, bm)), 1)
    mom = float(torch.tensor(R.BN_MOM, dtype=F32))
    sc, sh, nrm, nrv = R.bn_affine_exact(y, gamma, beta, rm, rv, mom)
    fm, fv = _chan(ms, mm, [n for _, n in chunks])
    fm32, fv32 = fm.float(), fv.float()
    msc = gamma / torch.sqrt(fv32 + torch.tensor(R.BN_EPS, dtype=F32))
    msh = beta - fm32 * msc
    k = M / (M - 1.0)
    mrm = (1.0 - torch.tensor(mom, dtype=F32)) * rm + torch.tensor(mom, dtype=F32) * fm32
    mrv = (1.0 - torch.tensor(mom, dtype=F32)) * rv + torch.tensor(mom, dtype=F32) * (fv * k).float()
    bmean, bvar, _ = R.finalize_bound((ps, pm), (bs, bm), M, R.C1_CHUNK)
    bounds = R.bn_affine_bound(y, gamma, beta, rm, rv, mom, bmean, bvar)
    worst = max(R.ratio(a, b, c) for a, b, c in zip((msc, msh, mrm, mrv), (sc, sh, nrm, nrv), bounds))
    _report(f"conv1_stats {case} -> bn_finalize", worst, 1)


# ---------------------------------------------------------------------------------------------------------------- linear3_gelu
@pytest.mark.parametrize("case", R.L3_CASES, ids=lambda c: f"m{c[0]}c{c[1]}-{R.dtype_name(c[2])}")
def test_linear3_gelu_reference_and_model(case):
    pts, w, b = R.l3_inputs(case)
    ref, bound = R.l3_exact(pts, w, b)
    v = F.linear(pts.double(), w.double(), b.double())
    _same(ref, 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0))), "erf-GELU")
    model = F.gelu(F.linear(pts, w, b)).to(case[2])
    _report(f"linear3_gelu {case[:2]} {R.dtype_name(case[2])}", R.ratio(model, ref, bound, case[2], slack=1.0), 1)


# ---------------------------------------------------------------------------------------------------------------- cls_max_pool
def _loop_max(col):
    """torch.max's rule written out: NaN is the maximum, the first of equals wins -> (value, 0-based index)"""
    best, bi = col[0], 0
    for i, v in enumerate(col[1:], 1):
        if math.isnan(best):
            break
        if math.isnan(v) or v > best:
            best, bi = v, i
    return best, bi


@pytest.mark.parametrize("nonfinite", [False, True], ids=["ties", "nonfinite"])
@pytest.mark.parametrize("T", R.CMP_T)
def test_cls_max_pool_reference_is_the_first_maximum_with_nan_as_maximum(T, nonfinite):
    for D in (5, 100):
        x = R.cmp_inputs(T, D, F32, nonfinite)
        out, idx = R.cmp_exact(x)
        assert torch.equal(out[:, :D], x[:, 0])
        assert idx.min() >= 1 and idx.max() <= T - 1
        for b in range(2):
            for d in range(D):
                v, i = _loop_max(x[b, 1:, d].tolist())
                assert idx[b, d] == i + 1 and (out[b, D + d] == v or (math.isnan(v) and math.isnan(out[b, D + d])))
        assert (idx[:, 2] == 1).all()                                          # the all-equal column
        if nonfinite:
            assert (idx[:, 3] == 1).all() and torch.isnan(out[:, D + 3]).all()                # all NaN: the first
            assert (idx[:, 4] == 1).all() and (out[:, D + 4] == -math.inf).all()              # all -inf: token 1
            if D > 64:
                assert (idx[:, 6] == min(2, T - 1)).all() and (idx[:, 8] == min(2, T - 1)).all() and (idx[:, 7] == T - 1).all()


# ----------------------------------------------------------------------------------------------------------------- pointmlp_pq
def test_pointmlp_pq_reference():
    case = R.PQ_CASES[2]
    B, N, S, C = case
    PQ, r, cidx, c0 = R.pq_inputs(case)
    P, Q = R.pq_ref(case, PQ, r, cidx, c0)
    for b, s, c in ((0, 0, 0), (2, 49, 35), (1, 7, 4)):
        a = b * N + int(cidx[b, s])
        assert P[a, c] == PQ[a, c] * r[b] and Q[b * S + s, c] == (c0[c] + PQ[a, C + c]) - P[a, c]
    n = (B * N + B * S) * (R.PQ_CASES[3][3] // 4) * 0 + (R.PQ_CASES[3][0] * (R.PQ_CASES[3][1] + R.PQ_CASES[3][2])) * (R.PQ_CASES[3][3] // 4)
    assert n > 4096 * 256, "the large case must send the grid-stride loop round again"


# ------------------------------------------------------------------------------------------------------------------- mutations
@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_breaks_the_criterion(mut):
    where, r = R.mutation_ratio(mut)
    print(f"MUTATION {mut} on {where}: error / bound {r:.3g}")
    assert r > 1.0, f"{mut} passes on {where}"


def test_half_ulp():
    for dtype, vals in ((BF16, (1.0, 1.5, 3.0, 0.007, 1e-30, 300.0)), (F16, (1.0, 1.5, 3.0, 0.007, 3e-6, 300.0))):
        for v in vals:
            t = torch.tensor([v]).to(dtype)
            up = torch.nextafter(t.float().to(dtype), torch.tensor([math.inf]).to(dtype)) if hasattr(torch, "nextafter") else None
            h = R.half_ulp(t, dtype).item()
            assert h > 0 and (up is None or abs((up.double() - t.double()).item() / 2 - h) <= 1e-300 + 1e-12 * h), (dtype, v)
    assert R.half_ulp(torch.zeros(1, dtype=BF16), BF16).item() == 2.0 ** -134
    assert R.half_ulp(torch.ones(1), F32).item() == 0.0
