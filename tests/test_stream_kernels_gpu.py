"""The streaming kernels between the GEMMs of the point encoders (Point-BERT's cls/max head and position embedding, PointNet2's
gather / pool / conv1 statistics, PointMLP's anchor statistics and residual rows; the two persistent PointNet2 branch kernels)
against the fp64 references and a-priori bounds of tests/stream_ref.py: every template instantiation, output format and
dispatch edge, at the smallest shapes that reach it.

Every output is written into a buffer with sentinel-filled guard rows behind it (and, where it is a column slice, sentinel columns
beside it), which must stay untouched; the kernels are therefore called through the library's C entry points with the ops module's
own argument helpers, except where the public wrapper is the thing under test (ops.cls_max_pool, ops.pointmlp_cloud_rstd,
ops.bn_finalize).  Every test prints one PARITY line with its largest error / bound ratio; a ratio above 1 is a kernel finding.
"""
import contextlib
import ctypes
import math

import pytest
import torch

import stream_ref as R

pytestmark = pytest.mark.gpu

F32, BF16, F16 = R.F32, R.BF16, R.F16
GUARD = 4                                   # guard rows behind every output
SENT16, SENT32, SENTI = -1234.0, 12345.0, -7777


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ppt_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _sent(dtype):
    return SENT32 if dtype == F32 else SENTI if dtype == torch.int32 else SENT16


def _guarded(rows, cols, dtype, side=0):
    """[rows + GUARD, side + cols + side] filled with the sentinel -> (the whole buffer, its [rows, cols] window)"""
    buf = torch.full((rows + GUARD, cols + 2 * side), _sent(dtype), dtype=dtype, device="cuda")
    return buf, buf[:rows, side:side + cols] if side else buf[:rows]


def _guards_untouched(*pairs):
    for buf, out in pairs:
        mask = torch.ones(buf.shape, dtype=torch.bool, device="cuda")
        side = (buf.shape[1] - out.shape[1]) // 2
        mask[:out.shape[0], side:side + out.shape[1]] = False
        assert (buf[mask] == _sent(buf.dtype)).all(), "memory around an output was written"
        assert not mask.all() and mask.any()


def _call(ops, name, *args):
    ops._lib.check(getattr(ops._lib.lib(), name)(*args), name)


def _parity(name, worst):
    print(f"PARITY stream {name}: largest error / bound {worst:.3f}")
    assert worst <= 1.0, name


# ------------------------------------------------------------------------------------------ group_anchor_stats and cloud_rstd
@pytest.mark.parametrize("dtype", [F32, BF16], ids=R.dtype_name)
@pytest.mark.parametrize("case", R.GAS_CASES, ids=str)
def test_group_anchor_stats(ops, case, dtype):
    B, Nsrc, S, K, D = case
    x, idx, anchor = R.gas_inputs(case, dtype)
    ref, bound = R.gas_exact(case, x, idx, anchor)
    buf, out = _guarded(B * S, 2, F32)
    xg, ig, ag = x.cuda(), idx.cuda(), anchor.cuda()           # (named: a pointer taken from a temporary outlives it)
    _call(ops, "ppt_group_anchor_stats", ops._p(xg), ops.dtype_code(dtype), ops._p(ig), ops._p(ag), B, Nsrc, S, K, D, ops._p(out), ops._stream())
    _guards_untouched((buf, out))
    st = out.view(B, S, 2)
    assert torch.equal(st, ops.group_anchor_stats(xg, ig, ag, Nsrc))
    worst = R.ratio(st.cpu(), ref, bound)
    n = float(S * K * D)
    r = ops.pointmlp_cloud_rstd(st.contiguous(), n)
    worst_r = R.ratio(r.cpu(), R.gas_rstd_exact(case, x, idx, anchor), R.rstd_bound(ref, n, bound))
    _parity(f"group_anchor_stats {case} {R.dtype_name(dtype)} (1 / std after it: {worst_r:.3f})", max(worst, worst_r))


@pytest.mark.parametrize("S", R.RSTD_S)
def test_cloud_rstd(ops, S):
    st, n = R.rstd_inputs(S)
    buf, out = _guarded(3, 1, F32)
    sg = st.cuda()
    _call(ops, "ppt_pointmlp_cloud_rstd", ops._p(sg), 3, S, n, ops._p(out), ops._stream())
    _guards_untouched((buf, out))
    r = out[:, 0].cpu()
    assert torch.equal(r, ops.pointmlp_cloud_rstd(sg, n).cpu())
    want0 = torch.tensor(1.0 / 1e-5, dtype=torch.float64).float()
    assert r[1] == want0 and r[2] == want0, "equal values: the variance clamps to 0"
    _parity(f"cloud_rstd S {S}", R.ratio(r, R.rstd_from_stats(st, n), R.rstd_bound(st, n)))


# ----------------------------------------------------------------------------------------------------------------- pointmlp_pq
@pytest.mark.parametrize("case", R.PQ_CASES, ids=str)
def test_pointmlp_pq_is_the_aten_expression_bit_for_bit(ops, case):
    B, N, S, C = case
    PQ, r, cidx, c0 = R.pq_inputs(case)
    Pw, Qw = R.pq_ref(case, PQ, r, cidx, c0)
    PQd, rd, cd, c0d = PQ.cuda(), r.cuda(), cidx.cuda(), c0.cuda()
    bp, P = _guarded(B * N, C, F32)
    bq, Q = _guarded(B * S, C, F32)
    _call(ops, "ppt_pointmlp_pq", ops._p(PQd), ops._p(rd), ops._p(cd), ops._p(c0d), ops._p(P), ops._p(Q), B, N, S, C, ops._stream())
    _guards_untouched((bp, P), (bq, Q))
    assert torch.equal(P.cpu(), Pw) and torch.equal(Q.cpu(), Qw), "against the fp32 expression on the CPU"
    Pg = (PQd[:, :C].reshape(B, N, C) * rd.view(B, 1, 1)).reshape(B * N, C)
    a = (torch.arange(B, device="cuda").view(B, 1) * N + cd).view(-1)
    assert torch.equal(P, Pg) and torch.equal(Q, (c0d.view(1, C) + PQd[:, C:][a] - Pg[a])), "against the ATen launches it replaces"
    P2, Q2 = ops.pointmlp_pq(PQd, rd, cd, c0d, B, N)
    assert torch.equal(P2, P) and torch.equal(Q2, Q)
    print(f"PARITY stream pointmlp_pq {case}: equal bits")


@pytest.mark.parametrize("C", [6, 37])
def test_pointmlp_pq_refuses_channels_that_are_no_multiple_of_four(ops, C):
    B, N, S = 2, 10, 3
    PQ, r, cidx, c0 = R.pq_inputs((B, N, S, C))
    bp, P = _guarded(B * N, C, F32)
    bq, Q = _guarded(B * S, C, F32)
    PQd, rd, cd, c0d = PQ.cuda(), r.cuda(), cidx.cuda(), c0.cuda()
    code = ops._lib.lib().ppt_pointmlp_pq(ops._p(PQd), ops._p(rd), ops._p(cd), ops._p(c0d), ops._p(P), ops._p(Q), B, N, S, C, ops._stream())
    torch.cuda.synchronize()
    assert code != 0
    assert (bp == SENT32).all() and (bq == SENT32).all(), "refused, not computed"
    with pytest.raises(RuntimeError):
        ops.pointmlp_pq(PQd, rd, cd, c0d, B, N)


# ------------------------------------------------------------------------------------------------------------------ gather_add
@pytest.mark.parametrize("stats", [True, False], ids=["stats", "nostats"])
@pytest.mark.parametrize("y_dtype", [F32, BF16, F16], ids=R.dtype_name)
@pytest.mark.parametrize("case", R.GA_CASES, ids=str)
def test_gather_add(ops, case, y_dtype, stats):
    B, Nsrc, S, K, C = case
    M, chunks = B * S * K, -(-B * S * K // 32)
    P, Q, idx = R.ga_inputs(case)
    by, y = _guarded(M, C, y_dtype)
    bs, ps = _guarded(chunks, C, F32)
    bm, pm = _guarded(chunks, C, F32)
    Pg, Qg, ig = P.cuda(), Q.cuda(), idx.cuda()
    _call(ops, "ppt_gather_add", ops._p(Pg), ops.dtype_code(F32), ops._p(Qg), ops._p(ig), B, Nsrc, S, K, C, ops._p(y),
          ops.dtype_code(y_dtype), ops._p(ps) if stats else None, ops._p(pm) if stats else None, ops._stream())
    _guards_untouched((by, y))
    assert torch.equal(y.cpu(), R.ga_y(case, P, Q, idx, y_dtype)), "y is one IEEE addition, cast once"
    y2, st2 = ops.gather_add(Pg, Qg, ig, Nsrc, y_dtype, want_stats=stats)
    assert torch.equal(y2, y)
    if not stats:
        assert st2 is None and (bs == SENT32).all() and (bm == SENT32).all()
        print(f"PARITY stream gather_add {case} {R.dtype_name(y_dtype)} without statistics: equal bits")
        return
    _guards_untouched((bs, ps), (bm, pm))
    assert torch.equal(st2[0], ps) and torch.equal(st2[1], pm)
    (rs, rm), (bds, bdm), v = R.ga_exact(case, P, Q, idx)
    worst = max(R.ratio(ps.cpu(), rs, bds), R.ratio(pm.cpu(), rm, bdm))
    # bn_finalize on the partials against the fp64 mean and biased variance of all M rows.  It hands out no variance: with gamma 1,
    # beta 0 its moments are (mean, rstd = 1 / sqrtf(var + eps)), and rstd is held to the variance's bound propagated through that map.
    ones, zeros = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    _, _, mean, rstd = ops.bn_finalize(ones, zeros, True, partials=(ps.contiguous(), pm.contiguous()), rows_per_partial=32, count=M,
                                       update_running=False, want_moments=True)
    em, ev = R.moments_exact(v)
    bmean, _, brstd = R.finalize_bound((rs, rm), (bds, bdm), M, R.GA_CHUNK)
    worst_f = max(R.ratio(mean.cpu(), em, bmean), R.ratio(rstd.cpu(), 1.0 / (ev + R.BN_EPS).sqrt(), brstd))
    _parity(f"gather_add {case} {R.dtype_name(y_dtype)} partials (bn_finalize after them: {worst_f:.3f})", max(worst, worst_f))


# ----------------------------------------------------------------------------------------------------------------- pool_finish
@pytest.mark.parametrize("case", R.PF_CASES, ids=lambda c: f"{R.dtype_name(c[0])}-{R.dtype_name(c[1])}-fold{c[2]}")
def test_pool_finish_into_a_column_slice(ops, case):
    pd, od, fold = case
    pmax, pmin, sc, sh = R.pf_inputs(case)
    ref, bound = R.pf_exact(case, pmax, pmin, sc, sh)
    buf, out = _guarded(R.PF_G, R.PF_C, od, side=3)
    assert out.stride(0) == R.PF_C + 6 and out.data_ptr() != buf.data_ptr()
    ops.pool_finish(pmax.cuda(), pmin.cuda(), fold, sc.cuda(), sh.cuda(), out)
    _guards_untouched((buf, out))
    got = out.cpu()
    assert torch.equal(got[:, 0].double(), ref[:, 0]), "scale exactly 0: relu(shift)"
    _parity(f"pool_finish {R.dtype_name(pd)} -> {R.dtype_name(od)} fold {fold}", R.ratio(got, ref, bound, od))


# ------------------------------------------------------------------------------------------------------------ bn_res_act_rows
@pytest.mark.parametrize("cid", [c[0] for c in R.BRA_CASES])
def test_bn_res_act_rows(ops, cid):
    case = R.BRA_BY_ID[cid]
    _, (M, C, pool), xd, rd, yd, aff, mis = case
    x, res, sc, sh, rs, rh = R.bra_inputs(case)
    ref, bound = R.bra_exact(case, x, res, sc, sh, rs, rh)
    xg = x.cuda()
    if mis:                                                   # one element behind a 16-byte boundary: the scalar kernel although C % 8 == 0
        flat = torch.empty(M * C + 8, dtype=xd, device="cuda")
        xg = flat[1:1 + M * C].view(M, C)
        xg.copy_(x)
        assert flat.data_ptr() % 16 == 0 and xg.data_ptr() % 16 == xg.element_size() and xg.is_contiguous()
    by, y = _guarded(M // pool, C, yd)
    args = [t.cuda() for t in (res, sc, sh, rs, rh)]
    _call(ops, "ppt_bn_res_act_rows", ops._p(xg), ops.dtype_code(xd), ops._p(args[0]), ops.dtype_code(rd), M, C, pool, ops._p(args[1]), ops._p(args[2]),
          ops._p(args[3]) if aff else None, ops._p(args[4]) if aff else None, ops._p(y), ops.dtype_code(yd), ops._stream())
    _guards_untouched((by, y))
    y2 = ops.bn_res_act_rows(xg, args[0], args[1], args[2], yd, pool=pool, res_affine=(args[3], args[4]) if aff else None)
    assert torch.equal(y2, y)
    got = y.cpu()
    assert (got[0, 1] == 0).all() and ref[0, 1] == 0, "every pre-activation of the group negative: exactly 0"
    _parity("bn_res_act_rows " + cid, R.ratio(got, ref, bound, yd))


# ----------------------------------------------------------------------------------------------- conv1_stats and its bn_finalize
@pytest.mark.parametrize("case", R.C1_CASES, ids=str)
def test_conv1_stats_and_bn_finalize(ops, case):
    M, C = case
    pts, w1, b1 = R.c1_inputs(case)
    (rs, rm), (bds, bdm), y = R.c1_exact(case, pts, w1, b1)
    P = -(-M // R.C1_CHUNK)
    bs, ps = _guarded(P, C, F32)
    bm, pm = _guarded(P, C, F32)
    n = ctypes.c_int(0)
    pg, wg, bg = pts.cuda(), w1.cuda(), b1.cuda()
    _call(ops, "ppt_conv1_stats", ops._p(pg), M, ops._p(wg), ops._p(bg), C, ops._p(ps), ops._p(pm), ctypes.byref(n), ops._stream())
    _guards_untouched((bs, ps), (bm, pm))
    ps2, pm2, rows = ops.conv1_stats(pg, wg, bg)
    assert n.value == P and rows == R.C1_CHUNK and torch.equal(ps2, ps) and torch.equal(pm2, pm)
    worst = max(R.ratio(ps.cpu(), rs, bds), R.ratio(pm.cpu(), rm, bdm))
    g = torch.Generator().manual_seed(M + C)
    gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    rmean, rvar = torch.randn(C, generator=g), 1.0 + torch.rand(C, generator=g)
    rmean_d, rvar_d, nbt = rmean.cuda(), rvar.cuda(), torch.zeros(1, dtype=torch.int64, device="cuda")
    sc, sh = ops.bn_finalize(gamma.cuda(), beta.cuda(), True, partials=(ps.contiguous(), pm.contiguous()), rows_per_partial=rows, count=M,
                             running_mean=rmean_d, running_var=rvar_d, num_batches_tracked=nbt, eps=R.BN_EPS, momentum=R.BN_MOM)
    assert nbt.item() == 1
    mom = float(torch.tensor(R.BN_MOM, dtype=F32))            # the fp32 momentum the library is handed
    want = R.bn_affine_exact(y, gamma, beta, rmean, rvar, mom)
    bmean, bvar, _ = R.finalize_bound((rs, rm), (bds, bdm), M, R.C1_CHUNK)
    bounds = R.bn_affine_bound(y, gamma, beta, rmean, rvar, mom, bmean, bvar)
    worst_f = max(R.ratio(a.cpu(), b, c) for a, b, c in zip((sc, sh, rmean_d, rvar_d), want, bounds))
    _parity(f"conv1_stats {case} partials (scale / shift / running statistics after them: {worst_f:.3f})", max(worst, worst_f))


# ---------------------------------------------------------------------------------------------------------------- linear3_gelu
@pytest.mark.parametrize("case", R.L3_CASES, ids=lambda c: f"m{c[0]}c{c[1]}-{R.dtype_name(c[2])}")
def test_linear3_gelu(ops, case):
    M, C, yd = case
    pts, w, b = R.l3_inputs(case)
    ref, bound = R.l3_exact(pts, w, b)
    by, y = _guarded(M, C, yd)
    pg, wg, bg = pts.cuda(), w.cuda(), b.cuda()
    _call(ops, "ppt_linear3_gelu", ops._p(pg), M, ops._p(wg), ops._p(bg), C, ops._p(y), ops.dtype_code(yd), ops._stream())
    _guards_untouched((by, y))
    assert torch.equal(ops.linear3_gelu(pg, wg, bg, yd), y)
    _parity(f"linear3_gelu {(M, C)} {R.dtype_name(yd)}", R.ratio(y.cpu(), ref, bound, yd, slack=1.0))


# ---------------------------------------------------------------------------------------------------------------- cls_max_pool
def _cls_max_pool(ops, x, want_argmax):
    """ops.cls_max_pool, and the same launch into guarded buffers: equal bits"""
    B, T, D = x.shape
    xg = x.cuda()
    out, am = ops.cls_max_pool(xg, want_argmax=want_argmax)
    bo, o = _guarded(B, 2 * D, F32)
    ba, a = _guarded(B, D, torch.int32)
    _call(ops, "ppt_cls_max_pool", ops._p(xg), ops.dtype_code(x.dtype), B, T, D, ops._p(o), ops._p(a) if want_argmax else None, ops._stream())
    _guards_untouched((bo, o))
    assert torch.equal(o, out) or (torch.isnan(o) == torch.isnan(out)).all() and torch.equal(torch.nan_to_num(o), torch.nan_to_num(out))
    if want_argmax:
        _guards_untouched((ba, a))
        assert torch.equal(a, am)
    else:
        assert am is None and (ba == SENTI).all()
    return out.cpu(), None if am is None else am.cpu()


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=R.dtype_name)
@pytest.mark.parametrize("T", R.CMP_T)
def test_cls_max_pool_values_and_first_maximum(ops, T, dtype):
    for D in R.CMP_D:
        x = R.cmp_inputs(T, D, dtype)
        want, widx = R.cmp_exact(x)
        for want_argmax in (True, False):
            out, am = _cls_max_pool(ops, x, want_argmax)
            assert torch.equal(out, want), (D, want_argmax)
            if want_argmax:
                assert torch.equal(am, widx), D
                assert (am[:, 2] == 1).all()                                    # the all-equal column
    print(f"PARITY stream cls_max_pool T {T} {R.dtype_name(dtype)}: values and indices equal torch's")


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=R.dtype_name)
@pytest.mark.parametrize("T", R.CMP_T)
def test_cls_max_pool_nan_and_minus_infinity_columns(ops, T, dtype):
    """Columns whose tokens 1 .. T-1 are all NaN or all -inf, one NaN among finite values, NaN only in a later wave's tokens: value and
    index are torch's (NaN is the maximum, the first wins; all -inf: token 1), and every index is a token, 1 <= index <= T - 1.  Only
    the kernel's own output is looked at: nothing is scattered with these indices."""
    for D in (5, 100):
        x = R.cmp_inputs(T, D, dtype, nonfinite=True)
        want, widx = R.cmp_exact(x)
        out, am = _cls_max_pool(ops, x, True)
        assert am.min().item() >= 1 and am.max().item() <= T - 1, f"D {D}: an index that is no token ({am.min().item()} .. {am.max().item()})"
        assert torch.equal(am, widx), D
        assert torch.allclose(out, want, rtol=0.0, atol=0.0, equal_nan=True), D
        out2, _ = _cls_max_pool(ops, x, False)
        assert torch.allclose(out2, want, rtol=0.0, atol=0.0, equal_nan=True), D
    print(f"PARITY stream cls_max_pool non-finite columns T {T} {R.dtype_name(dtype)}: values and indices equal torch's")


# ----------------------------------------------------------------------------------------------- conv12_stats (csrc/mpn1.hip)
C12_FORMS = ((32, 32), (64, 64), (64, 96), (64, 128), (128, 128))          # (C1, N)
_C12 = {}


def _c12_case(ops, form, tiles, bias):
    """operands of `tiles` 32-row tiles and the ops.gemm(A_CONV1) reference, computed once and never written again"""
    key = (form, tiles, bias)
    if key not in _C12:
        C1, N = form
        g = torch.Generator(device="cuda").manual_seed(C1 + N + tiles)
        M = 32 * tiles
        c = {"M": M, "form": form}
        c["pts"] = torch.randn(M, 3, device="cuda", generator=g) * 0.3
        c["w1"] = torch.randn(C1, 3, device="cuda", generator=g)
        c["b1"] = torch.randn(C1, device="cuda", generator=g) * 0.1
        c["sc"] = 1.0 + 0.1 * torch.randn(C1, device="cuda", generator=g)
        c["sh"] = 0.1 * torch.randn(C1, device="cuda", generator=g)
        c["w2"] = (torch.randn(N, C1, device="cuda", generator=g) / C1 ** 0.5).to(BF16)
        c["b2"] = torch.randn(N, device="cuda", generator=g) * 0.1 if bias else None
        c["st_ref"] = (torch.empty((tiles, N), device="cuda"), torch.empty((tiles, N), device="cuda"))
        c["y_ref"] = ops.gemm(None, c["w2"], out_dtype=BF16, a_mode=ops.A_CONV1, pts=c["pts"], w1=c["w1"], b1=c["b1"], a_scale=c["sc"],
                              a_shift=c["sh"], bias=c["b2"], col_stats=c["st_ref"])
        _C12[key] = c
    return _C12[key]


def _c12_check(ops, form, tiles, bias, share=100):
    c = _c12_case(ops, form, tiles, bias)
    C1, N = form
    by, y = _guarded(c["M"], N, BF16)
    bs, ps = _guarded(tiles, N, F32)
    bm, pm = _guarded(tiles, N, F32)
    with ops.persistent_occupancy(share) if share < 100 else contextlib.nullcontext():
        _call(ops, "ppt_conv12_stats_bf16", ops._p(c["pts"]), c["M"], ops._p(c["w1"]), ops._p(c["b1"]), ops._p(c["sc"]), ops._p(c["sh"]), C1, ops._p(c["w2"]),
              ops._p(c["b2"]), N, ops._p(y), ops._p(ps), ops._p(pm), ops._stream())
    _guards_untouched((by, y), (bs, ps), (bm, pm))
    assert torch.equal(y, c["y_ref"]), f"y, {tiles} tiles"
    rs, rm = c["st_ref"]
    assert (ps - rs).abs().max().item() < 1e-4 * max(1.0, rs.abs().max().item())
    assert (pm - rm).abs().max().item() < 1e-3 * max(1.0, rm.abs().max().item())
    return y, ps, pm


def _c12_grid(cus, share):
    return max(8, cus * 3 * share // 100)                     # mpn1_grid: three persistent workgroups per CU, at least 8


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("form", C12_FORMS, ids=str)
def test_conv12_stats_few_tiles_and_an_uneven_last_sweep(ops, cus, form, bias):
    """fewer tiles than the four waves of one workgroup, more, and 4 * grid + 1 on the smallest grid: one wave takes a second tile"""
    for tiles in (1, 2, 3, 5, 7):
        _c12_check(ops, form, tiles, bias)
    _c12_check(ops, form, 4 * _c12_grid(cus, 10) + 1, bias, share=10)
    print(f"PARITY stream conv12_stats {form} {'with' if bias else 'without'} bias: y equal bits, partials within 1e-4 / 1e-3")


@pytest.mark.parametrize("form", C12_FORMS, ids=str)
def test_conv12_stats_does_not_depend_on_the_grid(ops, cus, form):
    for tiles in (7, 4 * _c12_grid(cus, 10) + 1):
        outs = [_c12_check(ops, form, tiles, True, share) for share in (10, 30, 100)]
        for other in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(outs[0], other)), tiles


# -------------------------------------------------------------------------------------------- affine_conv_pool (csrc/affpool.hip)
AFP_FORMS = ((32, 64, 16, 4), (64, 128, 32, 2), (96, 128, 64, 2), (128, 256, 64, 1))      # (K, N, pool_rows, NWM = 4 / NWN)


@pytest.mark.parametrize("sliced", [False, True], ids=["contiguous", "lda=K+8"])
@pytest.mark.parametrize("form", AFP_FORMS, ids=str)
def test_affine_conv_pool_few_units_and_an_uneven_last_sweep(ops, cus, form, sliced):
    """units (32 rows; 64 where pool_rows is 64) below and above the NWM waves of a workgroup that each take one, and
    4 * CUs * NWM + 1: the grid is full and one wave takes a second unit"""
    K, N, pr, nwm = form
    rows = 64 if pr == 64 else 32
    worst = 0.0
    for units in (1, 2, 3, 5, 4 * cus * nwm + 1):
        g = torch.Generator(device="cuda").manual_seed(K + N + units)
        M = rows * units
        wide = torch.randn(M, K + 8, device="cuda", generator=g).to(BF16)
        A = wide[:, 8:] if sliced else wide[:, 8:].contiguous()
        assert A.stride(0) == (K + 8 if sliced else K) and A.data_ptr() % 16 == 0
        sc = 1.0 + 0.2 * torch.randn(K, device="cuda", generator=g)
        sh = 0.2 * torch.randn(K, device="cuda", generator=g)
        w = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(BF16)
        b = torch.randn(N, device="cuda", generator=g) * 0.1
        pairs = [_guarded(M // pr, N, F32), _guarded(M // pr, N, F32), _guarded(M // 32, N, F32), _guarded(M // 32, N, F32)]
        pmax, pmin, ps, pm = (p[1] for p in pairs)
        _call(ops, "ppt_affine_conv_pool_bf16", ops._p(A), A.stride(0), M, K, ops._p(sc), ops._p(sh), ops._p(w), ops._p(b), N, pr, ops._p(pmax), ops._p(pmin),
              ops._p(ps), ops._p(pm), ops._stream())
        _guards_untouched(*pairs)
        rmax, rmin = torch.empty((M // pr, N), device="cuda"), torch.empty((M // pr, N), device="cuda")
        rst = (torch.empty((M // 32, N), device="cuda"), torch.empty((M // 32, N), device="cuda"))
        Ac = A.contiguous()
        ops.gemm(Ac, w, a_mode=ops.A_AFFINE_RELU, a_scale=sc, a_shift=sh, bias=b, want_out=False, pool_max=rmax, pool_min=rmin, pool_rows=pr,
                 col_stats=rst)
        assert torch.equal(pmax, rmax) and torch.equal(pmin, rmin), f"{units} units"
        assert (ps - rst[0]).abs().max().item() < 1e-4 * max(1.0, rst[0].abs().max().item())
        assert (pm - rst[1]).abs().max().item() < 1e-3 * max(1.0, rst[1].abs().max().item())
        a = torch.relu(Ac.double() * sc.double() + sh.double()).to(BF16).double()
        v = (a @ w.double().t() + b.double()).view(M // pr, pr, N)
        tol = 2e-4 * max(1.0, v.abs().max().item())
        err = max((pmax.double() - v.amax(1)).abs().max().item(), (pmin.double() - v.amin(1)).abs().max().item())
        worst = max(worst, err / tol)
    _parity(f"affine_conv_pool {form[:3]} {'lda = K + 8' if sliced else 'contiguous'} max / min against fp64 (error / 2e-4 max|v|)", worst)
