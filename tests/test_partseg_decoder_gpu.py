"""GPU: the part-segmentation decoder's fused autograd nodes (ppt_amd/autograd.py: _FeaturePropagation, _DGCNNLayer,
_ConvBNReLURows) in their four precisions, train() and eval(), and the kernel forms only the 16-bit decoder reaches, against fp64
on the same operands (tests/decoder_ref.py; tests/test_decoder_ref_cpu.py checks those references and the criterion on the CPU).

Node tests: float32 and float32 + split16 are held to the bound of the two older module tests of tests/test_kernels_gpu.py
(maximum absolute error 2e-3 * max(1, max |exact|)); float16 and bfloat16 to decoder_ref.ratio <= CAP = 2 -- per output and per
group of 8 channels, ||node - exact|| <= 2 (||rounding model - exact|| + floor) -- with the rounding model at the gradient scale
the node picks (2^floor(log2 rows)).  Every run is repeated and must return the same bits.  Figures are printed (pytest -s) as
`PARITY <what>: <value> (bound <bound>)`.

Worst measured ratio per node, format and mode (MI355X, over this file's cases and all outputs; the bound is 2):
    feature propagation   float16  train 0.68   eval 0.68      bfloat16  train 0.85   eval 1.00
    DGCNN layer           float16        1.00                  bfloat16        1.00            (eval() = train(): GroupNorm)
    conv_bn_relu_rows     float16  train 0.63   eval 0.65      bfloat16  train 0.90   eval 0.98
1.00 is always a dbeta: a channel group where 16-bit operands move one ReLU / LeakyReLU decision of the rounding model away from
fp64's, which the kernels follow -- node error = model error.  Every other output stays at 0.5 - 0.7, as decoder_ref.rounded_tiled
does on the CPU.  Float32 and split16 use at most 1.2 % of their bound.
"""
import contextlib

import pytest
import torch

import decoder_ref as R

pytestmark = pytest.mark.gpu
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
PRECISIONS = ("float32", "split16", "float16", "bfloat16")
DTYPE = {"float32": F32, "split16": F32, "float16": F16, "bfloat16": BF16}
FP32_BOUND = 2e-3                                    # test_feature_propagation_... / test_dgcnn_layer_... of tests/test_kernels_gpu.py


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ppt_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def _precision(ops, prec):
    """the GEMM mode of `prec`: split16 switched on for its case only, and restored"""
    before = ops.split16_enabled()
    ops.set_split16(prec == "split16")
    try:
        yield DTYPE[prec]
    finally:
        ops.set_split16(before)


def _dev(t):
    return None if t is None else t.cuda()


def _load_bn(bn, lay):
    with torch.no_grad():
        bn.weight.copy_(lay.gamma); bn.bias.copy_(lay.beta); bn.running_mean.copy_(lay.rm); bn.running_var.copy_(lay.rv)
        bn.num_batches_tracked.zero_()


def _load_conv(conv, lay):
    with torch.no_grad():
        conv.weight.copy_(lay.W.view_as(conv.weight)); conv.bias.copy_(lay.b)


def _mlp_results(res, pairs, training, layers):
    for li, (conv, bn) in enumerate(pairs):
        res.update({f"W{li}": conv.weight.grad.reshape(conv.weight.shape[0], -1), f"b{li}": conv.bias.grad, f"g{li}": bn.weight.grad,
                    f"be{li}": bn.bias.grad})
        if training:
            res[f"rm{li}"], res[f"rv{li}"] = bn.running_mean.clone(), bn.running_var.clone()
            assert int(bn.num_batches_tracked) == 1
        else:                                        # eval(): the running statistics are read, never written
            assert torch.equal(bn.running_mean.cpu(), layers[li].rm) and torch.equal(bn.running_var.cpu(), layers[li].rv)
            assert int(bn.num_batches_tracked) == 0


def _run(ops, c, inp, T, training, announce_rows=None, generic=False):
    """one forward + backward of a case's node on fresh modules -> {output name: CPU tensor}, keys as decoder_ref's"""
    from ppt_amd import autograd as A, gradscale
    from ppt_amd.models.pointbert.pointnet2_utils import DGCNN_Propagation, PointNetFeaturePropagation
    ctx = gradscale.rows(announce_rows) if announce_rows else contextlib.nullcontext()
    dout = inp["dout"].cuda()
    res = {}
    if c.node == "fp":
        B, N, S, D1, D2, mlp = c.shape
        m = PointNetFeaturePropagation(in_channel=D1 + D2, mlp=list(mlp)).cuda()
        m.precision = T
        m.train(training)
        for conv, bn, lay in zip(m.mlp_convs, m.mlp_bns, inp["layers"]):
            _load_conv(conv, lay); _load_bn(bn, lay)
        p2 = inp["p2"].cuda().requires_grad_()
        with ctx:
            if generic:
                out = m.forward_rows(inp["xyz1"].cuda(), inp["xyz2"].cuda(), _dev(inp["p1"]), p2)
            else:
                out = A.feature_propagation(m, _dev(inp["p1"]), p2, inp["idx"].cuda(), inp["dist"].cuda(), T)
        out.backward(dout)
        res.update(out=out.detach(), dp2=p2.grad)
        _mlp_results(res, list(zip(m.mlp_convs, m.mlp_bns)), training, inp["layers"])
    elif c.node == "cbr":
        M, K, N = c.shape
        conv, bn = torch.nn.Conv1d(K, N, 1).cuda(), torch.nn.BatchNorm1d(N).cuda()
        _load_conv(conv, inp["layers"][0]); _load_bn(bn, inp["layers"][0])
        bn.train(training)
        x = inp["x"].cuda().requires_grad_()
        with ctx:
            out = A.conv_bn_relu_rows(x, conv, bn, training, T)
        out.backward(dout)
        assert x.grad.shape == (M, K)                # K columns, not the operand's padded Kp
        res.update(out=out.detach(), dx=x.grad)
        _mlp_results(res, [(conv, bn)], training, inp["layers"])
    else:
        layer = c.shape[0]
        m = DGCNN_Propagation(k=R.DG_K).cuda()
        m.precision = T
        m.train(training)
        seq = m.layer1 if layer == 1 else m.layer2
        with torch.no_grad():
            seq[0].weight.copy_(inp["W"].view_as(seq[0].weight)); seq[1].weight.copy_(inp["gamma"]); seq[1].bias.copy_(inp["beta"])
        x_k = inp["x_k"].cuda().requires_grad_()
        x_q = x_k if inp["x_q"] is None else inp["x_q"].cuda().requires_grad_()
        with ctx:
            if inp["x_q"] is None:                   # layer2 as the module calls it: one tensor is both operands
                coor = inp["coor"].cuda()
                idx, _ = ops.knn_group(coor, coor, R.DG_K, want_nbhd=False)
                assert torch.equal(idx.cpu(), inp["idx"])
                out = m._layer(seq, coor, x_k, coor, x_k)
            else:
                out = A.dgcnn_layer(x_k, x_q, seq[0], seq[1], inp["idx"].cuda(), 0.2, T)
        out.backward(dout)
        res.update(out=out.detach(), W=seq[0].weight.grad.reshape(seq[0].weight.shape[0], -1), g0=seq[1].weight.grad,
                   be0=seq[1].bias.grad, dx_k=x_k.grad)
        if inp["x_q"] is not None:
            res["dx_q"] = x_q.grad
    torch.cuda.synchronize()
    return {k: v.detach().float().cpu() for k, v in res.items()}


def _same_bits(a, b, errors, tag):
    for k in a:
        if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)):
            errors.append(f"{tag} {k}: a second run returned other bits")


def _check_fp32(got, ref, errors, tag, keys=None):
    worst = 0.0
    for k in (keys or ref):
        bound = FP32_BOUND * max(1.0, ref[k].abs().max().item())
        err = (got[k].double() - ref[k]).abs().max().item()
        worst = max(worst, err / bound)
        if not err < bound:
            errors.append(f"{tag} {k}: max |err| {err:.3e} >= {bound:.3e}")
    print(f"PARITY {tag} worst |err| / allowed: {worst:.4f} (bound 1: {FP32_BOUND} * max(1, max |exact|) per output)")


def _check_ratio(got, mod, ref, mag, errors, tag, skip=()):
    res = R.ratios(got, mod, ref, mag, skip=skip)
    print(f"PARITY {tag} ratios: " + " ".join(f"{k}={v[0]:.3f}@{v[1]}" for k, v in res.items()) + f" (bound {R.CAP})")
    for k, (q, ch) in res.items():
        if not q <= R.CAP:
            errors.append(f"{tag} {k}: ratio {q:.3f} > {R.CAP} in the channels from {ch}")
    return res


MODES = [pytest.param(True, id="train"), pytest.param(False, id="eval")]


def _node_case(ops, c, prec, training):
    inp = R.inputs(c)
    errors = []
    tag = f"{R.case_id(c)} {prec} {'train' if training else 'eval'}"
    with _precision(ops, prec) as T:
        got = _run(ops, c, inp, T, training)
        again = _run(ops, c, inp, T, training)
    _same_bits(got, again, errors, tag)
    if T == F32:
        ref, _ = R.exact_cached(c, training)
        assert set(got) == set(ref)
        _check_fp32(got, ref, errors, tag)
    else:
        ref, mag, mod = R.references(c, T, training, R.pow2_floor(R.rows(c)))
        assert set(got) == set(ref)
        _check_ratio(got, mod, ref, mag, errors, tag)
    if c.name == "tie":
        _check_tie(c, inp, got, T, errors, tag)
    assert not errors, "\n".join(errors)


def _check_tie(c, inp, got, T, errors, tag):
    """the twin source rows: every query that has both sends its gradient to the first (lower-index) one, in every channel; and the
    two rows' gradients together are exact's"""
    a, b = inp["dup"]
    ref, mag = R.exact_cached(c, True)
    everyone = R.model(c, R.Opt(ft=torch.float64, mut="tie_to_all"))["dx_k"]
    pair = lambda t: t[:, [a, b]]
    both = lambda t: t[:, a] + t[:, b]
    assert (pair(everyone) - pair(ref["dx_k"])).abs().max().item() > 100 * FP32_BOUND * max(1.0, ref["dx_k"].abs().max().item())
    if T == F32:
        _check_fp32({"twin rows": pair(got["dx_k"]), "sum of the twin rows": both(got["dx_k"])},
                    {"twin rows": pair(ref["dx_k"]), "sum of the twin rows": both(ref["dx_k"])}, errors, tag + " first maximiser")
    else:
        mod = R.references(c, T, True, R.pow2_floor(R.rows(c)))[2]
        _check_ratio({"twin rows": pair(got["dx_k"]), "sum of the twin rows": both(got["dx_k"])},
                     {"twin rows": pair(mod["dx_k"]), "sum of the twin rows": both(mod["dx_k"])},
                     {"twin rows": pair(ref["dx_k"]), "sum of the twin rows": both(ref["dx_k"])}, {}, errors, tag + " first maximiser")


FP_CASES = [c for c in R.CASES if c.node == "fp"]
DG_CASES = [c for c in R.CASES if c.node == "dg"]
CBR_CASES = [c for c in R.CASES if c.node == "cbr"]


@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("c", FP_CASES, ids=[R.case_id(c) for c in FP_CASES])
def test_feature_propagation_node_against_fp64(ops, c, prec, training):
    _node_case(ops, c, prec, training)


@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("c", DG_CASES, ids=[R.case_id(c) for c in DG_CASES])
def test_dgcnn_layer_node_against_fp64(ops, c, prec, training):
    """(GroupNorm has no eval form: eval() must give what train() gives)"""
    _node_case(ops, c, prec, training)


@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("c", CBR_CASES, ids=[R.case_id(c) for c in CBR_CASES])
def test_conv_bn_relu_rows_node_against_fp64(ops, c, prec, training):
    _node_case(ops, c, prec, training)


@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("prec", ["float32", "split16"])
@pytest.mark.parametrize("c", R.GENERIC, ids=[R.case_id(c) for c in R.GENERIC])
def test_feature_propagation_generic_path_against_fp64(ops, c, prec, training):
    """S == 1 and a three-layer mlp leave the fused node for _Linear + _BatchNormReLURows: the fp32 bound"""
    inp = dict(R.inputs(c))
    if c.shape[2] > 1:                               # forward_rows searches the neighbours itself: the reference gets what it found
        idx, _, d = ops.knn_group(inp["xyz2"].cuda(), inp["xyz1"].cuda(), 3, want_nbhd=False, want_dist=True)
        assert torch.equal(idx.cpu(), inp["idx"]) and (d.cpu() - inp["dist"]).abs().max().item() < 1e-5
        inp["dist"] = d.cpu()
    errors = []
    tag = f"{R.case_id(c)} {prec} {'train' if training else 'eval'} (generic path)"
    with _precision(ops, prec) as T:
        got = _run(ops, c, inp, T, training, generic=True)
        again = _run(ops, c, inp, T, training, generic=True)
    _same_bits(got, again, errors, tag)
    ref, _ = R.exact(c, training, inp)
    assert set(got) == set(ref)
    _check_fp32(got, ref, errors, tag)
    assert not errors, "\n".join(errors)


def test_gradient_scale_keeps_a_tiny_float16_gradient(ops, monkeypatch):
    """dout * 2^-20 through the first feature-propagation case in float16: inside gradscale.rows(B * N) and with the node's own
    default the result stays within the cap of the rounding model at that scale and no gradient is flushed to zero; with the
    scale policy off the same input loses the gradient, and this test sees it (ratio above the cap)"""
    from ppt_amd import gradscale
    c = R.BY_ID["fp-m640"]
    inp = dict(R.inputs(c))
    inp["dout"] = inp["dout"] * 2.0 ** -20
    S = R.pow2_floor(R.rows(c))
    ref, mag = R.exact(c, True, inp)
    mod = R.rounded(c, F16, True, S=S, inp=inp)
    errors = []
    for announce in (R.rows(c), None):
        tag = f"fp-m640 float16 train dout * 2^-20, " + ("inside gradscale.rows" if announce else "the node's default scale")
        got = _run(ops, c, inp, F16, True, announce_rows=announce)
        _check_ratio(got, mod, ref, mag, errors, tag)
        for k in ref:
            if k not in R.ZERO_IN_TRAIN and bool(((got[k] == 0) & (ref[k] != 0)).any()):
                errors.append(f"{tag} {k}: zero where exact is not")
    assert not errors, "\n".join(errors)
    monkeypatch.setattr(gradscale, "POLICY", "off")
    got = _run(ops, c, inp, F16, True)
    lost = []
    res = _check_ratio(got, mod, ref, mag, lost, "fp-m640 float16 train dout * 2^-20, scale policy off (must exceed the cap)")
    assert max(v[0] for v in res.values()) > R.CAP, res


# ------------------------------------------------------------------------------------------------ kernel forms of the 16-bit decoder
def _offset_copy(t, elems):
    """a contiguous copy of t that starts `elems` elements into its buffer"""
    buf = torch.empty(t.numel() + elems, dtype=t.dtype, device=t.device)
    v = buf[elems:].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("T", [F16, BF16], ids=R.dtype_name)
@pytest.mark.parametrize("M,D,pad,off", [(777, 136, 0, 0), (515, 128, 8, 0), (1000, 36, 4, 0), (5, 8, 0, 0), (515, 128, 0, 4)])
def test_col_sums_16bit_matches_fp64(ops, T, M, D, pad, off):
    """bias gradients of the 16-bit decoder: column sums of an f16 / bf16 matrix against fp64 on the stored values -- the
    eight-per-thread kernel (D % 8 == 0, 16-byte aligned, row stride wider than D allowed), the scalar one (D % 8 != 0; a base 8
    bytes into its buffer), the bound of test_col_sums_matches_torch, and the same bits twice"""
    g = torch.Generator(device="cuda").manual_seed(M + D)
    full = torch.randn(M, D + pad, device="cuda", generator=g).to(T)
    if off:
        full = _offset_copy(full, off)
        assert full.data_ptr() % 16 == 2 * off
    x = full[:, :D]
    out = ops.col_sums(x)
    ref = x.double().sum(0)
    err = (out.double() - ref).abs().max().item()
    bound = 1e-5 * max(1.0, float(M) ** 0.5)
    print(f"PARITY col_sums {R.dtype_name(T)} {M}x{D} pad {pad} offset {off}: {err:.3e} (bound {bound:.3e})")
    assert out.shape == (D,) and out.dtype == F32 and err < bound
    assert torch.equal(out, ops.col_sums(x))


@pytest.mark.parametrize("batch_stats", [1, 0])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("M,C,off", [(330, 48, 0), (66, 30, 0), (130, 68, 0), (330, 48, 1)])
def test_bn_rows_backward_forms_match_fp64(ops, M, C, off, relu, batch_stats):
    """ppt_bn_rows_bwd_reduce / _apply in the forms of the 16-bit decoder: with and without the ReLU mask, batch statistics
    (train) or not (eval), the fp32 and the half output together and the half output alone (want_dx = False), f16 and bf16;
    C % 4 != 0 and a base 4 bytes into its buffer leave the float4 reduction.  Against the fp64 formula on the same operands at the
    bounds of test_batch_norm_relu_rows_matches_torch; pre-activations are kept 1e-3 away from zero."""
    g = torch.Generator().manual_seed(M * 100 + C + off)
    x = torch.randn(M, C, generator=g) * 2 + torch.randn(C, generator=g) * 3
    dy = torch.randn(M, C, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    if batch_stats:
        mean, var = x.mean(0), x.var(0, unbiased=False)
    else:
        mean, var = x.mean(0) + 0.3 * torch.randn(C, generator=g), x.var(0, unbiased=False) * (0.5 + torch.rand(C, generator=g))
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    sc = gamma * rstd
    sh = beta - mean * sc
    near = (x * sc + sh).abs() < 2e-3                # moved away from the ReLU edge; the statistics are operands and stay as they are
    assert near.float().mean().item() <= 0.01
    x = torch.where(near, x + 8e-3 / sc, x)
    assert ((x.double() * sc.double() + sh.double()).abs() >= 1e-3).all()
    xd, dyd, scd, shd, md, rd = (t.double() for t in (x, dy, sc, sh, mean, rstd))
    gd = dyd * (xd * scd + shd > 0) if relu else dyd
    xhat = (xd - md) * rd
    sg, sgx = gd.sum(0), (gd * xhat).sum(0)
    dx_ref = scd * (gd - sg / M - xhat * sgx / M) if batch_stats else scd * gd
    xg, dyg = (_offset_copy(t.cuda(), off) for t in (x, dy))
    assert xg.data_ptr() % 16 == 4 * off
    a = [t.cuda() for t in (sc, sh, mean, rstd)]
    tag = f"bn_rows_backward {M}x{C} offset {off} relu {relu} batch_stats {batch_stats}"
    for half in (F16, BF16):
        dx, dgamma, dbeta, dxh = ops.bn_rows_backward(dyg, xg, *a, relu, batch_stats, want_dx=True, want_bf16=True, half_dtype=half)
        none, dgamma2, dbeta2, dxh2 = ops.bn_rows_backward(dyg, xg, *a, relu, batch_stats, want_dx=False, want_bf16=True, half_dtype=half)
        torch.cuda.synchronize()
        e_dx = (dx.double().cpu() - dx_ref).abs().max().item()
        e_g, e_b = (dgamma.double().cpu() - sgx).abs().max().item(), (dbeta.double().cpu() - sg).abs().max().item()
        print(f"PARITY {tag} {R.dtype_name(half)}: dx {e_dx:.3e} dgamma {e_g:.3e} dbeta {e_b:.3e} (bounds rtol 1e-3 + atol 2e-4 / 1e-2 / 1e-2)")
        assert torch.allclose(dx.double().cpu(), dx_ref, rtol=1e-3, atol=2e-4)
        assert torch.allclose(dgamma.double().cpu(), sgx, rtol=1e-3, atol=1e-2)
        assert torch.allclose(dbeta.double().cpu(), sg, rtol=1e-3, atol=1e-2)
        assert dxh.dtype == half and torch.equal(dxh.view(torch.int16), dx.to(half).view(torch.int16))
        assert none is None and torch.equal(dxh2.view(torch.int16), dxh.view(torch.int16))
        assert torch.equal(dgamma2, dgamma) and torch.equal(dbeta2, dbeta)


@pytest.mark.parametrize("T", [F16, BF16], ids=R.dtype_name)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_bn_act_rows_into_16bit_is_the_fp32_result_cast(ops, T, masked):
    g = torch.Generator(device="cuda").manual_seed(7)
    M, C = 333, 48
    x = torch.randn(M, C, device="cuda", generator=g) * 3
    sc, sh = 1 + 0.2 * torch.randn(C, device="cuda", generator=g), torch.randn(C, device="cuda", generator=g)
    mask = (torch.rand(M, C, device="cuda", generator=g) >= 0.5).float() * 2.0 if masked else None
    y32 = ops.bn_act_rows(x, sc, sh, F32, mask=mask)
    y16 = ops.bn_act_rows(x, sc, sh, T, mask=mask)
    ref = torch.relu(x.double() * sc.double() + sh.double()) * (mask.double() if masked else 1.0)
    err = (y32.double() - ref).abs().max().item()
    print(f"PARITY bn_act_rows {R.dtype_name(T)} {'masked' if masked else 'plain'} fp32 result: {err:.3e} (bound 1e-5)")
    assert err < 1e-5 and y16.dtype == T
    assert torch.equal(y16.view(torch.int16), y32.to(T).view(torch.int16))


def _offset_rows(M, C, ratio, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, C, generator=g) + ratio).float()


@pytest.mark.parametrize("ratio", [10.0, 100.0])
@pytest.mark.parametrize("M,C", [(66, 30), (330, 48)])
def test_rows_stats_under_a_common_offset(ops, M, C, ratio):
    """ops.rows_stats -> ops.bn_finalize -> ops.bn_act_rows with |mean| / std of 10 and 100 (Welford chunk partials merged in fp64):
    rstd and the shift at the bounds of test_bn_finalize_many_partials, the output at test_batch_norm_relu_rows_matches_torch's"""
    x = _offset_rows(M, C, ratio, M + C)
    xd = x.double()
    gamma, beta = torch.ones(C), 0.25 * torch.ones(C)
    xg = x.cuda()
    parts, rpp = ops.rows_stats(xg)
    sc, sh, mean, rstd = ops.bn_finalize(gamma.cuda(), beta.cuda(), True, partials=parts, rows_per_partial=rpp, count=M, want_moments=True,
                                         update_running=False)
    y = ops.bn_act_rows(xg, sc, sh, F32)
    rstd_ref = 1.0 / torch.sqrt(xd.var(0, unbiased=False) + 1e-5)
    y_ref = torch.relu((xd - xd.mean(0)) * rstd_ref + 0.25)
    print(f"PARITY rows_stats {M}x{C} |mean|/std {ratio:g}: rstd rel {((rstd.double().cpu() - rstd_ref).abs() / rstd_ref).max().item():.3e} "
          f"(bound 2e-5), out {(y.double().cpu() - y_ref).abs().max().item():.3e} (bound 1e-4 + 1e-4 |ref|)")
    assert torch.allclose(rstd.double().cpu(), rstd_ref, rtol=2e-5, atol=1e-6)
    assert torch.allclose(sc.double().cpu(), rstd_ref, rtol=2e-5, atol=1e-6)
    assert torch.allclose(sh.double().cpu(), 0.25 - xd.mean(0) * rstd_ref, rtol=2e-5, atol=2e-4)
    assert torch.allclose(y.double().cpu(), y_ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("ratio", [10.0, 100.0])
def test_group_norm_statistics_under_a_common_offset(ops, ratio):
    """ops.gn_lrelu_max_forward on y = offset + noise, |mean| / std of 10 and 100: rstd and the output against fp64 at the bound of
    test_group_norm_lrelu_max_matches_torch (2e-4 * max(1, max |ref|)).  Before the chunk sums were centred (csrc/groupnorm.hip,
    gn_stats_kernel: fp32 sum and sum of squares per channel, S1 / n - mean^2) a ratio of 100 missed it."""
    B, Q, K, C = 1, 33, 4, 64
    y = _offset_rows(B * Q * K, C, ratio, 33).view(B, Q, K, C)
    g = torch.Generator().manual_seed(5)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    out, arg, mean, rstd = ops.gn_lrelu_max_forward(y.cuda(), gamma.cuda(), beta.cuda(), R.GN_GROUPS, R.GN_EPS, R.SLOPE)
    yd = y.double()
    z = torch.nn.functional.group_norm(yd.permute(0, 3, 1, 2), R.GN_GROUPS, gamma.double(), beta.double(), R.GN_EPS)
    ref = torch.nn.functional.leaky_relu(z, R.SLOPE).max(dim=-1)[0].permute(0, 2, 1)
    yg = yd.view(B, Q * K, R.GN_GROUPS, C // R.GN_GROUPS)
    rstd_ref = 1.0 / torch.sqrt(yg.var((1, 3), unbiased=False) + R.GN_EPS)
    e_r = (rstd.double().cpu() - rstd_ref).abs().max().item()
    e_o = (out.double().cpu() - ref).abs().max().item()
    b_r, b_o = 2e-4 * max(1.0, rstd_ref.abs().max().item()), 2e-4 * max(1.0, ref.abs().max().item())
    print(f"PARITY gn_lrelu_max_forward |mean|/std {ratio:g}: rstd {e_r:.3e} (bound {b_r:.3e}), out {e_o:.3e} (bound {b_o:.3e})")
    assert e_r < b_r and e_o < b_o
