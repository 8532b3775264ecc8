"""CPU: the references and the criterion of tests/decoder_ref.py checked without a GPU, on the cases and inputs of
tests/test_partseg_decoder_gpu.py.

  * `exact` is the reference formulation: it agrees with torch.nn modules run in fp64 (Conv1d + BatchNorm1d + ReLU; Conv2d +
    GroupNorm + LeakyReLU + max) to 1e-10, in train() and eval(); and the written-out backward of the rounding model, run in
    fp64 without casts, agrees with exact's autograd.
  * A correct result in another summation order (rounded_tiled) passes every case, both formats and both modes with room to
    spare: maximum ratio <= CAP / 2.
  * Every model broken on purpose (decoder_ref.MUTATIONS) fails, with a ratio above CAP in at least one output, on a case where
    it can act.  Where a mutation cannot act, and so is NOT seen (this is a property of the mathematics, not of the criterion):
      - bn_train_terms_dropped / bn_eval_terms_kept change nothing in `out` or the running statistics (forward only);
      - db_unmasked in train(): the bias in front of a BatchNorm has gradient zero whatever the mask (the BatchNorm input gradient
        sums to zero per channel), so it is tested in eval(), where db is a real gradient;
      - last_quad on db in train(): the same zero; dgamma and dbeta show it;
      - unscale_missing needs S != 1 (a bare fp32 stage has S = 1 and nothing to forget);
      - dgamma_from_rounded with gradients in the normal range of T adds one rounding of g to a sum whose other factor xhat
        already carries the 16-bit error of y: its ratio stays below CAP (test_dgamma_from_the_rounded_gradient_..., figures
        printed).  It is seen where it bites, in float16 with a gradient of 2^-20 and no gradient scale, where T(g) underflows.
  * The conditioning holds for every case and at most 1 % of the input values were nudged.
"""
import pytest
import torch

import decoder_ref as R

F16, BF16 = R.F16, R.BF16
CASE_IDS = [R.case_id(c) for c in R.CASES]
MODES = {"fp": (True, False), "cbr": (True, False), "dg": (True,)}          # (GroupNorm has no eval form)


def _close(a, b, tol, what):
    err = (a.double() - b.double()).abs().max().item()
    assert err <= tol * max(1.0, b.abs().max().item()), f"{what}: {err:.3e}"


# ------------------------------------------------------------------------------------------------ exact is the formulation
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("cid", ["fp-m640", "fp-nop1", "cbr-m330", "fp-mlp3", "fp-s1"])
def test_exact_conv_bn_relu_is_the_torch_modules(cid, training):
    c = R.BY_ID[cid]
    inp = R.inputs(c)
    ref, _ = R.exact(c, training)
    convs, bns = [], []
    for lay in inp["layers"]:
        conv, bn = torch.nn.Conv1d(lay.W.shape[1], lay.W.shape[0], 1).double(), torch.nn.BatchNorm1d(lay.W.shape[0]).double()
        with torch.no_grad():
            conv.weight.copy_(lay.W[:, :, None]); conv.bias.copy_(lay.b); bn.weight.copy_(lay.gamma); bn.bias.copy_(lay.beta)
            bn.running_mean.copy_(lay.rm); bn.running_var.copy_(lay.rv)
        conv.train(training); bn.train(training)
        convs.append(conv); bns.append(bn)
    if c.node == "cbr":
        leaf = inp["x"].double().requires_grad_()
        x = leaf.t()[None]                                                        # [1, K, M]
    else:                                                                         # pointnet2_utils.py:333-358, channel-first
        leaf = inp["p2"].double().requires_grad_()
        B, N, k = inp["idx"].shape
        if inp["p2"].shape[1] == 1:
            interp = leaf.repeat(1, N, 1)
        else:
            recip = 1.0 / (inp["dist"].double() + 1e-8)
            w = recip / recip.sum(dim=2, keepdim=True)
            interp = (leaf[torch.arange(B)[:, None, None], inp["idx"]] * w.unsqueeze(-1)).sum(dim=2)
        x = (interp if inp["p1"] is None else torch.cat([inp["p1"].double(), interp], dim=-1)).permute(0, 2, 1)
    for conv, bn in zip(convs, bns):
        x = torch.relu(bn(conv(x)))
    out = x.permute(0, 2, 1)
    out = out[0] if c.node == "cbr" else out
    out.backward(inp["dout"].double())
    _close(ref["out"], out.detach(), 1e-10, "out")
    _close(ref["dx" if c.node == "cbr" else "dp2"], leaf.grad, 1e-10, "input gradient")
    for li, (conv, bn) in enumerate(zip(convs, bns)):
        for k, t in ((f"W{li}", conv.weight.grad[:, :, 0]), (f"b{li}", conv.bias.grad), (f"g{li}", bn.weight.grad), (f"be{li}", bn.bias.grad)):
            _close(ref[k], t, 1e-10, k)
        if training:
            _close(ref[f"rm{li}"], bn.running_mean, 1e-10, "running_mean")
            _close(ref[f"rv{li}"], bn.running_var, 1e-10, "running_var")
            assert int(bn.num_batches_tracked) == 1
        else:
            assert f"rm{li}" not in ref
            assert torch.equal(bn.running_mean, inp["layers"][li].rm.double()) and int(bn.num_batches_tracked) == 0


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("cid", ["dg-layer1", "dg-layer2", "dg-nq33"])
def test_exact_dgcnn_layer_is_the_torch_modules(cid, training):
    c = R.BY_ID[cid]
    inp = R.inputs(c)
    ref, _ = R.exact(c)
    Co, C2 = inp["W"].shape
    seq = torch.nn.Sequential(torch.nn.Conv2d(C2, Co, kernel_size=1, bias=False), torch.nn.GroupNorm(4, Co),
                              torch.nn.LeakyReLU(negative_slope=0.2)).double()
    with torch.no_grad():
        seq[0].weight.copy_(inp["W"][:, :, None, None]); seq[1].weight.copy_(inp["gamma"]); seq[1].bias.copy_(inp["beta"])
    seq.train(training)
    xk = inp["x_k"].double().requires_grad_()
    xq = xk if inp["x_q"] is None else inp["x_q"].double().requires_grad_()
    B, Nq, K = inp["idx"].shape
    nb = xk[torch.arange(B)[:, None, None], inp["idx"]]                           # pointnet2_utils.py:404-431, get_graph_feature
    q = xq.unsqueeze(2).expand(-1, -1, K, -1)
    f = torch.cat((nb - q, q), dim=-1).permute(0, 3, 1, 2)                        # [B, 2C, Nq, K]
    out = seq(f).max(dim=-1, keepdim=False)[0].permute(0, 2, 1)
    out.backward(inp["dout"].double())
    _close(ref["out"], out.detach(), 1e-10, "out")
    _close(ref["dx_k"], xk.grad, 1e-10, "dx_k")
    if inp["x_q"] is not None:
        _close(ref["dx_q"], xq.grad, 1e-10, "dx_q")
    for k, t in (("W", seq[0].weight.grad[:, :, 0, 0]), ("g0", seq[1].weight.grad), ("be0", seq[1].bias.grad)):
        _close(ref[k], t, 1e-10, k)


@pytest.mark.parametrize("cid", ["fp-m330", "cbr-m640", "dg-nq33", "dg-tie"])
def test_written_out_backward_is_exact_in_fp64(cid):
    """the rounding model's hand-written backward, without casts and in fp64 (S = 4 on the way), against exact's autograd"""
    c = R.BY_ID[cid]
    for training in MODES[c.node]:
        ref, _ = R.exact(c, training)
        got = R.model(c, R.Opt(ft=torch.float64, S=4.0), training)
        assert set(got) == set(ref)
        for k in ref:
            _close(got[k], ref[k], 1e-9, f"{cid} {k}")


# ------------------------------------------------------------------------------------------------ the criterion
@pytest.mark.parametrize("T", R.DTYPES, ids=R.dtype_name)
@pytest.mark.parametrize("c", R.CASES, ids=CASE_IDS)
def test_tiled_model_passes_at_half_the_cap(c, T):
    for training in MODES[c.node]:
        ref, mag, mod = R.references(c, T, training)
        res = R.ratios(R.rounded_tiled(c, T, training), mod, ref, mag)
        print(f"DEC-REF tiled {R.case_id(c)} {R.dtype_name(T)} {'train' if training else 'eval'} " + " ".join(f"{k}={v[0]:.3f}" for k, v in res.items()))
        for k, (q, ch) in res.items():
            assert q <= R.CAP / 2, f"{R.case_id(c)} {R.dtype_name(T)} {k}: ratio {q:.3f} at channel {ch}"


# (mutation, case, format, training, S): each where it can act (module docstring)
MUTANTS = [
    ("bn_train_terms_dropped", "fp-m640", F16, True, 1.0), ("bn_train_terms_dropped", "cbr-m330", BF16, True, 1.0),
    ("bn_eval_terms_kept", "fp-m330", F16, False, 1.0), ("bn_eval_terms_kept", "cbr-m640", BF16, False, 1.0),
    ("ragged_chunk", "fp-m330", F16, True, 1.0), ("ragged_chunk", "cbr-m330", BF16, False, 1.0),
    ("last_quad", "fp-nop1", F16, True, 1.0), ("last_quad", "cbr-m640", BF16, False, 1.0),
    ("db_unmasked", "fp-m640", BF16, False, 1.0), ("db_unmasked", "cbr-m330", F16, False, 1.0),
    ("interp_unnormalised", "fp-m640", BF16, True, 1.0), ("interp_unnormalised", "fp-nop1", F16, False, 1.0),
    ("wd_is_wb", "dg-layer1", F16, True, 1.0), ("wd_is_wb", "dg-layer2", BF16, True, 1.0),
    ("tie_to_all", "dg-tie", F16, True, 1.0), ("tie_to_all", "dg-tie", BF16, True, 1.0),
    ("gn_n_without_cg", "dg-layer1", BF16, True, 1.0), ("gn_n_without_cg", "dg-nq33", F16, True, 1.0),
    ("unscale_missing", "fp-m640", F16, True, 512.0), ("unscale_missing", "cbr-m330", BF16, True, 256.0),
]


@pytest.mark.parametrize("mutation,cid,T,training,S", MUTANTS,
                         ids=[f"{m}-{c}-{R.dtype_name(d)}-{'train' if t else 'eval'}" for m, c, d, t, _ in MUTANTS])
def test_mutated_model_fails(mutation, cid, T, training, S):
    c = R.BY_ID[cid]
    ref, mag, mod = R.references(c, T, training)
    if S != 1.0:
        mod = R.rounded(c, T, training, S=S)
    res = R.ratios(R.rounded(c, T, training, S=S, mut=mutation), mod, ref, mag)
    print(f"DEC-REF mutant {mutation} {cid} {R.dtype_name(T)} " + " ".join(f"{k}={v[0]:.1f}" for k, v in res.items()))
    assert max(v[0] for v in res.values()) > R.CAP, res


def _tiny_gradient(c):
    inp = dict(R.inputs(c))
    inp["dout"] = inp["dout"] * 2.0 ** -20
    return inp


def test_dgamma_from_the_rounded_gradient_is_seen_where_it_underflows():
    """(module docstring) gradients in T's normal range: below the cap, and documented; float16, a gradient of 2^-20 and S = 1:
    T(g) is subnormal or zero and dgamma shows it"""
    c = R.BY_ID["cbr-m640"]
    for T in R.DTYPES:
        ref, mag, mod = R.references(c, T, True)
        res = R.ratios(R.rounded(c, T, True, mut="dgamma_from_rounded"), mod, ref, mag)
        print(f"DEC-REF mutant dgamma_from_rounded cbr-m640 {R.dtype_name(T)} normal range g0={res['g0'][0]:.3f}")
        assert res["g0"][0] <= R.CAP, res
    inp = _tiny_gradient(c)
    ref, mag = R.exact(c, True, inp)
    mod = R.rounded(c, F16, True, inp=inp)
    res = R.ratios(R.rounded(c, F16, True, mut="dgamma_from_rounded", inp=inp), mod, ref, mag)
    print(f"DEC-REF mutant dgamma_from_rounded cbr-m640 f16 2^-20 g0={res['g0'][0]:.1f}")
    assert res["g0"][0] > R.CAP


def test_gradient_scale_is_what_keeps_float16_gradients():
    """the rounding model itself with a gradient of 2^-20: with S = 2^floor(log2(rows)) it stays where it is at S = 1 with a
    gradient of order one; without, float16 loses the gradient and the criterion says so (the GPU test relies on this)"""
    c = R.BY_ID["fp-m640"]
    inp = _tiny_gradient(c)
    ref, mag = R.exact(c, True, inp)
    good = R.rounded(c, F16, True, S=512.0, inp=inp)
    res = R.ratios(R.rounded(c, F16, True, S=1.0, inp=inp), good, ref, mag, skip=("out", "rm0", "rv0", "rm1", "rv1"))
    print("DEC-REF unscaled f16 2^-20 fp-m640 " + " ".join(f"{k}={v[0]:.1f}" for k, v in res.items()))
    assert max(v[0] for v in res.values()) > R.CAP
    for k in ref:
        if k not in R.ZERO_IN_TRAIN:
            assert not ((good[k] == 0) & (ref[k] != 0)).any(), k


# ------------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("c", R.CASES + R.GENERIC, ids=[R.case_id(c) for c in R.CASES + R.GENERIC])
def test_inputs_are_away_from_ties(c):
    lead, lead_rounded, nudged = R.conditioning(c)
    print(f"DEC-REF conditioning {R.case_id(c)} fp64 {lead:.2e} rounded {lead_rounded:.2e} nudged {100 * nudged:.3f} %")
    assert lead >= R.MARGIN and lead_rounded >= R.MARGIN_ROUNDED and nudged <= R.MAX_NUDGED
    if c.name == "tie":
        inp = R.inputs(c)
        a, b = inp["dup"]
        assert torch.equal(inp["x_k"][:, a], inp["x_k"][:, b]) and torch.equal(inp["coor"][:, a], inp["coor"][:, b])
        both = ((inp["idx"] == a).any(-1) & (inp["idx"] == b).any(-1)).sum().item()
        assert both >= 4                                                          # queries that have both twins as neighbours
        pos_a = (inp["idx"] == a).float().argmax(-1)[(inp["idx"] == a).any(-1) & (inp["idx"] == b).any(-1)]
        pos_b = (inp["idx"] == b).float().argmax(-1)[(inp["idx"] == a).any(-1) & (inp["idx"] == b).any(-1)]
        assert (pos_a < pos_b).all()                                              # the lower index comes first: it is the first maximiser
