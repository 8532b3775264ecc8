"""The criterion of tests/chain_ends_ref.py proved without a GPU (tests/test_chain_ends_gpu.py applies it to the kernels):

  1. the fp64 references equal torch's own fp64 results on every case (1e-12 relative): torch.nn.functional.layer_norm and its
     double autograd, cross_entropy(label_smoothing=...) and its autograd through t / t.norm(), index_put and its autograd;
  2. a correct fp32 evaluation in another summation order (chain_ends_ref.standin) sits at <= tol / 2 in every output of every case
     -- |x - exact| <= E / 2 + R: the half of E, the arithmetic's share; a 16-bit store errs up to exactly R whatever computed it
     -- and holds the bits of the documented orders;
  3. every mutation of chain_ends_ref.MUTATIONS exceeds tol (or breaks the bits) on each of the cases chosen for it, at least two.

The worst ratios are printed (pytest -s): profiles/chain_ends_tests.md holds them.
"""
import collections

import pytest
import torch

import chain_ends_ref as R

F = torch.nn.functional
_WORST = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(_WORST):
        print(f"\nCHAIN-ENDS-REF worst stand-in ratio {k}: {_WORST[k]:.3f}", end="")
    print()


def _close(a, b, what):
    a, b = a.double(), b.double()
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= 1e-12 * scale, (what, float((a - b).abs().max()), scale)


def _row64(c, I):
    r = I["x"].double()
    if c.op == "ln_fwd_sum":
        r = r + (I["bias"].double() if c.bias else 0) + I["parts"].double().sum(0)
    elif c.add:
        a = I["add"].double()
        r = r + (a if c.add == "full" else a.repeat((c.M + a.shape[0] - 1) // a.shape[0], 1)[:c.M])
    return r


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_reference_is_torch_fp64(case):
    c, I, ref = case, R.inputs(case), R.reference(case)
    ex = {k: v.exact for k, v in ref.items()}
    if c.op in ("ln_fwd", "ln_fwd_sum", "ln_chain"):
        r = _row64(c, I).requires_grad_(True)
        w, b = I["w"].double(), I["b"].double()
        y = F.layer_norm(r, (c.D,), w, b, c.eps)
        _close(ex["y"], y.detach(), "y")
        if c.stats:
            _close(ex["mean"], r.detach().mean(1), "mean")
            _close(ex["rstd"], (r.detach().var(1, unbiased=False) + c.eps).rsqrt(), "rstd")
        if "xs" in ex:
            _close(ex["xs"], r.detach(), "xs")
            assert R.worst(ref["xs"].bits, ref["xs"]) <= 1.0
        if c.op == "ln_chain":
            y.backward(I["dy"].double())
            _close(ex["dx"], r.grad, "dx")
    elif c.op in ("ln_bwd", "ln_bwd_sum", "ln_bwd_w"):
        # the kernel's operands are the fp32-rounded statistics: the formula itself against autograd on the exact ones, then the
        # case's reference is that formula on the rounded ones
        x, w, b = I["xs"].double().requires_grad_(True), I["w"].double().requires_grad_(True), I["b"].double().requires_grad_(True)
        dy = I["dy"].double().sum(0) if c.S else I["dy"].double()
        F.layer_norm(x, (c.D,), w, b, c.eps).backward(dy)
        xd = x.detach()
        got = R.ln_bwd64(dy, xd, w.detach(), xd.mean(1), (xd.var(1, unbiased=False) + c.eps).rsqrt())
        _close(got["dx"], x.grad, "dx")
        _close(got["dw"], w.grad, "dw")
        _close(got["db"], b.grad, "db")
        mine = R.ln_bwd64(dy, xd, w.detach(), I["mean"].double(), I["rstd"].double())
        _close(ex["dx"], mine["dx"] + (I["dx0"].double() if c.acc else 0), "dx on the operand statistics")
        if c.op == "ln_bwd_w":
            _close(ex["dw"], mine["dw"], "dw")
            _close(ex["db"], mine["db"], "db")
        if c.copy:
            _close(ex["copy"], ex["dx"], "copy")
    elif c.op == "matmul":
        _close(ex["out"], c.alpha * (I["a"].double() @ I["w"].double()), "out")
    elif c.op == "head":
        t = I["text"].double().requires_grad_(True)
        logits = torch.exp(I["scale"].double()) * (I["feat"].double() @ I["w"].double()) @ (t / t.norm(dim=-1, keepdim=True)).t()
        loss = F.cross_entropy(logits, I["labels"], label_smoothing=c.smooth)
        loss.backward()
        _close(ex["logits"], logits.detach(), "logits")
        _close(ex["loss"], loss.detach(), "loss")
        _close(ex["d_text"], t.grad, "d_text")
    elif c.op in ("rows", "rows_bwd"):
        slot = I["slot"].long()
        idx = torch.nonzero(slot >= 0)[:, 0]
        gen = torch.Generator().manual_seed(5)
        Rn = slot.numel()
        base = (I["base"] if c.op == "rows" else torch.randn(Rn, c.W, generator=gen)).double()
        pos = (I["pos"] if c.op == "rows" else torch.randn(Rn, c.W, generator=gen)).double()
        tok = (I["tokens"] if c.op == "rows" else torch.randn(R.N_TOK, c.W, generator=gen)).double().requires_grad_(True)
        out = base.clone().index_put((idx,), tok[slot[idx]] + pos[idx])
        if c.op == "rows":
            _close(ex["out"], out.detach(), "rows")
        else:
            # rows_of lists exactly the rows of each token, ascending, -1 behind them
            for t_ in range(R.N_TOK):
                rows = torch.nonzero(slot == t_)[:, 0].tolist()
                assert I["rows_of"][t_].tolist() == rows + [-1] * (c.max_rows - len(rows))
            (out * I["g"].double()).sum().backward()
            _close(ex["out"], c.sc * tok.grad, "d tokens")
            assert float(ex["out"][1].abs().max()) == 0.0 and (I["rows_of"][0] >= 0).all() and (I["rows_of"][1] < 0).all()
    else:
        raise AssertionError(c.op)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_standin_passes_at_half_the_tolerance(case):
    errors = []
    res = R.check(case, R.standin(case), errors, cap=0.5, what="CHAIN-ENDS-REF standin")
    for name, v in res.items():
        k = f"{R.family(case, name)} {name}"
        _WORST[k] = max(_WORST[k], v)
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("mutation,cid", [(m, cid) for m in R.MUTATIONS for cid in R.MUTANT_CASES[m]])
def test_mutation_is_caught(mutation, cid):
    c = R.BY_ID[cid]
    errors = []
    res = R.check(c, R.standin(c, mutate=mutation), errors, what=f"CHAIN-ENDS-REF mutant {mutation}")
    assert errors, f"{mutation} passes {cid}: {res}"


def test_tables():
    R._assert_coverage()
    assert all(len(v) >= 2 for v in R.MUTANT_CASES.values())
    for c in R.CASES:
        assert c.note and R.family(c) in R.FAMILIES | {"ln_bwd_dx8_kernel (S = %d slices)" % c.S}, R.case_id(c)
    # place(): the window is 16 bytes in (20 when misaligned), NaN or the sentinel everywhere else
    v = torch.arange(6, dtype=torch.float32).view(2, 3)
    for mis in (False, True):
        buf, win = R.place(v, mis)
        assert torch.equal(win, v) and win.data_ptr() - buf.data_ptr() == (20 if mis else 16) and int(torch.isnan(buf).sum()) == buf.numel() - 6
        assert torch.equal(R.window(buf, v.shape, mis), v)
        sb, sw = R.place(v, mis, sentinel=True)
        assert R.outside_same(sb, sb.clone(), v.shape, mis)
        sb2 = sb.clone(); sb2[0] = 1.0
        assert not R.outside_same(sb2, sb, v.shape, mis)
