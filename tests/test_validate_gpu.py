"""GPU: csrc/metrics.hip and ppt_amd/evaluate.py on the cases of tests/golden/g_validate.npz, which the reference's own
main_cls.validate / main_partseg.validate wrote (tests/golden/make_golden_validate.py).  The kernels' integer records must equal
a plain torch recomputation exactly (tests/validate_ref.py); the returned figures must be bit-equal to the reference's, except
`loss`: within 4 x the reference's own recorded |fp32 - fp64| deviation of the fp64 value, floor 1e-6 relative (the measured
deviation is printed: pytest -s)."""
import contextlib
import io
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import validate_ref as V
from ppt_amd import weights as W

pytestmark = pytest.mark.gpu


def _loss_col(rec, col):
    return rec[:, col].contiguous().view(torch.float32).double()


def _ints_equal(got, want, loss_col):
    keep = [c for c in range(want.shape[1]) if c != loss_col]
    return torch.equal(got[:, keep], want[:, keep])


def _run_partseg(name):
    from ppt_amd import evaluate
    c = V.ps_case(name)
    m = evaluate.PartsegMetrics(V.category2part(), c["smoothing"])
    o = 0
    for b in c["sizes"]:
        m.update(c["logits"][o:o + b].cuda(), c["labels"][o:o + b].cuda())
        o += b
    return m


def _run_cls(name):
    from ppt_amd import evaluate
    c = V.cls_case(name)
    m = evaluate.ClsMetrics(c["logits"].shape[1], c["smoothing"], c["classnames"])
    o = 0
    for b in c["sizes"]:
        m.update(c["logits"][o:o + b].cuda(), c["labels"][o:o + b].cuda())
        o += b
    return m


@pytest.mark.parametrize("name", V.PS_CASES)
def test_partseg_kernel_and_figures(name):
    c = V.ps_case(name)
    m = _run_partseg(name)
    got = m.records.host()
    got_t = torch.from_numpy(got)
    assert _ints_equal(got_t, c["records"], 4), (got_t[:, :8], c["records"][:, :8])
    # a cloud's loss sum: double accumulation rounded to fp32 once on both sides -> a few fp32 ulps of expf / log differences
    rel = ((_loss_col(got_t, 4) - _loss_col(c["records"], 4)).abs() / _loss_col(c["records"], 4)).max().item()
    print(f"VALIDATE {name}: cloud loss sums, max relative deviation from the double recomputation {rel:.3g}")
    assert rel < 1e-6
    out = m.result()
    V.check_partseg_figures(name, out)
    assert out["n"] == sum(c["sizes"]) and out["nonfinite_rows"] == 0


@pytest.mark.parametrize("name", V.CLS_CASES)
def test_cls_kernel_and_figures(name):
    c = V.cls_case(name)
    m = _run_cls(name)
    got_t = torch.from_numpy(m.records.host())
    assert _ints_equal(got_t, c["records"], 0), (got_t, c["records"])
    rel = ((_loss_col(got_t, 0) - _loss_col(c["records"], 0)).abs() / _loss_col(c["records"], 0)).max().item()
    print(f"VALIDATE {name}: row losses, max relative deviation from the double recomputation {rel:.3g}")
    assert rel < 1e-6
    out = m.result()
    V.check_cls_figures(name, out)
    assert out["n"] == sum(c["sizes"]) and out["nonfinite_rows"] == 0


def test_update_makes_no_host_read_and_runs_are_byte_identical():
    """update() under torch.cuda.set_sync_debug_mode("error") (any synchronising call raises), buffer growth included; two runs of
    every case leave identical bytes -- the multi-chunk case too, whose chunks meet in atomics and a last-arrival fold."""
    from ppt_amd import evaluate
    inputs = {n: [(V.ps_case(n)["logits"].cuda(), V.ps_case(n)["labels"].cuda())] for n in V.PS_CASES}
    x, y = V.cls_case("cls40")["logits"].cuda(), V.cls_case("cls40")["labels"].cuda()
    big = torch.randn(300, 40, device="cuda")                   # more rows than the buffer starts with: it doubles
    big_y = torch.randint(0, 40, (300,), device="cuda")
    torch.cuda.synchronize()
    runs = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            ms = []
            for n in V.PS_CASES:
                m = evaluate.PartsegMetrics(V.category2part(), 0.3)
                for lg, lb in inputs[n]:
                    m.update(lg, lb)
                ms.append(m)
            m = evaluate.ClsMetrics(40, 0.2)
            m.update(x, y)
            m.update(big, big_y)
            m.update(x, y)
            ms.append(m)
            res, correct = evaluate.accuracy(x, y, topk=(1, 5))
            runs.append((ms, res, correct))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    a, b = ([m.records.host().tobytes() for m in r[0]] for r in runs)
    assert a == b
    assert runs[0][0][-1].records.n == 21 + 300 + 21 and runs[0][0][-1].records.buf.shape[0] >= 342
    # utils.accuracy's return shape and values (utils/utils.py:376-398)
    ms, res, correct = runs[0]
    rank = V.cls_case("cls40")["records"][:, 1]
    assert correct.shape == (5, 21) and correct.dtype == torch.bool and res[0].shape == (1,) and res[0].is_cuda
    assert torch.equal(correct.cpu(), rank.view(1, -1) == torch.arange(5).view(-1, 1))
    for r, k in zip(res, (1, 5)):                               # correct[:k].reshape(-1).float().sum(0, keepdim=True).mul_(1.0 / B)
        assert r.item() == torch.tensor([float((rank < k).sum())]).mul_(1.0 / 21).item()


def test_flags_and_limits():
    """a non-finite logit and a label outside the range set their bits (result() raises ValueError on the label); P = 65 and 9
    parts per category return PPT_EUNSUPPORTED with nothing launched"""
    from ppt_amd import _lib, evaluate, ops
    c = V.cls_case("cls15")
    x, y = c["logits"].clone(), c["labels"].clone()
    x[2, 7] = float("inf")
    y[4] = 15
    m = evaluate.ClsMetrics(15, 0.2)
    m.update(x.cuda(), y.cuda())
    rec = m.records.host()
    assert rec[2, 2] == ops.METRIC_NONFINITE and rec[4, 2] == ops.METRIC_BAD_LABEL and rec[4, 3] == -1 and rec[4, 1] == 15
    assert (np.delete(rec[:, 2], [2, 4]) == 0).all()
    with pytest.raises(ValueError, match="label"):
        m.result()
    p = V.ps_case("ps_five")
    lg, lb = p["logits"][:3].clone(), p["labels"][:3].clone()
    lg[0, 95, 49] = float("nan")
    lb[1, 17] = 50
    lb[2, 0] = -1
    m = evaluate.PartsegMetrics(V.category2part(), 0.0)
    m.update(lg.cuda(), lb.cuda())
    rec = m.records.host()
    assert rec[0, 3] == ops.METRIC_NONFINITE and rec[1, 3] == ops.METRIC_BAD_LABEL and rec[2, 3] == ops.METRIC_BAD_LABEL
    assert (rec[2, :3] == 0).all() and (rec[2, 8:] == 0).all()             # no category: no counts
    with pytest.raises(ValueError, match="label"):
        m.result()
    # the limits, through the C entry point itself
    L = _lib.lib()
    z = torch.zeros(2 * 8 * 65, device="cuda")
    lbl = torch.zeros(2 * 8, dtype=torch.int64, device="cuda")
    tbl = torch.zeros(65, dtype=torch.int32, device="cuda")
    rec = torch.full((2, 32), 7, dtype=torch.int32, device="cuda")
    part = torch.zeros(2, device="cuda")
    args = lambda P, mp: (z.data_ptr(), lbl.data_ptr(), 0.0, 2, 8, P, tbl.data_ptr(), tbl.data_ptr(), mp, rec.data_ptr(), part.data_ptr(), None)
    assert L.ppt_partseg_metrics(*args(65, 4)) == -3
    assert L.ppt_partseg_metrics(*args(50, 9)) == -3
    torch.cuda.synchronize()
    assert (rec == 7).all()                                                 # nothing was launched, nothing cleared
    with pytest.raises(RuntimeError, match="ppt_partseg_metrics"):
        ops.partseg_metrics(z.view(2, 8, 65), lbl.view(2, 8), 0.0, tbl, tbl, 4, rec, part)


class _Recording(torch.nn.Module):
    """hands the model's own logits on and keeps a copy of them"""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, []

    def forward(self, *a):
        out = self.inner(*a)
        self.seen.append(out.detach().clone())
        return out


def _args(task, ds):
    from ppt_amd.models import ULIP_models as M
    return SimpleNamespace(classnames=M.dataset_classnames(ds), template_init='', class_name_position='middle',
                           num_learnable_prompt_tokens=32, gpu=0, task=task, head_type=0, evaluate_3d=False, ulip2=False,
                           synthetic_weights=True)


def test_validate_end_to_end_recognition():
    """validate() with ULIP_PointBERT on synthetic weights, B = 4 x 1024 points, two batches (the second of 3): the figures equal
    the host finalisation of the torch-recomputed records of the logits model(pc) returned"""
    from ppt_amd import evaluate
    from ppt_amd.models import ULIP_models as M
    args = _args('cls', "modelnet40")
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.ULIP_PointBERT(args)
    m.load_state_dict(W.ulip_pointbert_state_dict(seed=0), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding(40, seed=0)
    m.cuda()
    pc, _ = W.synth_clouds(7, 1024, seed=31)
    pc = torch.from_numpy(pc)
    labels = torch.tensor([3, 9, 9, 17, 39, 0, 3])
    loader = [(pc[:4], labels[:4], None), (pc[4:], labels[4:], None)]
    model = _Recording(m)
    with contextlib.redirect_stdout(io.StringIO()) as printed:
        out = evaluate.validate(loader, model, torch.nn.CrossEntropyLoss(label_smoothing=0.2), args)
    assert not m.training and len(model.seen) == 2
    logits = torch.cat(model.seen).float().cpu()
    assert logits.shape == (7, 40) and torch.isfinite(logits).all()
    want = evaluate.finalize_cls(V.cls_records(logits, labels, 0.2).numpy(), [4, 3], args.classnames)
    for k in ("acc", "acc5", "n", "nonfinite_rows", "per_class_acc"):
        assert out[k] == want[k], (k, out[k], want[k])
    assert abs(out["loss"] - want["loss"]) <= 1e-6 * want["loss"]
    assert ','.join(want["per_class_acc"].keys()) in printed.getvalue().splitlines()           # main_cls.py:294


def test_validate_end_to_end_partseg():
    """validate_partseg() with ULIP_PointBERT_partseg on synthetic weights, B = 2 x 2048 points (clouds split over several
    workgroups), the one-hot class label built on the device"""
    from ppt_amd import evaluate
    from ppt_amd.models import ULIP_models as M
    args = _args('partseg', "shapenetpart")
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.ULIP_PointBERT_partseg(args)
    m.load_state_dict(W.ulip_partseg_state_dict(seed=0), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding(50, seed=0)
    m.cuda()
    c2p = V.category2part()
    pc, _ = W.synth_clouds(2, 2048, seed=55)
    g = torch.Generator().manual_seed(5)
    cls = torch.tensor([[10], [1]])                                      # Motorbike (6 parts), Bag (2)
    part = torch.stack([torch.randint(30, 36, (2048,), generator=g), torch.randint(4, 6, (2048,), generator=g)])
    loader = [(torch.from_numpy(pc), cls, part)]
    loader = type("L", (list,), {})(loader)
    loader.dataset = SimpleNamespace(category2part=c2p)
    model = _Recording(m)
    with contextlib.redirect_stdout(io.StringIO()):
        out = evaluate.validate_partseg(loader, model, torch.nn.CrossEntropyLoss(label_smoothing=0.3), args)
    assert not m.training and len(model.seen) == 1
    logits = model.seen[0].float().cpu()
    assert logits.shape == (2, 2048, 50) and torch.isfinite(logits).all()
    want = evaluate.finalize_partseg(V.partseg_records(logits, part, c2p, 0.3).numpy(), [(2, 2048)], c2p)
    for k in ("acc", "mean_inst_iou", "n", "nonfinite_rows", "category_counts"):
        assert out[k] == want[k], (k, out[k], want[k])
    assert V.same_bits(out["mean_class_iou"], want["mean_class_iou"])
    assert V.same_bits(list(out["category_ious"].values()), list(want["category_ious"].values()))
    assert abs(out["loss"] - want["loss"]) <= 1e-6 * want["loss"]
