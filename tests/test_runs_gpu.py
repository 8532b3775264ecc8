"""GPU: the training meters (csrc/meters.hip) against AverageMeter's arithmetic restated in Python floats, ppt_sgd_multi and
Trainer(optim=...) against torch.optim, and run_cls / run_partseg against the same loops written out with Trainer.step, .item()
meters and evaluate.validate."""
import contextlib
import io
import math
import os
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ppt_amd import weights as W

pytestmark = pytest.mark.gpu


# ---- the meters --------------------------------------------------------------------------------------------------------------
class _Meter:
    """AverageMeter.update (utils/utils.py:333-337) on Python floats + the record's counters, as include/ppt_hip.h lays them out"""

    def __init__(self):
        self.rec = [0.0] * 8

    def update(self, loss, acc, weight, metered, bad_label):
        r = self.rec
        r[3] += 1
        r[4] += 0 if math.isfinite(loss) else 1                # main_cls.py:205 sits in front of the `continue` of :209
        r[7] += 1 if bad_label else 0
        if metered:
            r[0] += loss * weight                              # sum += val * n
            r[1] += acc * weight
            r[2] += weight
            r[5], r[6] = loss, acc

    def bytes(self):
        return np.asarray(self.rec, dtype=np.float64).tobytes()


def _rec_bytes(rec):
    return rec.cpu().numpy().tobytes()


def _cls_calls(B, C, seed):
    """5 steps: integer-valued logits (tied maxima in most rows), a row of NaNs in step 2, a label equal to C in the un-metered
    step 1, a NaN loss in the last, metered step"""
    g = torch.Generator().manual_seed(seed)
    calls = []
    for i, (metered, weight) in enumerate([(True, 1.0), (False, 1.0), (True, 4.0), (False, 1.0), (True, 2.0)]):
        logits = torch.randint(-2, 3, (B, C), generator=g).float()
        logits[0, :] = 2.0                                     # a row whose every class ties: index 0 wins
        y = torch.randint(0, C, (B,), generator=g)
        y[0] = 0 if i % 2 == 0 else C - 1
        if B > 2:
            logits[2, C - 1] = logits[2, C // 2] = 7.0         # two maxima: the lower index wins
            y[2] = C // 2 if i < 3 else C - 1
        if i == 2:
            logits[B - 1, :] = float("nan")
            y[B - 1] = C - 1                                   # (torch.argmax names index 0 for a row of NaNs: wrong either way)
        if i == 1:
            y[B // 2] = C
        loss = torch.tensor(float("nan") if i == 4 else 0.25 + 1.37 * i, dtype=torch.float32)
        calls.append((logits, y, loss, weight, metered))
    return calls


@pytest.mark.parametrize("B, C", [(1, 3), (5, 40), (64, 15), (33, 65)])
def test_cls_meter_equals_the_python_meters_bit_for_bit(B, C):
    from ppt_amd import ops
    calls = _cls_calls(B, C, seed=B * 100 + C)
    finals = []
    for _ in range(2):
        rec = torch.zeros(8, dtype=torch.float64, device="cuda")
        want = _Meter()
        for logits, y, loss, weight, metered in calls:
            ops.train_meter_cls(logits.cuda(), y.cuda(), loss.cuda(), rec, weight, metered)
            acc = float((logits.argmax(dim=1) == y).sum() / len(y))               # main_cls.py:200-202
            want.update(loss.item(), acc, weight, metered, bool(((y < 0) | (y >= C)).any()))
            assert _rec_bytes(rec) == want.bytes(), (rec.cpu().tolist(), want.rec)
        finals.append(_rec_bytes(rec))
    assert finals[0] == finals[1]
    got = rec.cpu().tolist()
    assert got[3] == 5 and got[4] == 1 and got[7] == 1 and got[2] == 7.0 and math.isnan(got[0]) and math.isnan(got[5])
    if B > 2:
        assert 0 < got[1] < 7                                  # some rows right, some wrong: the ties decided something


def _partseg_calls(B, N, seed, c2p):
    """5 steps over P = 50: every cloud of a category of its own, the global maximum of every row OUTSIDE the category's range,
    integer-valued logits inside it (ties); in step 3 the last cloud's labels[b, 0] is 50"""
    g = torch.Generator().manual_seed(seed)
    cats = list(c2p.values())
    calls = []
    for i, metered in enumerate([True, False, True, True, False]):
        logits = torch.randint(-2, 3, (B, N, 50), generator=g).float()
        labels = torch.empty((B, N), dtype=torch.int64)
        for b in range(B):
            parts = cats[(3 * i + 5 * b + 10) % 16]
            labels[b] = torch.randint(parts[0], parts[-1] + 1, (N,), generator=g)
            logits[b, :, (parts[-1] + 1) % 50] = 9.0           # the row's arg-max over all 50 parts is not in the range
            if N > 1:
                logits[b, 1, parts[0]:parts[-1] + 1] = 1.0     # a full tie: the range's first part wins
        if i == 3:
            labels[B - 1, 0] = 50
        loss = torch.tensor(float("nan") if i == 4 else 3.5 - 0.61 * i, dtype=torch.float32)
        calls.append((logits, labels, loss, float(B), metered))
    return calls


def _partseg_acc(logits, labels, c2p):
    """main_partseg.py:218-229 with torch ops, one cloud after the other; a cloud without a category predicts nothing"""
    part2cat = {p: c for c, parts in c2p.items() for p in parts}
    B, N, _ = logits.shape
    refined = torch.full((B, N), -1, dtype=torch.int32)
    bad = False
    for i in range(B):
        idx = labels[i, 0].item()
        if idx not in part2cat:
            bad = True
            continue
        parts = c2p[part2cat[idx]]
        refined[i, :] = torch.argmax(logits[i][:, parts], dim=1) + parts[0]
    correct = torch.eq(refined, labels).sum()
    return (correct / (B * N)).item(), bad


@pytest.mark.parametrize("B, N", [(1, 1), (3, 257), (2, 2051)])
def test_partseg_meter_equals_the_per_cloud_loop_bit_for_bit(B, N):
    from ppt_amd import evaluate, ops, partseg
    c2p = partseg.shapenetpart_category2part()
    start, count = (torch.from_numpy(t).cuda() for t in evaluate.part_tables(c2p))
    calls = _partseg_calls(B, N, seed=B * 10000 + N, c2p=c2p)
    finals = []
    for _ in range(2):
        rec = torch.zeros(8, dtype=torch.float64, device="cuda")
        scratch = torch.zeros(4, dtype=torch.int32, device="cuda")
        want = _Meter()
        for logits, labels, loss, weight, metered in calls:
            ops.train_meter_partseg(logits.cuda(), labels.cuda(), loss.cuda(), start, count, rec, scratch, weight, metered)
            acc, bad = _partseg_acc(logits, labels, c2p)
            want.update(loss.item(), acc, weight, metered, bad)
            assert _rec_bytes(rec) == want.bytes(), (rec.cpu().tolist(), want.rec)
            assert scratch.cpu().tolist() == [0, 0, 0, 0]
        finals.append(_rec_bytes(rec))
    assert finals[0] == finals[1]
    got = rec.cpu().tolist()
    assert got[3] == 5 and got[4] == 1 and got[7] == 1 and got[2] == 3.0 * B
    if N > 1:
        assert 0 < got[1] < 3.0 * B


def test_partseg_meter_limits():
    from ppt_amd import ops
    z = torch.zeros((2, 8, 65), device="cuda")
    lbl = torch.zeros((2, 8), dtype=torch.int64, device="cuda")
    tbl = torch.ones(65, dtype=torch.int32, device="cuda")
    rec = torch.zeros(8, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="ppt_train_meter_partseg"):             # P > 64: PPT_EUNSUPPORTED, nothing launched
        ops.train_meter_partseg(z, lbl, torch.zeros((), device="cuda"), tbl, tbl, rec, scratch, 2.0, True)
    assert rec.cpu().tolist() == [0.0] * 8


# ---- the optimizers ----------------------------------------------------------------------------------------------------------
class _Tiny(torch.nn.Module):
    """three trained tensors and a frozen one in the middle (the checkpoint layout indexes over ALL parameters)"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.a = torch.nn.Parameter(torch.randn(32, 512, generator=g) * 0.02)
        self.frozen = torch.nn.Parameter(torch.randn(7, generator=g), requires_grad=False)
        self.b = torch.nn.Parameter(torch.randn(1025, generator=g) * 0.02)
        self.c = torch.nn.Parameter(torch.randn(1, generator=g))


def _close(p, ref):
    """the rule of test_adamw_step_matches_torch"""
    return (p - ref).abs().max().item() < 2e-7 * max(1.0, ref.abs().max().item())


def _grads(model, g, step):
    return [(torch.randn(p.shape, generator=g) * (10.0 ** (step - 3))).cuda() for p in model.parameters() if p.requires_grad]


def test_sgd_multi_matches_torch_and_counts_what_it_skips():
    from ppt_amd import ops
    g = torch.Generator().manual_seed(3)
    ref_model = _Tiny().cuda()
    trained = [p for p in ref_model.parameters() if p.requires_grad]
    opt = torch.optim.SGD(trained, lr=3e-3)                    # main_cls.py:55
    mine = [p.detach().clone() for p in trained]
    for step in range(1, 6):
        lr = 3e-3 / step
        for gr in opt.param_groups:
            gr['lr'] = lr
        grads = _grads(ref_model, g, step)
        for p, gd in zip(trained, grads):
            p.grad = gd.clone()
        opt.step()
        ops.sgd_multi(list(zip(mine, grads)), lr)
        for p, ref in zip(mine, trained):
            assert _close(p, ref.detach()), step
    # the non-finite skip: the element keeps its value, its gradient reads 0, the counter moves; the rest updates
    before = [p.clone() for p in mine]
    grads = _grads(ref_model, g, 3)
    grads[0][3, 7], grads[0][5, 9], grads[1][1024] = float("inf"), float("nan"), float("-inf")
    skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.sgd_multi(list(zip(mine, grads)), 1e-2, skipped=skipped)
    assert skipped.item() == 3 and all(torch.isfinite(p).all() for p in mine)
    assert mine[0][3, 7] == before[0][3, 7] and mine[0][5, 9] == before[0][5, 9] and mine[1][1024] == before[1][1024]
    assert grads[0][3, 7] == 0 and grads[0][5, 9] == 0 and grads[1][1024] == 0
    assert not torch.equal(mine[0][0], before[0][0]) and not torch.equal(mine[2], before[2])
    # without a counter: torch.optim.SGD's own behaviour, the value propagates
    grads = _grads(ref_model, g, 3)
    grads[2][0] = float("nan")
    ops.sgd_multi(list(zip(mine, grads)), 1e-2)
    assert torch.isnan(mine[2][0])


@pytest.mark.parametrize("optim", ["adam", "sgd"])
def test_trainer_optim_matches_torch_and_round_trips_its_state(optim):
    """Trainer(optim=...): main_cls.py:54-57's optimizers, stepped by the fused kernels, against torch's own over 5 steps with a
    changing lr; then the checkpoint's optimizer entry, through the reference's loader and back"""
    from ppt_amd.train import Trainer, load_reference_optimizer_state, reference_optimizer_state
    g = torch.Generator().manual_seed(4)
    model, ref_model = _Tiny().cuda(), _Tiny().cuda()
    tr = Trainer(model, lr=3e-3, optim=optim, distributed=False)
    assert type(tr.optimizer) is (torch.optim.Adam if optim == "adam" else torch.optim.SGD)
    trained = [p for p in model.parameters() if p.requires_grad]
    ref_trained = [p for p in ref_model.parameters() if p.requires_grad]
    opt = (torch.optim.Adam if optim == "adam" else torch.optim.SGD)(ref_trained, lr=3e-3)           # torch's defaults but lr
    calls = []
    from ppt_amd import ops
    real = {n: getattr(ops, n) for n in ("adamw_step", "adamw_multi", "sgd_multi")}
    try:
        for n, fn in real.items():
            setattr(ops, n, (lambda n_, fn_: lambda *a, **k: (calls.append(n_), fn_(*a, **k))[1])(n, fn))
        for step in range(1, 6):
            lr = 3e-3 / step
            for gr in list(opt.param_groups) + list(tr.optimizer.param_groups):
                gr['lr'] = lr
            grads = _grads(model, g, step)
            for p, q, gd in zip(trained, ref_trained, grads):
                p.grad, q.grad = gd.clone(), gd.clone()
            opt.step()
            tr._optimizer_step()
            for p, q in zip(trained, ref_trained):
                assert _close(p.detach(), q.detach()), step
                if optim == "adam":
                    m, v = tr.optimizer.state[p]['exp_avg'], tr.optimizer.state[p]['exp_avg_sq']
                    assert (m - opt.state[q]['exp_avg']).abs().max().item() <= 1e-6 * m.abs().max().item()
                    assert (v - opt.state[q]['exp_avg_sq']).abs().max().item() <= 1e-6 * v.abs().max().item()
    finally:
        for n, fn in real.items():
            setattr(ops, n, fn)
    assert calls == ["adamw_multi" if optim == "adam" else "sgd_multi"] * 5          # ONE launch per step, the kernel of its type
    # a non-finite gradient element is skipped and counted (this model names no precision: the guarded modes' behaviour)
    grads = _grads(model, g, 3)
    grads[1][5] = float("inf")
    for p, gd in zip(trained, grads):
        p.grad = gd
    tr._optimizer_step()
    assert tr.nonfinite_grad_elements() == 1 and all(torch.isfinite(p).all() for p in trained)

    # the checkpoint entry: indexed over model.parameters() (4 tensors), loadable by the reference's optimizer, and back
    entry = reference_optimizer_state(model, tr.optimizer)
    assert entry['param_groups'][0]['params'] == [0, 1, 2, 3] and entry['param_groups'][0]['lr'] == tr.optimizer.param_groups[0]['lr']
    assert sorted(entry['state']) == ([0, 2, 3] if optim == "adam" else [])          # SGD keeps no state
    theirs = (torch.optim.Adam if optim == "adam" else torch.optim.SGD)(model.parameters(), lr=5.0)  # main_cls.py:55 / :57
    theirs.load_state_dict(entry)
    assert theirs.param_groups[0]['lr'] == entry['param_groups'][0]['lr']
    fresh = Trainer(_Tiny().cuda(), lr=1.0, optim=optim, distributed=False)
    load_reference_optimizer_state(fresh.model, fresh.optimizer, entry)
    assert fresh.optimizer.param_groups[0]['lr'] == tr.optimizer.param_groups[0]['lr']
    fresh_trained = [p for p in fresh.model.parameters() if p.requires_grad]
    for p, q in zip(trained, fresh_trained):
        a, b = tr.optimizer.state.get(p, {}), fresh.optimizer.state.get(q, {})
        assert sorted(a) == sorted(b) == (['exp_avg', 'exp_avg_sq', 'step'] if optim == "adam" else [])
        for k in a:
            assert torch.equal(a[k].cpu(), b[k].cpu()), k
    back = reference_optimizer_state(fresh.model, fresh.optimizer)
    assert sorted(back['state']) == sorted(entry['state']) and back['param_groups'] == entry['param_groups']


def test_trainer_rejects_an_unknown_optimizer():
    from ppt_amd.train import Trainer
    with pytest.raises(ValueError, match="optim"):
        Trainer(_Tiny().cuda(), optim="lion", distributed=False)


# ---- the runs ----------------------------------------------------------------------------------------------------------------
def _bits(x):
    return struct.pack("<d", x) if isinstance(x, float) else x


def _same(a, b):
    """== on the logs with floats compared by their bits (a NaN equals itself: mean_class_iou of a test set without every category)"""
    if isinstance(a, dict) and isinstance(b, dict):
        return list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and _bits(a) == _bits(b)


def _cls_model(head_type):
    from ppt_amd.models import ULIP_models as M
    names = M.dataset_classnames("modelnet40")[:3]
    args = SimpleNamespace(classnames=names, template_init='', class_name_position='middle', num_learnable_prompt_tokens=32, gpu=0,
                           task='cls', head_type=head_type, evaluate_3d=False, ulip2=False, synthetic_weights=True)
    torch.manual_seed(0)                          # (an un-frozen block is random per construction)
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.ULIP_PointBERT(args)
    m.load_state_dict(W.ulip_pointbert_state_dict(seed=0), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding(3, seed=0)
    m.cuda().set_precision("fp32")
    return m, names


@pytest.mark.parametrize("head_type", [0, 2])
def test_run_cls_equals_the_loop_written_out(tmp_path, head_type):
    """3 classes, 14 train clouds (batches of 4, 4, 4, 2) and 5 test clouds of 1024 points, 2 epochs, data_ratio 0.5 (4 * 0.5 = 2.0:
    batches 0, 1, 2 run), update_freq 2 (schedule entries 0, 0, 1 / 2, 2, 3; only batch 1 is metered), fp32; head_type 0 takes the
    fused head path of Trainer.step, head_type 2 the general one"""
    from ppt_amd import evaluate, recognition
    from ppt_amd.data import DeviceBatchLoader, DeviceCloudSet
    from ppt_amd.train import Trainer, cosine_scheduler, load_prompt_checkpoint
    pc, _ = W.synth_clouds(19, 1024, seed=23)
    train_labels = np.array([2, 0, 1, 1, 0, 2, 2, 1, 0, 0, 1, 2, 0, 1])
    test_labels = np.array([0, 1, 2, 2, 1])

    def args_for(names, out):
        return SimpleNamespace(classnames=names, epochs=2, batch_size=4, npoints=1024, lr=3e-3, lr_start=1e-6, lr_end=1e-5,
                               warmup_epochs=1, label_smoothing=0.2, seed=0, head_type=head_type, recipe="modelnet", gpu=0,
                               data_ratio=0.5, update_freq=2, output_dir=out, proj_name="cls", exp_name="t")

    def sets():
        return DeviceCloudSet(pc[:14], train_labels), DeviceCloudSet(pc[14:], test_labels)

    # the run
    m, names = _cls_model(head_type)
    assert (sum(p.requires_grad for p in m.parameters()) == 1) == (head_type == 0)
    train_set, test_set = sets()
    torch.manual_seed(1)
    with contextlib.redirect_stdout(io.StringIO()):
        log = recognition.run_cls(m, train_set, test_set, args_for(names, str(tmp_path)))

    # the same loop, written out: main_cls.py:155-234 with its host reads
    m2, _ = _cls_model(head_type)
    train_set, test_set = sets()
    a = args_for(names, None)
    train_loader = DeviceBatchLoader(train_set, 4, 1024, "modelnet", train=True, shuffle=True, drop_last=False, seed=0)
    test_loader = DeviceBatchLoader(test_set, 4, 1024, "modelnet", train=False, shuffle=False, drop_last=False, seed=0)
    assert len(train_loader) == 4
    iters_per_epoch = len(train_loader) // 2
    sched = cosine_scheduler(3e-3, 1e-5, 2, iters_per_epoch, warmup_epochs=1, start_warmup_value=1e-6)
    tr = Trainer(m2, lr=3e-3, label_smoothing=0.2, lr_schedule=sched)
    criterion = torch.nn.CrossEntropyLoss(label_smoothing=0.2)
    torch.manual_seed(1)
    want, best_acc, best_epoch, steps = [], 0, -1, []
    for epoch in range(2):
        train_loader.set_epoch(epoch)
        m2.train()
        sums = {"loss": 0, "acc": 0, "count": 0}
        for data_iter, (x, y) in enumerate(train_loader):
            if data_iter > len(train_loader) * 0.5:
                break
            tr.it = iters_per_epoch * epoch + data_iter // 2
            steps.append(tr.it)
            loss, pred = tr.step(x, y)
            acc = torch.eq(pred.argmax(dim=1), y).sum() / len(y)
            assert math.isfinite(loss.item())
            if (data_iter + 1) % 2 != 0:
                continue
            logit_scale = m2.logit_scale.exp().item()
            sums["loss"] += loss.item() * 1
            sums["acc"] += acc.item() * 1
            sums["count"] += 1
        tr.finish()
        with contextlib.redirect_stdout(io.StringIO()):
            val = evaluate.validate(test_loader, m2, criterion, a)
        if val["acc"] > best_acc:
            best_epoch = epoch
        best_acc = max(val["acc"], best_acc)
        want.append({"train_loss": sums["loss"] / sums["count"], "train_acc": sums["acc"] / sums["count"],
                     "train_lr": tr.optimizer.param_groups[0]["lr"], "train_logit_scale": logit_scale,
                     **{f"test_{k}": v for k, v in val.items()}, "epoch": epoch, "best_acc": best_acc, "best_epoch": best_epoch})
    print(log)
    assert steps == [0, 0, 1, 2, 2, 3]
    assert log == want
    assert all(np.isfinite(e["train_loss"]) and np.isfinite(e["test_loss"]) for e in log)
    assert [e["train_lr"] for e in log] == [float(sched[1]), float(sched[3])]
    assert set(log[0]) >= {"train_loss", "train_acc", "train_lr", "train_logit_scale", "test_acc", "test_loss", "epoch", "best_acc",
                           "best_epoch"}

    # the checkpoint and its reader
    where = log[-1]["best_epoch"]
    assert where >= 0                             # (every class is in the test set: even a constant prediction scores above 0)
    ckpt = torch.load(os.path.join(str(tmp_path), "cls", "t", "checkpoint_best.pt"), weights_only=False)
    assert set(ckpt) == {'epoch', 'state_dict', 'optimizer', 'best_acc', 'args', 'last_block', 'ppt_precision'}
    assert ckpt['epoch'] == where + 1 and ckpt['best_acc'] == log[-1]["best_acc"] and list(ckpt['state_dict']) == ['learnable_tokens']
    assert (ckpt['last_block'] is not None) == (head_type > 0)
    if where == 1:
        assert torch.equal(ckpt['state_dict']['learnable_tokens'].cuda(), m.prompt_learner.learnable_tokens.detach())
    m3, _ = _cls_model(head_type)
    load_prompt_checkpoint(m3, ckpt)
    assert torch.equal(m3.prompt_learner.learnable_tokens.detach().cpu(), ckpt['state_dict']['learnable_tokens'].cpu())
    if head_type > 0:
        w = m3.point_encoder.blocks.blocks[-1].mlp.fc2.weight.detach().cpu()
        assert torch.equal(w, ckpt['last_block']['mlp.fc2.weight'].cpu())


def _partseg_model():
    from ppt_amd.models import ULIP_models as M
    args = SimpleNamespace(classnames=M.dataset_classnames("shapenetpart"), template_init='', class_name_position='middle',
                           num_learnable_prompt_tokens=32, gpu=0, task='partseg', head_type=0, evaluate_3d=False, ulip2=False,
                           synthetic_weights=True)
    torch.manual_seed(0)                          # (the decoder is random per construction)
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.ULIP_PointBERT_partseg(args)
    m.load_state_dict(W.ulip_partseg_state_dict(seed=0), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding(50, seed=0)
    m.cuda().set_precision("fp32")
    return m, args.classnames


def _partseg_sets(lengths_train, cats_train, lengths_test, cats_test, c2p, seed):
    from ppt_amd.data import DeviceCloudSet
    parts = list(c2p.values())
    rs = np.random.RandomState(seed)
    out = []
    for lengths, cats in ((lengths_train, cats_train), (lengths_test, cats_test)):
        pc, _ = W.synth_clouds(len(lengths), max(lengths), seed=seed + len(lengths))
        clouds = [np.ascontiguousarray(pc[i, :n]) for i, n in enumerate(lengths)]
        seg = [rs.randint(parts[c][0], parts[c][-1] + 1, n).astype(np.int32) for c, n in zip(cats, lengths)]
        out.append(DeviceCloudSet(clouds, np.asarray(cats), seg=seg))
    return out


def _partseg_args(names, c2p, out, **kw):
    base = dict(classnames=names, category2part=c2p, epochs=2, batch_size=2, npoints=1024, lr=3e-3, lr_start=1e-6, lr_end=1e-5,
                warmup_epochs=1, label_smoothing=0.2, seed=0, gpu=0, output_dir=out, proj_name="partseg", exp_name="t")
    base.update(kw)
    return SimpleNamespace(**base)


PARTSEG_KEYS = {'epoch', 'state_dict_prompt', 'state_dict_partseg', 'optimizer', 'best_test_acc', 'best_mean_class_iou',
                'best_mean_inst_iou', 'args', 'ppt_precision'}


def test_run_partseg_equals_the_loop_written_out(tmp_path):
    """6 ragged train clouds (3 batches of 2) and 3 test clouds, 1024 points sampled per cloud, 2 epochs, fp32.  Three test clouds
    cannot cover 16 categories: mean_class_iou is the reference's mean over an empty category, NaN, which never beats 0 -- the
    reference writes no checkpoint in such a run, and neither does this one (the payload: the next test)."""
    from ppt_amd import evaluate, partseg
    from ppt_amd.data import DeviceBatchLoader
    from ppt_amd.train import Trainer, cosine_scheduler
    c2p = partseg.shapenetpart_category2part()
    part2cat = {p: c for c, parts in c2p.items() for p in parts}

    def sets():
        return _partseg_sets([1500, 1024, 2000, 1100, 1800, 1300], [0, 10, 15, 4, 1, 8], [1200, 1024, 1700], [10, 0, 4], c2p, seed=7)

    m, names = _partseg_model()
    train_set, test_set = sets()
    torch.manual_seed(1)
    with contextlib.redirect_stdout(io.StringIO()):
        log = partseg.run_partseg(m, train_set, test_set, _partseg_args(names, c2p, str(tmp_path)))

    # the same loop, written out: main_partseg.py:164-257 with its host reads (one .item() per cloud, loss.item(), acc.item())
    m2, _ = _partseg_model()
    train_set, test_set = sets()
    a = _partseg_args(names, c2p, None)
    train_loader = DeviceBatchLoader(train_set, 2, 1024, "shapenetpart", train=True, shuffle=True, drop_last=False, seed=0)
    test_loader = DeviceBatchLoader(test_set, 2, 1024, "shapenetpart", train=False, shuffle=False, drop_last=False, seed=0)
    assert len(train_loader) == 3
    sched = cosine_scheduler(3e-3, 1e-5, 2, 3, warmup_epochs=1, start_warmup_value=1e-6)
    tr = Trainer(m2, lr=3e-3, label_smoothing=0.2, lr_schedule=sched)
    criterion = torch.nn.CrossEntropyLoss(label_smoothing=0.2)
    torch.manual_seed(1)
    want, best_epoch = [], -1
    best_test_acc = best_mean_class_iou = best_mean_inst_iou = 0
    for epoch in range(2):
        train_loader.set_epoch(epoch)
        m2.train()
        sums = {"loss": 0, "acc": 0, "count": 0}
        for data_iter, (x, cls_label, part_label) in enumerate(train_loader):
            tr.extra_inputs = (evaluate.to_categorical(cls_label, 16),)
            tr.it = 3 * epoch + data_iter
            loss, part_pred = tr.step(x, part_label)
            B, N, _ = x.size()
            refined = torch.zeros(B, N, dtype=torch.int32, device="cuda")
            for i in range(B):
                parts = c2p[part2cat[part_label[i, 0].item()]]
                refined[i, :] = torch.argmax(part_pred[i, :, :][:, parts], dim=1) + parts[0]
            acc = torch.eq(refined, part_label).sum() / (B * N)
            assert math.isfinite(loss.item())
            logit_scale = m2.logit_scale.exp().item()
            sums["loss"] += loss.item() * B
            sums["acc"] += acc.item() * B
            sums["count"] += B
        tr.finish()
        with contextlib.redirect_stdout(io.StringIO()):
            val = evaluate.validate_partseg(test_loader, m2, criterion, a)
        is_best = val["mean_class_iou"] > best_mean_class_iou
        best_test_acc = max(val["acc"], best_test_acc)
        best_mean_class_iou = max(val["mean_class_iou"], best_mean_class_iou)
        best_mean_inst_iou = max(val["mean_inst_iou"], best_mean_inst_iou)
        if is_best:
            best_epoch = epoch
        want.append({"train_loss": sums["loss"] / sums["count"], "train_acc": sums["acc"] / sums["count"],
                     "train_lr": tr.optimizer.param_groups[0]["lr"], "train_logit_scale": logit_scale,
                     **{f"test_{k}": v for k, v in val.items()}, "best_test_acc": best_test_acc,
                     "best_mean_inst_iou": best_mean_inst_iou, "test_mean_inst_iou": val["mean_inst_iou"],
                     "best_mean_class_iou": best_mean_class_iou, "test_mean_class_iou": val["mean_class_iou"], "best_epoch": best_epoch})
    print(log)
    assert _same(log, want), (log, want)
    assert all(np.isfinite(e["train_loss"]) and 0 <= e["train_acc"] <= 1 and np.isfinite(e["test_loss"]) for e in log)
    assert all(e["test_n"] == 3 and np.isfinite(e["test_mean_inst_iou"]) for e in log)
    # (:119's max(nan, 0) is nan: the reference's best figure is lost with the first such epoch, and so is this run's)
    assert math.isnan(log[-1]["test_mean_class_iou"]) and log[-1]["best_epoch"] == -1 and math.isnan(log[-1]["best_mean_class_iou"])
    assert not os.path.exists(os.path.join(str(tmp_path), "partseg", "t", "checkpoint_best.pt"))


def test_run_partseg_writes_the_part_seg_payload(tmp_path):
    """one test cloud per category (mean_class_iou is a number), 2 train clouds, 1 epoch: the best rule fires and the payload has
    main_partseg.py:134-143's keys"""
    from ppt_amd import partseg
    from ppt_amd.train import load_prompt_checkpoint
    c2p = partseg.shapenetpart_category2part()
    m, names = _partseg_model()
    train_set, test_set = _partseg_sets([1100, 1024], [3, 12], [1024] * 16, list(range(16)), c2p, seed=9)
    torch.manual_seed(1)
    with contextlib.redirect_stdout(io.StringIO()):
        log = partseg.run_partseg(m, train_set, test_set, _partseg_args(names, c2p, str(tmp_path), epochs=1, batch_size=8))
    assert len(log) == 1 and log[0]["best_epoch"] == 0 and log[0]["test_mean_class_iou"] > 0
    assert log[0]["best_mean_class_iou"] == log[0]["test_mean_class_iou"] and log[0]["best_test_acc"] == log[0]["test_acc"]
    ckpt = torch.load(os.path.join(str(tmp_path), "partseg", "t", "checkpoint_best.pt"), weights_only=False)
    assert set(ckpt) == PARTSEG_KEYS
    assert ckpt['epoch'] == 1 and ckpt['best_test_acc'] == log[0]["best_test_acc"]
    assert ckpt['best_mean_class_iou'] == log[0]["best_mean_class_iou"] and ckpt['best_mean_inst_iou'] == log[0]["best_mean_inst_iou"]
    assert torch.equal(ckpt['state_dict_prompt']['learnable_tokens'].cuda(), m.prompt_learner.learnable_tokens.detach())
    m2, _ = _partseg_model()
    load_prompt_checkpoint(m2, ckpt)
    assert torch.equal(m2.point_encoder.state_dict()['conv1.weight'].cpu(), ckpt['state_dict_partseg']['conv1.weight'].cpu())


class _StubTrainer:
    """Trainer's surface as run_cls uses it; hands out a NaN loss in its first step"""

    def __init__(self, num_classes):
        self.optimizer = SimpleNamespace(param_groups=[{"lr": 1e-3}])
        self.lr_schedule, self.it, self.extra_inputs = None, 0, ()
        self.steps, self.finished, self.num_classes = 0, 0, num_classes

    def step(self, pc, label):
        self.steps += 1
        loss = torch.tensor(float("nan") if self.steps == 1 else 1.0, dtype=torch.float32, device=pc.device)
        return loss, torch.zeros((pc.shape[0], self.num_classes), device=pc.device)

    def finish(self):
        self.finished += 1


class _StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.logit_scale = torch.nn.Parameter(torch.ones([]), requires_grad=False)

    def forward(self, pc):
        raise AssertionError("the run went on to validate after a non-finite loss")


def test_run_cls_stops_at_the_end_of_an_epoch_that_met_a_nan_loss(tmp_path):
    """the reference stops inside the step (main_cls.py:205-207); this run at the end of that epoch: every planned step ran, finish()
    was called, FloatingPointError is raised before validation and nothing is written"""
    from ppt_amd import recognition
    from ppt_amd.data import DeviceCloudSet
    pc, _ = W.synth_clouds(8, 1024, seed=5)
    train_set, test_set = DeviceCloudSet(pc[:6], np.array([0, 1, 2, 0, 1, 2])), DeviceCloudSet(pc[6:], np.array([0, 1]))
    args = SimpleNamespace(classnames=["a", "b", "c"], epochs=2, batch_size=2, npoints=1024, recipe="modelnet", gpu=0,
                           update_freq=2, output_dir=str(tmp_path), proj_name="cls", exp_name="nan")
    tr = _StubTrainer(3)
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(FloatingPointError, match="not finite in 1 of 3 steps"):
        recognition.run_cls(_StubModel().cuda(), train_set, test_set, args, trainer=tr)      # (step 1 is un-metered: still checked)
    assert tr.steps == 3 and tr.finished == 1
    assert not os.path.exists(os.path.join(str(tmp_path), "cls", "nan", "checkpoint_best.pt"))
