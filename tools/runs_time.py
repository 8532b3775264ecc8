"""The numbers of profiles/r25_runs.md: the training meters alone, and run_cls / run_partseg beside the same loops written out with the
reference's host reads (loss.item() per step, one .item() per cloud).  Synthetic weights and clouds; epoch 0 (graph capture, the
gradient self-check) is left out of the averages.

    python tools/runs_time.py [meters|cls|partseg|all]          # one JSON line per figure
"""
import contextlib
import io
import json
import math
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ppt_amd import evaluate, ops, partseg, recognition, runs      # noqa: E402
from ppt_amd import weights as W                                   # noqa: E402
from ppt_amd.data import DeviceBatchLoader, DeviceCloudSet         # noqa: E402
from ppt_amd.models import ULIP_models as M                        # noqa: E402
from ppt_amd.train import Trainer, cosine_scheduler                # noqa: E402

EPOCHS = 4


def out(**kw):
    print(json.dumps(kw), flush=True)


def time_launches(fn, n=300):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    host = (time.perf_counter() - t0) / n
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n, host * 1e6


def meters_alone():
    g = torch.Generator().manual_seed(0)
    rec = torch.zeros(8, dtype=torch.float64, device="cuda")
    loss = torch.tensor(1.5, device="cuda")
    logits, y = torch.randn(32, 40, generator=g).cuda(), torch.randint(0, 40, (32,), generator=g).cuda()
    us, host = time_launches(lambda: ops.train_meter_cls(logits, y, loss, rec, 1.0, True))
    out(what="train_meter_cls B=32 C=40", gpu_us_per_call_back_to_back=us, host_us_per_call=host)
    c2p = partseg.shapenetpart_category2part()
    start, count = (torch.from_numpy(t).cuda() for t in evaluate.part_tables(c2p))
    scratch = torch.zeros(4, dtype=torch.int32, device="cuda")
    logits = torch.randn(16, 2048, 50, generator=g).cuda()
    labels = torch.randint(12, 16, (16, 2048), generator=g).cuda()
    us, host = time_launches(lambda: ops.train_meter_partseg(logits, labels, loss, start, count, rec, scratch, 16.0, True))
    out(what="train_meter_partseg B=16 N=2048 P=50", gpu_us_per_call_back_to_back=us, host_us_per_call=host)
    # what run_fewshot does per step instead (two ATen reductions + the stack at the end), for scale
    us, host = time_launches(lambda: torch.eq(logits[0, :32, :40].argmax(dim=1), y).sum() / 32)
    out(what="ATen argmax/eq/sum/div B=32 C=40", gpu_us_per_call_back_to_back=us, host_us_per_call=host)


def cls_model():
    names = M.dataset_classnames("modelnet40")
    args = SimpleNamespace(classnames=names, template_init='', class_name_position='middle', num_learnable_prompt_tokens=32, gpu=0,
                           task='cls', head_type=0, evaluate_3d=False, ulip2=False, synthetic_weights=True)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.ULIP_PointBERT(args)
    m.load_state_dict(W.ulip_pointbert_state_dict(seed=0), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding(40, seed=0)
    return m.cuda(), names


def partseg_model():
    args = SimpleNamespace(classnames=M.dataset_classnames("shapenetpart"), template_init='', class_name_position='middle',
                           num_learnable_prompt_tokens=32, gpu=0, task='partseg', head_type=0, evaluate_3d=False, ulip2=False,
                           synthetic_weights=True)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.ULIP_PointBERT_partseg(args)
    m.load_state_dict(W.ulip_partseg_state_dict(seed=0), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding(50, seed=0)
    return m.cuda(), args.classnames


class Stamps:
    """wraps validate: the time it is entered (the epoch's training side is complete: its figures have been read) and left"""

    def __init__(self, fn):
        self.fn, self.enter, self.leave = fn, [], []

    def __call__(self, *a, **k):
        torch.cuda.synchronize()
        self.enter.append(time.perf_counter())
        r = self.fn(*a, **k)
        torch.cuda.synchronize()
        self.leave.append(time.perf_counter())
        return r


def report(what, t0, st, clouds):
    train = [st.enter[0] - t0] + [st.enter[i] - st.leave[i - 1] for i in range(1, len(st.enter))]
    steady = train[1:]
    out(what=what, train_seconds_per_epoch=train, steady_mean_s=sum(steady) / len(steady), steady_best_s=min(steady),
        clouds_per_s_mean=clouds / (sum(steady) / len(steady)), clouds_per_s_best=clouds / min(steady),
        validate_seconds=[b - a for a, b in zip(st.enter, st.leave)])


def cls_runs():
    B, n_train, n_test = 32, 640, 64
    pc, _ = W.synth_clouds(n_train + n_test, 1024, seed=3)
    rs = np.random.RandomState(0)
    ytr, yte = rs.randint(0, 40, n_train), rs.randint(0, 40, n_test)

    def args_for(names):
        return SimpleNamespace(classnames=names, epochs=EPOCHS, batch_size=B, npoints=1024, label_smoothing=0.2, seed=0, head_type=0,
                               recipe="modelnet", gpu=0, output_dir=None)

    # run_cls
    m, names = cls_model()
    st = recognition.validate = Stamps(evaluate.validate)
    torch.manual_seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        log = recognition.run_cls(m, DeviceCloudSet(pc[:n_train], ytr), DeviceCloudSet(pc[n_train:], yte), args_for(names))
    recognition.validate = evaluate.validate
    report("run_cls C2 shape (B=32, 1024 pts, 40 classes, head_type 0, 20 steps/epoch)", t0, st, n_train)
    out(what="run_cls log", train_loss=[e["train_loss"] for e in log], train_acc=[e["train_acc"] for e in log])

    # the written-out loop: loss.item() and acc.item() per step (main_cls.py:205, :216-217)
    del m
    m, names = cls_model()
    a = args_for(names)
    train_loader = DeviceBatchLoader(DeviceCloudSet(pc[:n_train], ytr), B, 1024, "modelnet", train=True, shuffle=True, seed=0)
    test_loader = DeviceBatchLoader(DeviceCloudSet(pc[n_train:], yte), B, 1024, "modelnet", train=False, shuffle=False, seed=0)
    sched = cosine_scheduler(3e-3, 1e-5, EPOCHS, len(train_loader), warmup_epochs=1, start_warmup_value=1e-6)
    tr = Trainer(m, lr=3e-3, label_smoothing=0.2, lr_schedule=sched)
    criterion = torch.nn.CrossEntropyLoss(label_smoothing=0.2)
    st = Stamps(evaluate.validate)
    torch.manual_seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = []
    with contextlib.redirect_stdout(io.StringIO()):
        for epoch in range(EPOCHS):
            train_loader.set_epoch(epoch)
            m.train()
            s = c = 0
            for data_iter, (x, y) in enumerate(train_loader):
                tr.it = len(train_loader) * epoch + data_iter
                loss, pred = tr.step(x, y)
                acc = torch.eq(pred.argmax(dim=1), y).sum() / len(y)
                if not math.isfinite(loss.item()):
                    raise FloatingPointError
                s += loss.item()
                acc.item()
                c += 1
            tr.finish()
            losses.append(s / c)
            st(test_loader, m, criterion, a)
    report("written-out loop with the reference's host reads, C2 shape", t0, st, n_train)
    out(what="written-out log", train_loss=losses)


def partseg_runs():
    B, N, n_train, n_test = 16, 2048, 192, 16
    c2p = partseg.shapenetpart_category2part()
    part2cat = {p: c for c, parts in c2p.items() for p in parts}
    parts = list(c2p.values())
    pc, _ = W.synth_clouds(n_train + n_test, N, seed=4)
    rs = np.random.RandomState(1)
    cats = np.concatenate([rs.randint(0, 16, n_train), np.arange(16)])
    seg = np.stack([rs.randint(parts[c][0], parts[c][-1] + 1, N) for c in cats]).astype(np.int32)

    def sets():
        return (DeviceCloudSet(pc[:n_train], cats[:n_train], seg=seg[:n_train]), DeviceCloudSet(pc[n_train:], cats[n_train:], seg=seg[n_train:]))

    def args_for(names):
        return SimpleNamespace(classnames=names, category2part=c2p, epochs=EPOCHS, batch_size=B, npoints=N, label_smoothing=0.2, seed=0,
                               gpu=0, output_dir=None)

    m, names = partseg_model()
    st = partseg.validate_partseg = Stamps(evaluate.validate_partseg)
    train_set, test_set = sets()
    torch.manual_seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        log = partseg.run_partseg(m, train_set, test_set, args_for(names))
    partseg.validate_partseg = evaluate.validate_partseg
    report("run_partseg C5 per-GPU shape (B=16, 2048 pts, 50 parts, 12 steps/epoch)", t0, st, n_train)
    out(what="run_partseg log", train_loss=[e["train_loss"] for e in log], train_acc=[e["train_acc"] for e in log],
        precision=getattr(m, "precision_name", None))

    del m
    m, names = partseg_model()
    a = args_for(names)
    train_set, test_set = sets()
    train_loader = DeviceBatchLoader(train_set, B, N, "shapenetpart", train=True, shuffle=True, seed=0)
    test_loader = DeviceBatchLoader(test_set, B, N, "shapenetpart", train=False, shuffle=False, seed=0)
    sched = cosine_scheduler(3e-3, 1e-5, EPOCHS, len(train_loader), warmup_epochs=1, start_warmup_value=1e-6)
    tr = Trainer(m, lr=3e-3, label_smoothing=0.2, lr_schedule=sched)
    criterion = torch.nn.CrossEntropyLoss(label_smoothing=0.2)
    st = Stamps(evaluate.validate_partseg)
    torch.manual_seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = []
    with contextlib.redirect_stdout(io.StringIO()):
        for epoch in range(EPOCHS):
            train_loader.set_epoch(epoch)
            m.train()
            s = c = 0
            for data_iter, (x, cls_label, part_label) in enumerate(train_loader):
                tr.extra_inputs = (evaluate.to_categorical(cls_label, 16),)
                tr.it = len(train_loader) * epoch + data_iter
                loss, part_pred = tr.step(x, part_label)
                refined = torch.zeros(B, N, dtype=torch.int32, device="cuda")
                for i in range(x.shape[0]):                        # main_partseg.py:220-225: one host read per cloud
                    p_ = c2p[part2cat[part_label[i, 0].item()]]
                    refined[i, :] = torch.argmax(part_pred[i, :, :][:, p_], dim=1) + p_[0]
                acc = torch.eq(refined, part_label).sum() / (B * N)
                if not math.isfinite(loss.item()):
                    raise FloatingPointError
                s += loss.item() * B
                acc.item()
                c += B
            tr.finish()
            losses.append(s / c)
            st(test_loader, m, criterion, a)
    report("written-out loop with the reference's host reads, C5 per-GPU shape", t0, st, n_train)
    out(what="written-out log", train_loss=losses, precision=getattr(m, "precision_name", None))


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    out(device=torch.cuda.get_device_name(0), torch=torch.__version__)
    if which in ("all", "meters"):
        meters_alone()
    if which in ("all", "cls"):
        cls_runs()
    if which in ("all", "partseg"):
        partseg_runs()
