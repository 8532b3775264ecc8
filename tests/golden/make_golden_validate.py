#!/usr/bin/env python3
"""Generate tests/golden/g_validate.npz: what the UPSTREAM REFERENCE's own validate functions (main_cls.validate,
main_partseg.validate, imported through tests/golden/ref_import.py) return for recorded logits and labels -- the pin of
ppt_amd/evaluate.py and csrc/metrics.hip.  Build container only; only arrays and strings are stored.

    python tests/golden/make_golden_validate.py

The functions run on the CPU as they are: `wandb` is a stub in sys.modules, args.gpu = "cpu" (`.to("cpu")`; Tensor.cuda is the
identity, ref_import), torch.zeros drops its `device=` for the duration of the call (main_partseg.py:275 asks for
f'cuda:{args.gpu}'), the model is a stub that hands out the recorded logits batch by batch, and the loader is a list with a
`.dataset` that carries part2category / category2part.

Per case the file holds the logits (part-seg: int8 sixteenths, exact in fp32; recognition: fp32) and labels, the batch sizes, the
returned figures, what the reference prints per class / per category, the reference criterion applied to `.double()` logits
through the same meters (the fp64 loss), and the reference's own |fp32 - fp64| loss deviation.

Cases, aimed at the branches:
  ps_all    N = 96 (not a multiple of a wave), batches 4,4,4,4,3 over all 16 categories; odd clouds lack their category's last
            part in the labels, and every other one of them also in the predictions (union 0 -> IoU 1); every 7th point's logits
            rounded to integers (arg-max ties inside the masked range); label logits raised (accuracy neither 0 nor 1)
  ps_five   only 5 categories present (batches 4,3): NaN category IoUs and a NaN mean_class_iou; label_smoothing 0
  ps_long   N = 2048, one batch of 2: a cloud split over several workgroups
  cls40 / cls15   batches 8,8,5;   cls40_one   one batch of 1 (through the reference's pieces: see validate_batch_of_one)
"""
import argparse
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_import as R                     # noqa: E402

SEED = 20250
CATEGORY2PART = {'Airplane': [0, 1, 2, 3], 'Bag': [4, 5], 'Cap': [6, 7], 'Car': [8, 9, 10, 11], 'Chair': [12, 13, 14, 15],
                 'Earphone': [16, 17, 18], 'Guitar': [19, 20, 21], 'Knife': [22, 23], 'Lamp': [24, 25, 26, 27], 'Laptop': [28, 29],
                 'Motorbike': [30, 31, 32, 33, 34, 35], 'Mug': [36, 37], 'Pistol': [38, 39, 40], 'Rocket': [41, 42, 43],
                 'Skateboard': [44, 45, 46], 'Table': [47, 48, 49]}          # ShapeNetPart's table (the dataset's public part list)
P = 50


class _Loader(list):
    dataset = None


class _Model:
    def __init__(self, batches):
        self.batches, self.i = batches, 0

    def eval(self):
        return self

    def __call__(self, pc, *extra):
        out = self.batches[self.i]
        self.i += 1
        return out


@contextlib.contextmanager
def _zeros_without_device():
    real = torch.zeros

    def zeros(*a, **k):
        k.pop("device", None)
        return real(*a, **k)
    torch.zeros = zeros
    try:
        yield
    finally:
        torch.zeros = real


def _split(t, sizes):
    out, o = [], 0
    for b in sizes:
        out.append(t[o:o + b])
        o += b
    return out


def partseg_case(rng, cats, N, sizes):
    cat_names = list(CATEGORY2PART)
    n = sum(sizes)
    q = np.clip(np.round(rng.standard_normal((n, N, P)) * 2.0 * 16.0), -127, 127).astype(np.int8)
    labels = np.zeros((n, N), np.int64)
    cls = np.zeros((n, 1), np.int64)
    for i in range(n):
        c = cats[i % len(cats)]
        parts = CATEGORY2PART[cat_names[c]]
        cls[i, 0] = c
        usable = parts[:-1] if (i % 2 == 1 and len(parts) > 1) else parts          # odd clouds: the last part never occurs in gt
        labels[i] = rng.choice(usable, size=N)
        if i % 4 == 1:
            q[i, :, parts[-1]] = -127                                               # ... nor in the predictions: union 0
        raised = rng.random(N) < 0.6
        idx = np.nonzero(raised)[0]
        q[i, idx, labels[i, idx]] = np.clip(q[i, idx, labels[i, idx]].astype(np.int32) + 40, -127, 127).astype(np.int8)
    q[:, ::7, :] = (np.round(q[:, ::7, :].astype(np.float32) / 16.0) * 16).clip(-112, 112).astype(np.int8)      # ties
    return q, labels, cls


def run_partseg(name, q, labels, cls, sizes, smoothing, out):
    with R.reference_context():
        import main_partseg as MP
    logits = torch.from_numpy(q.astype(np.float32) / 16.0)
    lb = torch.from_numpy(labels)
    N = labels.shape[1]
    loader = _Loader((torch.zeros(b, N, 3), c, l) for b, c, l in zip(sizes, _split(torch.from_numpy(cls), sizes), _split(lb, sizes)))
    loader.dataset = types.SimpleNamespace(category2part=CATEGORY2PART,
                                           part2category={p: c for c, ps in CATEGORY2PART.items() for p in ps})
    args = argparse.Namespace(gpu="cpu", print_freq=1000)
    res = {}
    for tag, lg in (("f32", logits), ("f64", logits.double())):
        crit = torch.nn.CrossEntropyLoss(label_smoothing=smoothing)
        calls = []
        MP.print = lambda *a, **k: calls.append(a)               # the category IoUs are only printed (:354): take the tensors
        try:
            with _zeros_without_device():
                res[tag] = MP.validate(loader, _Model(_split(lg, sizes)), crit, args)
        finally:
            del MP.print
        if tag == "f32":
            cat_iou = {a[1]: float(a[3]) for a in calls if a and a[0] == 'Category:'}
    r = res["f32"]
    for k in ("acc", "loss", "mean_inst_iou", "mean_class_iou"):
        out[f"{name}_{k}"] = np.float64(r[k])
    assert list(cat_iou) == list(CATEGORY2PART)
    out[f"{name}_category_ious"] = np.array([cat_iou[c] for c in CATEGORY2PART], np.float64)
    out[f"{name}_loss64"] = np.float64(res["f64"]["loss"])
    out[f"{name}_loss_dev"] = np.float64(abs(r["loss"] - res["f64"]["loss"]))
    out[f"{name}_logits_q"] = q
    out[f"{name}_labels"] = labels.astype(np.int8)
    out[f"{name}_cls"] = cls.astype(np.int8)
    out[f"{name}_sizes"] = np.array(sizes, np.int64)
    out[f"{name}_smoothing"] = np.float64(smoothing)
    print(name, {k: r[k] for k in r}, "loss64", res["f64"]["loss"])


def validate_batch_of_one(test_loader, model, criterion, args):
    """main_cls.validate cannot run a batch of ONE sample: `correct[:1].squeeze()` (:281) is 0-dim there and `top1_accurate[idx]`
    (:283) raises IndexError.  The figures of such a batch are therefore taken from the reference's own pieces -- criterion,
    utils.accuracy, AverageMeter -- in validate's order (:266-274, :289-299), with `.reshape(-1)` in place of that squeeze."""
    with R.reference_context():
        from utils.utils import accuracy, AverageMeter
    val_top1, val_loss = AverageMeter('Acc@1', ':6.2f'), AverageMeter('Acc@5', ':6.2f')
    stats, hits = {}, {}
    with torch.no_grad():
        for pc, target, target_name in test_loader:
            pred = model(pc)
            loss = criterion(pred, target.long())
            res, correct = accuracy(pred, target, topk=(1,))
            val_loss.update(loss.item(), pc.size(0))
            val_top1.update(res[0].item(), pc.size(0))
            for idx, name in enumerate(target_name):
                stats[name] = stats.get(name, 0) + 1
                hits[name] = hits.get(name, 0) + int(correct[:1].reshape(-1)[idx].item())
    per = {k: hits[k] / stats[k] for k in stats}
    print(','.join(per.keys()))
    print(','.join([str(v) for v in per.values()]))
    print('Test * (batch of one)')
    return {'acc': val_top1.avg, 'loss': val_loss.avg}


def run_cls(name, rng, C, sizes, smoothing, out):
    with R.reference_context():
        import main_cls as MC
    n = sum(sizes)
    names = [f"class{c:02d}" for c in range(C)]
    logits = (rng.standard_normal((n, C)) * 3.0).astype(np.float32)
    labels = rng.integers(0, C, size=n).astype(np.int64)
    raised = rng.random(n) < 0.6
    logits[raised, labels[raised]] += np.float32(9.0)
    lg, lb = torch.from_numpy(logits), torch.from_numpy(labels)
    loader = _Loader((torch.zeros(b, 4, 3), l, [names[int(c)] for c in l]) for b, l in zip(sizes, _split(lb, sizes)))
    args = argparse.Namespace(gpu="cpu", print_freq=1000)
    res, lines = {}, None
    for tag, x in (("f32", lg), ("f64", lg.double())):
        crit = torch.nn.CrossEntropyLoss(label_smoothing=smoothing)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res[tag] = (validate_batch_of_one if sizes == [1] else MC.validate)(loader, _Model(_split(x, sizes)), crit, args)
        if tag == "f32":
            lines = buf.getvalue().splitlines()
    per_class = lines[-3:-1]                                     # main_cls.py:294-295: the names, then the accuracies
    assert per_class[0].startswith("class") and lines[-1].startswith("Test *"), lines[-3:]
    r = res["f32"]
    out[f"{name}_acc"] = np.float64(r["acc"])
    out[f"{name}_loss"] = np.float64(r["loss"])
    out[f"{name}_loss64"] = np.float64(res["f64"]["loss"])
    out[f"{name}_loss_dev"] = np.float64(abs(r["loss"] - res["f64"]["loss"]))
    out[f"{name}_per_class"] = np.array(per_class)
    out[f"{name}_logits"] = logits
    out[f"{name}_labels"] = labels.astype(np.int8)
    out[f"{name}_sizes"] = np.array(sizes, np.int64)
    out[f"{name}_smoothing"] = np.float64(smoothing)
    out[f"{name}_classnames"] = np.array(names)
    print(name, r, "loss64", res["f64"]["loss"], per_class)


def main():
    sys.modules.setdefault("wandb", types.ModuleType("wandb"))
    rng = np.random.default_rng(SEED)
    out = {"category2part_names": np.array(list(CATEGORY2PART)),
           "category2part_start": np.array([v[0] for v in CATEGORY2PART.values()], np.int64),
           "category2part_count": np.array([len(v) for v in CATEGORY2PART.values()], np.int64)}
    run_partseg("ps_all", *partseg_case(rng, list(range(16)), 96, [4, 4, 4, 4, 3]), [4, 4, 4, 4, 3], 0.3, out)
    run_partseg("ps_five", *partseg_case(rng, [0, 3, 4, 8, 15], 96, [4, 3]), [4, 3], 0.0, out)
    run_partseg("ps_long", *partseg_case(rng, [10, 1], 2048, [2]), [2], 0.3, out)
    run_cls("cls40", rng, 40, [8, 8, 5], 0.2, out)
    run_cls("cls15", rng, 15, [8, 8, 5], 0.2, out)
    run_cls("cls40_one", rng, 40, [1], 0.2, out)
    path = os.path.join(HERE, "g_validate.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
