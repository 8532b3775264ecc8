"""Shared by tests/test_validate_cpu.py and tests/test_validate_gpu.py: the cases of tests/golden/g_validate.npz (written by the
reference's own validate functions, tests/golden/make_golden_validate.py) and the metric records of csrc/metrics.hip recomputed
with plain torch -- the integer columns exactly, the loss columns from double arithmetic."""
import collections
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g_validate.npz")
PS_CASES = ("ps_all", "ps_five", "ps_long")
CLS_CASES = ("cls40", "cls15", "cls40_one")
CLS_REC, PARTSEG_REC = 4, 32


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN, allow_pickle=False) as g:
        return {k: g[k] for k in g.files}


def category2part():
    g = fixture()
    return collections.OrderedDict((str(n), list(range(int(s), int(s) + int(c))))
                                   for n, s, c in zip(g["category2part_names"], g["category2part_start"], g["category2part_count"]))


@functools.lru_cache(maxsize=None)
def ps_case(name):
    """-> dict(logits [n, N, 50] f32, labels [n, N] i64, cls [n, 1] i64, sizes, smoothing, records [n, 32] i32 (torch))"""
    g = fixture()
    logits = torch.from_numpy(g[f"{name}_logits_q"].astype(np.float32) / 16.0)
    labels = torch.from_numpy(g[f"{name}_labels"].astype(np.int64))
    s = float(g[f"{name}_smoothing"])
    return dict(logits=logits, labels=labels, cls=torch.from_numpy(g[f"{name}_cls"].astype(np.int64)),
                sizes=[int(b) for b in g[f"{name}_sizes"]], smoothing=s, records=partseg_records(logits, labels, category2part(), s))


@functools.lru_cache(maxsize=None)
def cls_case(name):
    g = fixture()
    logits = torch.from_numpy(g[f"{name}_logits"])
    labels = torch.from_numpy(g[f"{name}_labels"].astype(np.int64))
    s = float(g[f"{name}_smoothing"])
    return dict(logits=logits, labels=labels, sizes=[int(b) for b in g[f"{name}_sizes"]], smoothing=s,
                classnames=[str(n) for n in g[f"{name}_classnames"]], records=cls_records(logits, labels, s))


def row_losses(logits, labels, smoothing):
    """(1 - s)(lse - x_t) + s (lse - mean_c x_c) per row, in double"""
    x = logits.double()
    lse = torch.logsumexp(x, dim=-1)
    xt = x.gather(-1, labels.unsqueeze(-1)).squeeze(-1)
    return (1.0 - smoothing) * (lse - xt) + smoothing * (lse - x.mean(dim=-1))


def _f32_bits(t):
    return t.float().contiguous().view(torch.int32)


def cls_records(logits, labels, smoothing):
    """what ppt_cls_metrics writes: [B, 4] int32 = loss bits, rank of the target (larger logits + equal logits at a lower
    index), flags (0: finite rows, valid labels), label"""
    B, C = logits.shape
    xt = logits.gather(1, labels.view(-1, 1))
    idx = torch.arange(C).view(1, -1)
    rank = ((logits > xt) | ((logits == xt) & (idx < labels.view(-1, 1)))).sum(1)
    rec = torch.zeros((B, CLS_REC), dtype=torch.int32)
    rec[:, 0] = _f32_bits(row_losses(logits, labels, smoothing))
    rec[:, 1] = rank.int()
    rec[:, 3] = labels.int()
    return rec


def partseg_records(logits, labels, c2p, smoothing):
    """what ppt_partseg_metrics writes: [n, 32] int32 (layout: include/ppt_hip.h), with main_partseg.py:300-305's own statements
    for the prediction"""
    n, N, P = logits.shape
    by_part = {p: parts for parts in c2p.values() for p in parts}
    rec = torch.zeros((n, PARTSEG_REC), dtype=torch.int32)
    loss = row_losses(logits, labels, smoothing).sum(1)
    rec[:, 4] = _f32_bits(loss)
    for i in range(n):
        parts = by_part[int(labels[i, 0])]
        pred = torch.argmax(logits[i][:, parts], dim=1) + parts[0]
        gt = labels[i]
        rec[i, 0], rec[i, 1], rec[i, 2] = parts[0], len(parts), int((pred == gt).sum())
        rec[i, 5] = (N + 255) // 256
        for j, part in enumerate(parts):
            rec[i, 8 + 3 * j] = int((gt == part).sum())
            rec[i, 9 + 3 * j] = int((pred == part).sum())
            rec[i, 10 + 3 * j] = int(((gt == part) & (pred == part)).sum())
    return rec


def loss_bound(name):
    """the issue's bound on |loss - fp64 loss|: 4 x the reference's own recorded |fp32 - fp64| deviation, floor 1e-6 relative"""
    g = fixture()
    return max(4.0 * float(g[f"{name}_loss_dev"]), 1e-6 * abs(float(g[f"{name}_loss64"])))


def same_bits(a, b):
    """float equality that treats NaN as equal to NaN (mean_class_iou of a validation set that lacks a category)"""
    return np.array_equal(np.float64(a), np.float64(b), equal_nan=True)


def check_partseg_figures(name, out, report=print):
    g = fixture()
    dev = abs(out["loss"] - float(g[f"{name}_loss64"]))
    report(f"VALIDATE {name}: |loss - fp64| = {dev:.3g} (bound {loss_bound(name):.3g}, the reference's own {float(g[f'{name}_loss_dev']):.3g})")
    for k in ("acc", "mean_inst_iou", "mean_class_iou"):
        assert same_bits(out[k], g[f"{name}_{k}"]), (name, k, out[k], float(g[f"{name}_{k}"]))
    assert list(out["category_ious"]) == list(category2part())
    assert same_bits(list(out["category_ious"].values()), g[f"{name}_category_ious"]), (name, out["category_ious"])
    assert dev <= loss_bound(name), (name, out["loss"], float(g[f"{name}_loss64"]), dev)


def check_cls_figures(name, out, report=print):
    g = fixture()
    dev = abs(out["loss"] - float(g[f"{name}_loss64"]))
    report(f"VALIDATE {name}: |loss - fp64| = {dev:.3g} (bound {loss_bound(name):.3g}, the reference's own {float(g[f'{name}_loss_dev']):.3g})")
    assert same_bits(out["acc"], g[f"{name}_acc"]), (name, out["acc"], float(g[f"{name}_acc"]))
    names, values = (str(s) for s in g[f"{name}_per_class"])           # the two lines main_cls.py:294-295 prints
    assert ','.join(out["per_class_acc"].keys()) == names
    assert ','.join(str(v) for v in out["per_class_acc"].values()) == values
    assert dev <= loss_bound(name), (name, out["loss"], float(g[f"{name}_loss64"]), dev)
