"""CPU: the host half of ppt_amd/evaluate.py against tests/golden/g_validate.npz, which the reference's own main_cls.validate /
main_partseg.validate wrote (tests/golden/make_golden_validate.py).  The metric records the kernels of csrc/metrics.hip write are
recomputed here with plain torch (tests/validate_ref.py) and fed to the finalisation: `acc`, `mean_inst_iou`, `mean_class_iou`, the
category IoUs and the per-class accuracies must come out bit-equal to the reference's, NaN included; `loss` within 4 x the
reference's own |fp32 - fp64| deviation of the fp64 value (floor 1e-6 relative).  tests/test_validate_gpu.py checks that the
kernels write these records."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import validate_ref as V


@pytest.mark.parametrize("name", V.PS_CASES)
def test_partseg_finalisation_reproduces_the_reference(name):
    from ppt_amd import evaluate
    c = V.ps_case(name)
    N = c["logits"].shape[1]
    out = evaluate.finalize_partseg(c["records"].numpy(), [(b, N) for b in c["sizes"]], V.category2part())
    V.check_partseg_figures(name, out)
    assert set(out) >= {'acc', 'loss', 'mean_inst_iou', 'mean_class_iou', 'category_ious', 'category_counts', 'n', 'nonfinite_rows'}
    assert out["n"] == sum(c["sizes"]) == sum(out["category_counts"].values()) and out["nonfinite_rows"] == 0
    for cat, k in out["category_counts"].items():
        assert (k == 0) == bool(np.isnan(out["category_ious"][cat]))
    if name == "ps_five":
        assert np.isnan(out["mean_class_iou"]) and sum(k > 0 for k in out["category_counts"].values()) == 5
    if name == "ps_all":
        rec = c["records"]                          # the fixture does reach the IoU = 1 branch: a part absent from gt and pred
        slots = rec[:, 8:].view(-1, 8, 3)
        absent = [(int(i), j) for i in range(rec.shape[0]) for j in range(int(rec[i, 1])) if int(slots[i, j, 0]) + int(slots[i, j, 1]) == 0]
        assert absent and not np.isnan(out["mean_class_iou"])


@pytest.mark.parametrize("name", V.CLS_CASES)
def test_cls_finalisation_reproduces_the_reference(name):
    from ppt_amd import evaluate
    c = V.cls_case(name)
    out = evaluate.finalize_cls(c["records"].numpy(), c["sizes"], c["classnames"])
    V.check_cls_figures(name, out)
    assert set(out) >= {'acc', 'loss', 'per_class_acc', 'acc5', 'n', 'nonfinite_rows'}
    assert out["n"] == sum(c["sizes"]) and out["acc"] <= out["acc5"] <= 1.0 and out["nonfinite_rows"] == 0


def test_bad_label_raises_and_nonfinite_rows_are_counted():
    from ppt_amd import evaluate, ops
    c = V.cls_case("cls15")
    rec = c["records"].clone()
    rec[3, 2] = ops.METRIC_NONFINITE
    assert evaluate.finalize_cls(rec.numpy(), c["sizes"], c["classnames"])["nonfinite_rows"] == 1
    rec[5, 2] = ops.METRIC_BAD_LABEL
    with pytest.raises(ValueError, match="label"):
        evaluate.finalize_cls(rec.numpy(), c["sizes"], c["classnames"])
    p = V.ps_case("ps_five")
    rec = p["records"].clone()
    rec[2, 3] = ops.METRIC_BAD_LABEL
    with pytest.raises(ValueError, match="label"):
        evaluate.finalize_partseg(rec.numpy(), [(b, 96) for b in p["sizes"]], V.category2part())


def test_non_contiguous_parts_raise_valueerror():
    from ppt_amd import evaluate
    start, count = evaluate.part_tables(V.category2part())
    assert start.tolist()[:6] == [0, 0, 0, 0, 4, 4] and count.tolist()[:6] == [4, 4, 4, 4, 2, 2] and len(start) == 50
    with pytest.raises(ValueError, match="contiguous"):
        evaluate.PartsegMetrics({'a': [0, 1, 3], 'b': [2]}, 0.0)
    with pytest.raises(ValueError, match="contiguous"):
        evaluate.PartsegMetrics({'a': [1, 0], 'b': [2, 3]}, 0.0)


def test_criterion_other_than_the_references_raises():
    from types import SimpleNamespace
    from ppt_amd import evaluate
    args = SimpleNamespace(gpu=0)
    for crit in (torch.nn.CrossEntropyLoss(weight=torch.ones(40)), torch.nn.CrossEntropyLoss(reduction="sum"),
                 torch.nn.CrossEntropyLoss(ignore_index=3), torch.nn.NLLLoss()):
        with pytest.raises(NotImplementedError):
            evaluate.validate([], None, crit, args)
        with pytest.raises(NotImplementedError):
            evaluate.validate_partseg([], None, crit, args)


def test_surface_is_re_exported_and_rejects_cpu_tensors():
    import models.ULIP_models as models           # the reference's import line: the drop-in surface of INTEGRATION.md
    from ppt_amd import evaluate, ops
    assert models.validate is evaluate.validate and models.validate_partseg is evaluate.validate_partseg
    assert models.accuracy is evaluate.accuracy
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cls_metrics(torch.zeros(2, 5), torch.zeros(2, dtype=torch.long), 0.0, torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate.ClsMetrics(5, 0.0).update(torch.zeros(2, 5), torch.zeros(2, dtype=torch.long))


# ---- world size 2 over gloo: the figures of the union of two shards (the pattern of tests/test_dp_cpu.py) -------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard(sizes, rank):
    """rank 0 takes the first two batches, rank 1 the rest -> (first record, batch sizes)"""
    cut = min(2, len(sizes) - 1)
    return (0, sizes[:cut]) if rank == 0 else (sum(sizes[:cut]), sizes[cut:])


def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ppt_amd import evaluate
    calls = {"n": 0}
    real = dist.all_gather

    def counting(*a, **k):
        calls["n"] += 1
        return real(*a, **k)
    dist.all_gather = counting
    out = {}
    c = V.ps_case("ps_all")
    o, sizes = _shard(c["sizes"], rank)
    out["ps"] = evaluate.finalize_partseg(c["records"][o:o + sum(sizes)].numpy(), [(b, 96) for b in sizes], V.category2part(), dist.group.WORLD)
    c = V.cls_case("cls40")
    o, sizes = _shard(c["sizes"], rank)
    out["cls"] = evaluate.finalize_cls(c["records"][o:o + sum(sizes)].numpy(), sizes, c["classnames"], dist.group.WORLD, 40)
    out["collectives"] = calls["n"]
    dist.all_gather = real
    ret[rank] = out
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_two_shards_over_gloo_give_the_figures_of_the_union():
    """Integers travel as integers, so every figure that is a ratio of counts is EXACTLY the union's.  The float figures differ
    from the one-process result only in where fp32 rounds: one process holds each batch's accuracy and each mean IoU in fp32 as
    the reference does (relative 2^-24 = 6e-8 per rounding, a handful of them), the reduction carries float64 sums -- bound 1e-6."""
    from ppt_amd import evaluate
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    r0, r1 = ret[0], ret[1]
    assert r0["collectives"] == r1["collectives"] == 2          # one per result()
    for k in ("ps", "cls"):                                     # every rank ends with the same bits
        assert repr(r0[k]) == repr(r1[k]), k
    c = V.ps_case("ps_all")
    one = evaluate.finalize_partseg(c["records"].numpy(), [(b, 96) for b in c["sizes"]], V.category2part())
    two = r0["ps"]
    assert two["n"] == one["n"] == 19 and two["category_counts"] == one["category_counts"] and two["nonfinite_rows"] == 0
    assert two["acc"] == int(c["records"][:, 2].sum()) / (19 * 96)
    for k in ("acc", "loss", "mean_inst_iou", "mean_class_iou"):
        assert abs(two[k] - one[k]) <= 1e-6 * abs(one[k]), (k, two[k], one[k])
    for cat in one["category_ious"]:
        assert abs(two["category_ious"][cat] - one["category_ious"][cat]) <= 1e-6, cat
    c = V.cls_case("cls40")
    one = evaluate.finalize_cls(c["records"].numpy(), c["sizes"], c["classnames"])
    two = r0["cls"]
    assert two["n"] == one["n"] == 21 and two["acc"] == int((c["records"][:, 1] == 0).sum()) / 21
    assert two["per_class_acc"] == dict(sorted(one["per_class_acc"].items())) and list(two["per_class_acc"]) == sorted(one["per_class_acc"])
    for k in ("acc", "acc5", "loss"):
        assert abs(two[k] - one[k]) <= 1e-6 * abs(one[k]), (k, two[k], one[k])
