"""GPU: DeviceCloudSet.subset and the few-shot run of ppt_amd/fewshot.py against the same loop written out with Trainer.step and
evaluate.validate, and the checkpoint it writes through its reader."""
import contextlib
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ppt_amd import weights as W

pytestmark = pytest.mark.gpu


def test_subset_follows_the_host_fancy_index():
    from ppt_amd.data import DeviceCloudSet
    rs = np.random.RandomState(2)
    lengths = np.array([40, 64, 17, 50, 33, 64], np.int32)
    clouds = [rs.randn(n, 3).astype(np.float32) for n in lengths]
    seg = [rs.randint(0, 50, n).astype(np.int32) for n in lengths]
    labels = np.array([3, 1, 4, 1, 5, 9])
    full = DeviceCloudSet(clouds, labels, seg=seg)
    pick = [4, 0, 4, 2]
    sub = full.subset(pick)
    assert isinstance(sub, DeviceCloudSet) and len(sub) == 4 and sub.device == full.device
    for name in ("points", "labels", "seg", "lengths"):
        a, b = getattr(sub, name), getattr(full, name)
        assert a.is_cuda and a.dtype == b.dtype
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()[pick]), name
    assert np.array_equal(sub.lengths_host, lengths[pick]) and np.array_equal(sub.rows(np.arange(4)), lengths[pick])
    assert len(full) == 6 and full.points.shape[0] == 6                   # the source is untouched
    plain = DeviceCloudSet(np.stack([c[:17] for c in clouds]), labels).subset(torch.tensor([5, 5]))
    assert plain.seg is None and plain.lengths is None and plain.lengths_host is None and plain.labels.tolist() == [9, 9]
    with pytest.raises(IndexError):
        full.subset([6])


def _model():
    from ppt_amd.models import ULIP_models as M
    names = M.dataset_classnames("modelnet40")[:3]
    args = SimpleNamespace(classnames=names, template_init='', class_name_position='middle', num_learnable_prompt_tokens=32, gpu=0,
                           task='cls', head_type=2, evaluate_3d=False, ulip2=False, synthetic_weights=True)
    torch.manual_seed(0)                          # (the un-frozen block is random per construction)
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.ULIP_PointBERT(args)
    m.load_state_dict(W.ulip_pointbert_state_dict(seed=0), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding(3, seed=0)
    m.cuda().set_precision("fp32")
    return m, names


def test_run_fewshot_equals_the_loop_written_out(tmp_path):
    """3 classes x 4 clouds, 2 shots, batches of 4 (one full, one of 2), 2 epochs, 5 test clouds of 1024 points, head_type 2, fp32"""
    from ppt_amd import analysis, evaluate, fewshot
    from ppt_amd.data import DeviceBatchLoader, DeviceCloudSet, fewshot_indices
    from ppt_amd.train import Trainer, cosine_scheduler
    pc, _ = W.synth_clouds(17, 1024, seed=21)
    train_labels = np.array([2, 0, 1, 1, 0, 2, 2, 1, 0, 0, 1, 2])
    test_labels = np.array([0, 1, 2, 2, 1])
    picked = fewshot_indices(train_labels, 2, seed=0)
    assert picked.shape == (6,) and train_labels[picked].tolist() == [2, 2, 0, 0, 1, 1]

    def args_for(names, out):
        return SimpleNamespace(classnames=names, epochs=2, batch_size=4, npoints=1024, lr=3e-3, lr_start=1e-6, lr_end=1e-5,
                               warmup_epochs=1, label_smoothing=0.2, seed=0, head_type=2, recipe="modelnet", gpu=0, output_dir=out,
                               proj_name="fewshot", exp_name="t")

    def sets():
        return DeviceCloudSet(pc[:12], train_labels).subset(picked), DeviceCloudSet(pc[12:], test_labels)

    # the run
    m, names = _model()
    train_set, test_set = sets()
    torch.manual_seed(1)
    with contextlib.redirect_stdout(io.StringIO()):
        log = fewshot.run_fewshot(m, train_set, test_set, args_for(names, str(tmp_path)))

    # the same loop, written out
    m2, _ = _model()
    train_set, test_set = sets()
    a = args_for(names, None)
    train_loader = DeviceBatchLoader(train_set, 4, 1024, "modelnet", train=True, shuffle=True, drop_last=False, seed=0)
    test_loader = DeviceBatchLoader(test_set, 4, 1024, "modelnet", train=False, shuffle=False, drop_last=False, seed=0)
    assert len(train_loader) == 2
    tr = Trainer(m2, lr=3e-3, label_smoothing=0.2,
                 lr_schedule=cosine_scheduler(3e-3, 1e-5, 2, 2, warmup_epochs=1, start_warmup_value=1e-6))
    criterion = torch.nn.CrossEntropyLoss(label_smoothing=0.2)
    torch.manual_seed(1)
    want, best_acc, best_epoch = [], 0, -1
    for epoch in range(2):
        train_loader.set_epoch(epoch)
        m2.train()
        losses, accs = [], []
        for x, y in train_loader:
            loss, pred = tr.step(x, y)
            losses.append(loss.item())
            accs.append((torch.eq(pred.argmax(dim=1), y).sum() / len(y)).item())
        tr.finish()
        with contextlib.redirect_stdout(io.StringIO()):
            val = evaluate.validate(test_loader, m2, criterion, a)
        if val["acc"] > best_acc:
            best_epoch = epoch
        best_acc = max(val["acc"], best_acc)
        want.append({"train_loss": sum(losses) / len(losses), "train_acc": sum(accs) / len(accs), "test_acc": val["acc"],
                     "test_loss": val["loss"], "epoch": epoch, "best_acc": best_acc, "best_epoch": best_epoch})
    print(log)
    assert log == want
    assert all(np.isfinite(e["train_loss"]) and np.isfinite(e["test_loss"]) for e in log)
    assert [e["epoch"] for e in log] == [0, 1] and tr.it == 4
    # best_epoch follows acc > best_acc, from best_acc = 0 and best_epoch = -1
    best, where = 0, -1
    for e in log:
        if e["test_acc"] > best:
            best, where = e["test_acc"], e["epoch"]
        assert (e["best_acc"], e["best_epoch"]) == (best, where)

    # the checkpoint and its reader
    path = os.path.join(str(tmp_path), "fewshot", "t", "checkpoint_best.pt")
    assert where >= 0                             # (every class is in the test set: even a constant prediction scores above 0)
    ckpt = torch.load(path, weights_only=False)
    assert set(ckpt) == {'epoch', 'state_dict', 'optimizer', 'best_acc', 'args', 'last_block', 'ppt_precision'}
    assert ckpt['epoch'] == where + 1 and ckpt['best_acc'] == best and list(ckpt['state_dict']) == ['learnable_tokens']
    assert ckpt['last_block'] is not None and 'mlp.fc2.weight' in ckpt['last_block']
    if where == 1:
        assert torch.equal(ckpt['state_dict']['learnable_tokens'].cuda(), m.prompt_learner.learnable_tokens.detach())
    with contextlib.redirect_stdout(io.StringIO()) as printed:
        rows = analysis.interpret_prompt(ckpt, m, 4)
    assert len(rows) == 32 and all(len(r[1]) == 4 for r in rows)
    ids, dist = analysis.nearest_tokens(ckpt['state_dict']['learnable_tokens'], m.token_embedding.weight, 4)
    assert [r[1] for r in rows] == ids.tolist()
    assert "32: " in printed.getvalue()
