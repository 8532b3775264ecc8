"""The few-shot protocol of main_fewshot.py on the device: a K-shot training set drawn as the `*_fs` datasets draw it, the
finetuning loop, validation every epoch, the best checkpoint.

    train_set = DeviceCloudSet(points, labels).subset(fewshot_indices(labels, args.nshots, seed=args.seed))
    log = run_fewshot(model, train_set, test_set, args)             # one dict per epoch: the reference's log line
    python -m ppt_amd.fewshot --train train.npz --test test.npz --dataset_name modelnet40_fs --nshots 16 --head_type 2 ...

Every piece is the package's own: DeviceBatchLoader (the recipe's sampling and augmentation on the device), train.Trainer with
train.cosine_scheduler (main_fewshot.py:90-91, :182-184), evaluate.validate (:111), train.checkpoint_payload (:127-135).
No W&B, no pueue.  The tokenizer's BatchNorm statistics keep moving while the prompt trains, so every
validation runs the whole point tower: nothing of it is cached across epochs.
"""
import argparse
import os

import numpy as np
import torch

from .data import DeviceBatchLoader, DeviceCloudSet
from .data.fewshot import fewshot_indices
from .evaluate import validate
from .train import Trainer, checkpoint_payload, cosine_scheduler

DEFAULTS = dict(epochs=250, start_epoch=0, batch_size=64, npoints=8192, lr=3e-3, lr_start=1e-6, lr_end=1e-5, warmup_epochs=1,
                wd=0.1, betas=(0.9, 0.98), eps=1e-8, label_smoothing=0.3, seed=0, head_type=0, recipe="modelnet",
                output_dir=None, proj_name="fewshot", exp_name="run", gpu=0)          # parser.py's defaults


def _arg(args, name):
    return getattr(args, name, DEFAULTS[name])


def run_fewshot(model, train_set, test_set, args, trainer=None):
    """main_fewshot.py:81-141.  train_set / test_set: DeviceCloudSets (train_set usually a `subset` of fewshot_indices); args: the
    reference's names (epochs, batch_size, npoints, lr, lr_start, lr_end, warmup_epochs, wd, betas, eps, label_smoothing, seed,
    head_type, output_dir, proj_name, exp_name, classnames) plus `recipe` ("modelnet" | "scanobjectnn"); absent ones take
    parser.py's defaults.  -> one dict per epoch: train_loss, train_acc (the means of the per-batch figures, read from the device
    once per epoch), test_acc, test_loss, epoch, best_acc, best_epoch.  On a new best (acc > best_acc) the reference's payload is
    written to <output_dir>/<proj_name>/<exp_name>/checkpoint_best.pt (nothing is written when output_dir is None)."""
    recipe = _arg(args, "recipe")
    if recipe not in ("modelnet", "scanobjectnn"):
        raise ValueError(f"run_fewshot: recipe must be 'modelnet' or 'scanobjectnn', got {recipe!r}")
    epochs, batch_size, npoints, seed = (int(_arg(args, k)) for k in ("epochs", "batch_size", "npoints", "seed"))
    # (ragged: a set that carries lengths may hold clouds of differing length; the loader's one FPS launch then takes them)
    train_loader = DeviceBatchLoader(train_set, batch_size, npoints, recipe, train=True, shuffle=True, drop_last=False, seed=seed,
                                     ragged=train_set.lengths is not None)
    test_loader = DeviceBatchLoader(test_set, batch_size, npoints, recipe, train=False, shuffle=False, drop_last=False, seed=seed,
                                    ragged=test_set.lengths is not None)
    smoothing = float(_arg(args, "label_smoothing"))
    criterion = torch.nn.CrossEntropyLoss(label_smoothing=smoothing)                      # main_fewshot.py:52
    if trainer is None:
        schedule = cosine_scheduler(_arg(args, "lr"), _arg(args, "lr_end"), epochs, len(train_loader),
                                    warmup_epochs=_arg(args, "warmup_epochs"), start_warmup_value=_arg(args, "lr_start"))
        trainer = Trainer(model, lr=_arg(args, "lr"), betas=tuple(_arg(args, "betas")), eps=_arg(args, "eps"), wd=_arg(args, "wd"),
                          label_smoothing=smoothing, lr_schedule=schedule)
    if not hasattr(args, "gpu"):
        args.gpu = DEFAULTS["gpu"]
    out_dir = _arg(args, "output_dir")
    if out_dir is not None:
        out_dir = os.path.join(out_dir, _arg(args, "proj_name"), _arg(args, "exp_name"))
        os.makedirs(out_dir, exist_ok=True)
    head_type = int(_arg(args, "head_type"))
    start_epoch = int(_arg(args, "start_epoch"))
    trainer.it = start_epoch * len(train_loader)                                          # :182, it = iters_per_epoch * epoch + ...

    best_acc, best_epoch, log = 0, -1, []
    for epoch in range(start_epoch, epochs):
        train_loader.set_epoch(epoch)
        model.train()
        losses, accs = [], []
        for pc, label in train_loader:
            loss, pred = trainer.step(pc, label)
            losses.append(loss.detach().float().reshape(()))
            accs.append(torch.eq(pred.detach().argmax(dim=1), label).sum() / len(label))  # :199-201
        trainer.finish()
        figures = torch.stack([torch.stack(losses), torch.stack(accs)]).cpu().tolist()    # the epoch's one read of the train side
        val = validate(test_loader, model, criterion, args)
        acc = val["acc"]
        print(val)
        is_best = acc > best_acc
        best_acc = max(acc, best_acc)
        if is_best:
            best_epoch = epoch
            print("=> saving best checkpoint")
            if out_dir is not None:
                payload = checkpoint_payload(model, trainer.optimizer, epoch, best_acc, args, head_type=head_type)
                torch.save(payload, os.path.join(out_dir, "checkpoint_best.pt"))
        log.append({"train_loss": sum(figures[0]) / len(figures[0]), "train_acc": sum(figures[1]) / len(figures[1]),
                    "test_acc": val["acc"], "test_loss": val["loss"], "epoch": epoch, "best_acc": best_acc, "best_epoch": best_epoch})
        print(log[-1])
    return log


def _load_set(path):
    with np.load(path) as f:
        return DeviceCloudSet(np.ascontiguousarray(f["points"], dtype=np.float32), f["labels"]), np.asarray(f["labels"]).reshape(-1)


def main(argv=None):
    ap = argparse.ArgumentParser(description="few-shot prompt tuning (main_fewshot.py) on two cloud files (.npz: points [M, N, 3] "
                                             "f32, labels [M])")
    ap.add_argument("--train", required=True)
    ap.add_argument("--test", required=True)
    ap.add_argument("--dataset_name", default="modelnet40_fs")
    ap.add_argument("--proj_name", default="fewshot")
    ap.add_argument("--exp_name", default="run")
    ap.add_argument("--output_dir", default="outputs")
    ap.add_argument("--ulip2", action="store_true")
    ap.add_argument("--head_type", type=int, default=0)
    ap.add_argument("--num_learnable_prompt_tokens", type=int, default=32)
    ap.add_argument("--class_name_position", default="middle")
    ap.add_argument("--template_init", default="")
    ap.add_argument("--npoints", type=int, default=DEFAULTS["npoints"])
    ap.add_argument("--nshots", type=int, default=16)
    ap.add_argument("--lr", type=float, default=DEFAULTS["lr"])
    ap.add_argument("--label_smoothing", type=float, default=DEFAULTS["label_smoothing"])
    ap.add_argument("--epochs", type=int, default=DEFAULTS["epochs"])
    ap.add_argument("--batch_size", type=int, default=DEFAULTS["batch_size"])
    ap.add_argument("--seed", type=int, default=DEFAULTS["seed"])
    ap.add_argument("--gpu", type=int, default=0)
    args = ap.parse_args(argv)
    from .models import ULIP_models as M
    args.classnames = M.dataset_classnames(args.dataset_name)
    args.task, args.evaluate_3d = "cls", False
    args.recipe = "scanobjectnn" if args.dataset_name.startswith("scanobjectnn") else "modelnet"
    torch.cuda.set_device(args.gpu)
    torch.manual_seed(args.seed)                                                          # utils.set_random_seed
    np.random.seed(args.seed)
    model = M.ULIP_PointBERT(args).cuda()
    print(f"=> creating a {args.nshots}-Shot dataset")
    full, labels = _load_set(args.train)
    train_set = full.subset(fewshot_indices(labels, args.nshots, seed=args.seed))
    test_set, _ = _load_set(args.test)
    print('------ len(train_dataset)', len(train_set))
    print('------ len(val_dataset)', len(test_set))
    return run_fewshot(model, train_set, test_set, args)


if __name__ == "__main__":
    main()
