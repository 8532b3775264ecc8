"""The part-segmentation run of main_partseg.py on the device: the reference's loop on the package's own loader, trainer,
validation and checkpoint writer.

    log = run_partseg(model, train_set, test_set, args)             # one dict per epoch: the reference's log_stats
    python -m ppt_amd.partseg --train train.npz --test val.npz --epochs 300 --batch_size 16 --npoints 2048 ...

The reference's train() reads one label per cloud back to the host in every step (`part_label[i, 0].item()`,
main_partseg.py:220-225: B reads) to pick the category whose part range masks the arg-max, and `loss.item()` / `acc.item()` on top
(:231, :242-243).  Here the masked arg-max, the accuracy and the finite check are ONE launch per step (ops.train_meter_partseg,
csrc/meters.hip) into the epoch's device record, read once.  Loop control (runs.epoch_plan), the three stated deviations and the
shape of the run are those of ppt_amd/recognition.py.
"""
import argparse
import os

import torch

from .evaluate import part_tables, to_categorical, validate_partseg
from .recognition import (DEFAULTS as _CLS_DEFAULTS, _arg as _arg_of, _loaders, _out_dir, _train_stats, _trainer, add_common_arguments,
                          build_model, load_npz, seed_everything)
from .runs import TrainMeters, clamp_index, epoch_plan, order_draws
from .train import checkpoint_payload

DEFAULTS = dict(_CLS_DEFAULTS, recipe="shapenetpart")


def _arg(args, name):
    return _arg_of(args, name, DEFAULTS)


def shapenetpart_category2part():
    """ShapeNetPart's 16 categories and their 50 parts (data/dataset_3d.py:719-722), in the order of the one-hot label"""
    sizes = (("Airplane", 4), ("Bag", 2), ("Cap", 2), ("Car", 4), ("Chair", 4), ("Earphone", 3), ("Guitar", 3), ("Knife", 2),
             ("Lamp", 4), ("Laptop", 2), ("Motorbike", 6), ("Mug", 2), ("Pistol", 3), ("Rocket", 3), ("Skateboard", 3), ("Table", 3))
    out, first = {}, 0
    for name, n in sizes:
        out[name] = list(range(first, first + n))
        first += n
    return out


def run_partseg(model, train_set, test_set, args, trainer=None):
    """main_partseg.py:29-161.  train_set / test_set: DeviceCloudSets with `seg`; args: as for run_cls plus `category2part`
    ({category: [part ids]}, the dataset's table: it gives the one-hot width, the meter's and validate_partseg's part ranges);
    the recipe is "shapenetpart".
    Per step: trainer.extra_inputs = (to_categorical(cls_label, num_shape_classes),) (:210), trainer.it = the plan's schedule index,
    trainer.step, one meter launch with weight B (:242-243: update(val, n=batch_size)).  Per epoch: trainer.finish(), one read of
    the record (FloatingPointError as in run_cls), evaluate.validate_partseg, the best rule `mean_class_iou > best so far` from 0
    and the three best figures as :117-120 track them; on a new best checkpoint_payload(..., partseg=True, best_mean_class_iou=...,
    best_mean_inst_iou=...) written by rank 0.
    -> one dict per epoch with the reference's log_stats keys (:145-152): train_loss, train_acc, train_lr, train_logit_scale,
    test_<key> for every key validate_partseg returns, best_test_acc, best_mean_inst_iou, best_mean_class_iou, best_epoch.
    args.whole_shapes (--whole_shapes): the TEST loader yields every stored row of every shape (DeviceBatchLoader(ragged=True)) and
    acc / mean_inst_iou / mean_class_iou are over the points that exist, not over a 2048-point resample with duplicates; training
    stays on the resampled batches."""
    category2part = getattr(args, "category2part", None)
    if category2part is None:
        raise ValueError("run_partseg: args.category2part ({category: [part ids]}) is needed")
    num_shape_classes = len(category2part)
    train_loader, test_loader = _loaders(train_set, test_set, args, "shapenetpart", DEFAULTS,
                                         whole_shapes=bool(getattr(args, "whole_shapes", False)))
    criterion = torch.nn.CrossEntropyLoss(label_smoothing=float(_arg(args, "label_smoothing")))      # main_partseg.py:51
    if trainer is None:
        trainer = _trainer(model, args, len(train_loader), DEFAULTS)
    if not hasattr(args, "gpu"):
        args.gpu = DEFAULTS["gpu"]
    out_dir = _out_dir(args, DEFAULTS)
    rank, world = int(_arg(args, "rank")), int(_arg(args, "world_size"))
    data_ratio, update_freq, print_freq = float(_arg(args, "data_ratio")), int(_arg(args, "update_freq")), int(_arg(args, "print_freq"))
    meters = TrainMeters(train_set.device)
    start, count = (torch.from_numpy(t).to(train_set.device) for t in part_tables(category2part))
    schedule = getattr(trainer, "lr_schedule", None)

    best_test_acc = best_mean_class_iou = best_mean_inst_iou = 0
    best_epoch, log = -1, []
    for epoch in range(int(_arg(args, "start_epoch")), int(_arg(args, "epochs"))):
        train_loader.set_epoch(epoch)
        model.train()
        meters.reset()
        plan = epoch_plan(len(train_loader), epoch, data_ratio, update_freq)
        for (data_iter, index, metered), (pc, cls_label, part_label) in zip(plan, train_loader):
            trainer.extra_inputs = (to_categorical(cls_label, num_shape_classes),)       # :210
            trainer.it = index if schedule is None else clamp_index(index, len(schedule))
            loss, part_pred = trainer.step(pc, part_label)
            meters.partseg(part_pred, part_label, loss, start, count, float(pc.shape[0]), metered)
            order_draws(train_set.device)
            if metered and print_freq > 0 and (data_iter // update_freq) % print_freq == 0:
                print(f"Epoch: [{epoch}][{data_iter // update_freq}/{len(train_loader) // update_freq}]")     # :251-252
        trainer.finish()
        train_stats = _train_stats(meters, model, trainer, world)
        val = validate_partseg(test_loader, model, criterion, args)
        test_acc, test_mean_class_iou, test_mean_inst_iou = val["acc"], val["mean_class_iou"], val["mean_inst_iou"]
        print(val)
        is_best = test_mean_class_iou > best_mean_class_iou                              # :117-120
        best_test_acc = max(test_acc, best_test_acc)
        best_mean_class_iou = max(test_mean_class_iou, best_mean_class_iou)
        best_mean_inst_iou = max(test_mean_inst_iou, best_mean_inst_iou)
        if is_best:
            best_epoch = epoch
            print(f"=> find best Mean Class IoU `{best_mean_class_iou}` at Epoch `{epoch}`")
            print("=> saving best checkpoint")
            if out_dir is not None and rank == 0:
                payload = checkpoint_payload(model, trainer.optimizer, epoch, best_test_acc, args, partseg=True,
                                             best_mean_class_iou=best_mean_class_iou, best_mean_inst_iou=best_mean_inst_iou)
                torch.save(payload, os.path.join(out_dir, "checkpoint_best.pt"))
        log.append({**{f"train_{k}": v for k, v in train_stats.items()}, **{f"test_{k}": v for k, v in val.items()},
                    "best_test_acc": best_test_acc, "best_mean_inst_iou": best_mean_inst_iou, "test_mean_inst_iou": test_mean_inst_iou,
                    "best_mean_class_iou": best_mean_class_iou, "test_mean_class_iou": test_mean_class_iou, "best_epoch": best_epoch})
        print(log[-1])
    return log


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="prompt tuning for part segmentation (main_partseg.py) on two cloud files (.npz: "
                                             "points [M, N, 3] f32, labels [M] shape categories, seg [M, N] part labels)")
    add_common_arguments(ap, DEFAULTS)
    ap.add_argument("--model", default="ULIP_PointBERT_partseg")
    ap.add_argument("--dataset_name", default="shapenetpart")
    ap.add_argument("--whole_shapes", action="store_true",
                    help="validate on every stored point of every test shape (ragged batches) instead of a resample to --npoints")
    args = ap.parse_args(argv)
    args.betas = tuple(args.betas)
    args.task, args.evaluate_3d, args.rank, args.world_size, args.recipe = "partseg", False, 0, 1, "shapenetpart"
    args.category2part = shapenetpart_category2part()
    return args


def main(argv=None):
    args = parse_args(argv)
    from .models import ULIP_models as M
    args.classnames = M.dataset_classnames(args.dataset_name)
    torch.cuda.set_device(args.gpu)
    seed_everything(args.seed)
    model = build_model(args)
    train_set, test_set = load_npz(args.train, seg=True), load_npz(args.test, seg=True)
    print('------ len(train_dataset)', len(train_set))
    print('------ len(val_dataset)', len(test_set))
    return run_partseg(model, train_set, test_set, args)


if __name__ == "__main__":
    main()
