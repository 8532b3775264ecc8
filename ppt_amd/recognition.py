"""The recognition run of main_cls.py on the device: the reference's loop (data_ratio, update_freq, --optim, the best-accuracy
checkpoint) on the package's own loader, trainer, validation and checkpoint writer.

    log = run_cls(model, train_set, test_set, args)                 # one dict per epoch: the reference's log_stats
    python -m ppt_amd.recognition --train train.npz --test test.npz --model ULIP_PointBERT --dataset_name modelnet40 \
        --head_type 2 --data_ratio 0.3 ...

Every piece is the package's own: DeviceBatchLoader (the recipe's sampling and augmentation on the device), runs.epoch_plan (which
batches run, which schedule entry they read, which are metered), train.Trainer with train.cosine_scheduler (main_cls.py:90-91),
evaluate.validate (:111), train.checkpoint_payload (:129-137).  The reference reads `loss.item()` and `acc.item()` back in every
step (:205, :216-217); each read drains the two-stream schedule Trainer.step sets up.  Here a step's figures are folded into a
device record by ONE launch (ops.train_meter_cls, csrc/meters.hip) and the epoch's training side costs one host read.

Deviations from the reference, all three stated where they are made:
  * a schedule index past the end (n_batches % update_freq != 0, last epoch: IndexError there) reads the last entry (runs.epoch_plan);
  * a non-finite loss stops the run at the END of its epoch, not inside the step (the finite check is the record's, read once);
  * --optim adam steps on the AdamW kernels with weight_decay = 0 (train.Trainer).
No W&B, no pueue.
"""
import argparse
import os

import numpy as np
import torch

from .data import DeviceBatchLoader, DeviceCloudSet
from .evaluate import validate
from .runs import TrainMeters, clamp_index, epoch_plan, gather_sums, meter_average, order_draws
from .train import Trainer, checkpoint_payload, cosine_scheduler

DEFAULTS = dict(epochs=250, start_epoch=0, batch_size=64, npoints=8192, lr=3e-3, lr_start=1e-6, lr_end=1e-5, warmup_epochs=1,
                wd=0.1, betas=(0.9, 0.98), eps=1e-8, label_smoothing=0.3, seed=0, head_type=0, recipe="modelnet", use_height=False,
                data_ratio=1.0, update_freq=1, optim="adamw", print_freq=10, rank=0, world_size=1,
                output_dir=None, proj_name="L2P3D", exp_name="", gpu=0)                  # parser.py's defaults
RECIPES = ("modelnet", "scanobjectnn", "shapenet55")


def _arg(args, name, defaults=DEFAULTS):
    return getattr(args, name, defaults[name])


def _loaders(train_set, test_set, args, recipe, defaults, whole_shapes=False):
    batch_size, npoints, seed, rank, world = (int(_arg(args, k, defaults)) for k in ("batch_size", "npoints", "seed", "rank", "world_size"))
    kw = dict(drop_last=False, seed=seed, rank=rank, world_size=world, use_height=bool(_arg(args, "use_height", defaults)))
    # main_cls.py:74-87; the test split is walked in its stored order, as run_fewshot walks it (the reference shuffles it too, which
    # moves no figure but the order of the per-class table)
    # a set that carries lengths may hold clouds of differing length: the loader's one FPS launch then takes them (ragged=True)
    # part-seg: its sets are resampled to npoints rows whatever their lengths; whole_shapes puts the TEST loader into the
    # whole-shape mode (every stored row, batches that carry lengths) and leaves training on the resampled batches
    part = recipe == "shapenetpart"
    return (DeviceBatchLoader(train_set, batch_size, npoints, recipe, train=True, shuffle=True,
                              ragged=train_set.lengths is not None and not part, **kw),
            DeviceBatchLoader(test_set, batch_size, npoints, recipe, train=False, shuffle=False,
                              ragged=bool(whole_shapes) if part else test_set.lengths is not None, **kw))


def _trainer(model, args, n_batches, defaults):
    """main_cls.py:54-60, :90-91: the optimizer --optim names and the schedule over epochs * (n_batches // update_freq) entries"""
    epochs, update_freq, world = int(_arg(args, "epochs", defaults)), int(_arg(args, "update_freq", defaults)), int(_arg(args, "world_size", defaults))
    lr = _arg(args, "lr", defaults)
    schedule = cosine_scheduler(lr, _arg(args, "lr_end", defaults), epochs, n_batches // update_freq,
                                warmup_epochs=_arg(args, "warmup_epochs", defaults), start_warmup_value=_arg(args, "lr_start", defaults))
    return Trainer(model, lr=lr, betas=tuple(_arg(args, "betas", defaults)), eps=_arg(args, "eps", defaults), wd=_arg(args, "wd", defaults),
                   label_smoothing=float(_arg(args, "label_smoothing", defaults)), lr_schedule=schedule,
                   optim=_arg(args, "optim", defaults), distributed=world > 1)


def _out_dir(args, defaults):
    out_dir = _arg(args, "output_dir", defaults)
    if out_dir is not None:
        out_dir = os.path.join(out_dir, _arg(args, "proj_name", defaults), _arg(args, "exp_name", defaults))
        if int(_arg(args, "rank", defaults)) == 0:
            os.makedirs(out_dir, exist_ok=True)
    return out_dir


def _train_stats(meters, model, trainer, world_size):
    """The end of train() (main_cls.py:231-234): THE read of the epoch's train side -- the record and, in the same copy, the logit
    scale (:214; frozen in every PPT configuration, so its value at the end of the epoch is the last metered step's)."""
    fig = meters.read(extra=model.logit_scale.detach().exp())     # raises FloatingPointError: a non-finite loss, a label out of range
    out = {}
    for key, total in (("loss", fig["loss_sum"]), ("acc", fig["acc_sum"])):
        world = gather_sums(total, fig["weight"], world_size)
        out[key] = (meter_average(total, fig["weight"], world) if fig["weight"] or world else 0)          # AverageMeter.reset: avg = 0
    out["lr"] = trainer.optimizer.param_groups[0]["lr"]
    out["logit_scale"] = fig["extra"][0]
    return out


def run_cls(model, train_set, test_set, args, trainer=None):
    """main_cls.py:30-152.  train_set / test_set: DeviceCloudSets; args: the reference's names (epochs, start_epoch, batch_size,
    npoints, lr, lr_start, lr_end, warmup_epochs, wd, betas, eps, label_smoothing, seed, head_type, data_ratio, update_freq, optim,
    print_freq, rank, world_size, use_height, output_dir, proj_name, exp_name, classnames) plus `recipe` ("modelnet" |
    "scanobjectnn" | "shapenet55"); absent ones take parser.py's defaults.  Any ULIP_* recognition factory's model works
    (ULIP_PN_NEXT with use_height).
    Per step: trainer.it = the plan's schedule index (clamped to the schedule), trainer.step, one meter launch with weight 1
    (:216-217).  Per epoch: trainer.finish(), one read of the record -- FloatingPointError if a loss was not finite (:205-207; the
    reference stops inside that step, this run at the end of its epoch) or a label left [0, C) -- then evaluate.validate, the
    best-accuracy rule (:115-116) and, on a new best, checkpoint_payload(..., head_type=...) written by rank 0 to
    <output_dir>/<proj_name>/<exp_name>/checkpoint_best.pt (nothing is written when output_dir is None).
    -> one dict per epoch with the reference's log_stats keys (:139-143): train_loss, train_acc, train_lr, train_logit_scale,
    test_<key> for every key validate returns, epoch, best_acc, best_epoch."""
    recipe = _arg(args, "recipe")
    if recipe not in RECIPES:
        raise ValueError(f"run_cls: recipe must be one of {RECIPES}, got {recipe!r}")
    train_loader, test_loader = _loaders(train_set, test_set, args, recipe, DEFAULTS)
    criterion = torch.nn.CrossEntropyLoss(label_smoothing=float(_arg(args, "label_smoothing")))      # main_cls.py:52
    if trainer is None:
        trainer = _trainer(model, args, len(train_loader), DEFAULTS)
    if not hasattr(args, "gpu"):
        args.gpu = DEFAULTS["gpu"]
    out_dir = _out_dir(args, DEFAULTS)
    head_type, rank, world = int(_arg(args, "head_type")), int(_arg(args, "rank")), int(_arg(args, "world_size"))
    data_ratio, update_freq, print_freq = float(_arg(args, "data_ratio")), int(_arg(args, "update_freq")), int(_arg(args, "print_freq"))
    meters = TrainMeters(train_set.device)
    schedule = getattr(trainer, "lr_schedule", None)

    best_acc, best_epoch, log = 0, -1, []
    for epoch in range(int(_arg(args, "start_epoch")), int(_arg(args, "epochs"))):
        train_loader.set_epoch(epoch)
        model.train()
        meters.reset()
        plan = epoch_plan(len(train_loader), epoch, data_ratio, update_freq)
        for (data_iter, index, metered), (pc, label) in zip(plan, train_loader):
            trainer.it = index if schedule is None else clamp_index(index, len(schedule))
            loss, pred = trainer.step(pc, label)
            meters.cls(pred, label, loss, 1.0, metered)                                   # :216-217: update(val), n = 1
            order_draws(train_set.device)
            if metered and print_freq > 0 and (data_iter // update_freq) % print_freq == 0:
                print(f"Epoch: [{epoch}][{data_iter // update_freq}/{len(train_loader) // update_freq}]")     # :225-229, no figure read
        trainer.finish()
        train_stats = _train_stats(meters, model, trainer, world)
        val = validate(test_loader, model, criterion, args)
        acc = val["acc"]
        print(val)
        is_best = acc > best_acc
        best_acc = max(acc, best_acc)
        if is_best:
            best_epoch = epoch
            print("=> saving best checkpoint")
            if out_dir is not None and rank == 0:                                        # utils.save_on_master
                payload = checkpoint_payload(model, trainer.optimizer, epoch, best_acc, args, head_type=head_type)
                torch.save(payload, os.path.join(out_dir, "checkpoint_best.pt"))
        log.append({**{f"train_{k}": v for k, v in train_stats.items()}, **{f"test_{k}": v for k, v in val.items()},
                    "epoch": epoch, "best_acc": best_acc, "best_epoch": best_epoch})
        print(log[-1])
    return log


def load_npz(path, seg=False):
    """A cloud file: points [M, N, 3] f32 and labels [M]; part segmentation adds seg [M, N] per-point part labels."""
    with np.load(path) as f:
        return DeviceCloudSet(np.ascontiguousarray(f["points"], dtype=np.float32), f["labels"], seg=f["seg"] if seg else None)


def add_common_arguments(ap, defaults):
    """the reference's flags (parser.py) the two runs read, with its defaults"""
    ap.add_argument("--train", required=True)
    ap.add_argument("--test", required=True)
    ap.add_argument("--output_dir", default="outputs")
    ap.add_argument("--proj_name", default=defaults["proj_name"])
    ap.add_argument("--exp_name", default=defaults["exp_name"])
    ap.add_argument("--ulip2", action="store_true")
    ap.add_argument("--use_height", action="store_true")
    ap.add_argument("--head_type", type=int, default=0, choices=[0, 1, 2, 3])
    ap.add_argument("--num_learnable_prompt_tokens", type=int, default=32)
    ap.add_argument("--class_name_position", default="end")
    ap.add_argument("--template_init", default="")
    ap.add_argument("--npoints", type=int, default=defaults["npoints"])
    ap.add_argument("--epochs", type=int, default=defaults["epochs"])
    ap.add_argument("--warmup_epochs", type=int, default=defaults["warmup_epochs"])
    ap.add_argument("--start_epoch", type=int, default=defaults["start_epoch"])
    ap.add_argument("--batch_size", type=int, default=defaults["batch_size"])
    ap.add_argument("--data_ratio", type=float, default=defaults["data_ratio"])
    ap.add_argument("--update_freq", type=int, default=defaults["update_freq"])
    ap.add_argument("--optim", default=defaults["optim"], choices=["adamw", "adam", "sgd"])
    ap.add_argument("--lr", type=float, default=defaults["lr"])
    ap.add_argument("--lr_start", type=float, default=defaults["lr_start"])
    ap.add_argument("--lr_end", type=float, default=defaults["lr_end"])
    ap.add_argument("--wd", type=float, default=defaults["wd"])
    ap.add_argument("--betas", type=float, nargs=2, default=defaults["betas"])
    ap.add_argument("--eps", type=float, default=defaults["eps"])
    ap.add_argument("--label_smoothing", type=float, default=defaults["label_smoothing"])
    ap.add_argument("--print_freq", type=int, default=defaults["print_freq"])
    ap.add_argument("--seed", type=int, default=defaults["seed"])
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--synthetic_weights", action="store_true",
                    help="build the model without the pretrained checkpoints (a smoke run; PPT_SYNTHETIC_WEIGHTS=1 does the same)")
    return ap


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="prompt tuning for recognition (main_cls.py) on two cloud files (.npz: points "
                                             "[M, N, 3] f32, labels [M])")
    add_common_arguments(ap, DEFAULTS)
    ap.add_argument("--model", default="ULIP_PN_SSG")
    ap.add_argument("--dataset_name", default="modelnet40")
    args = ap.parse_args(argv)
    args.betas = tuple(args.betas)
    args.task, args.evaluate_3d, args.rank, args.world_size = "cls", False, 0, 1
    name = args.dataset_name.lower()
    args.recipe = "scanobjectnn" if name.startswith("scanobjectnn") else "shapenet55" if name.startswith("shapenet") else "modelnet"
    return args


def seed_everything(seed):
    """utils.set_random_seed (main_cls.py:39-40; one process: rank 0)"""
    torch.manual_seed(seed)
    np.random.seed(seed)


SYNTHETIC = {"ULIP_PointBERT": "ulip_pointbert_state_dict", "ULIP_PointBERT_partseg": "ulip_partseg_state_dict",
             "ULIP_PN_NEXT": "ulip_pn_next_state_dict", "ULIP_PN_MLP": "ulip_pn_mlp_state_dict", "ULIP_PN_SSG": "ulip_pn2_ssg_state_dict",
             "ULIP_PN_MSG": "ulip_pn2_msg_state_dict"}


def build_model(args):
    """main_cls.py:43-45.  --synthetic_weights: no checkpoint is read; the model gets ppt_amd.weights' synthetic state dict, so that
    a smoke run computes on defined values"""
    from . import weights
    from .models import ULIP_models as M
    print("=> creating model: {}".format(args.model))
    model = getattr(M, args.model)(args)
    if args.synthetic_weights:
        model.load_state_dict(getattr(weights, SYNTHETIC[args.model])(seed=args.seed), strict=False)
        model.prompt_learner.embedding = weights.synth_prompt_embedding(len(args.classnames), seed=args.seed)
    return model.cuda()


def main(argv=None):
    args = parse_args(argv)
    from .models import ULIP_models as M
    args.classnames = M.dataset_classnames(args.dataset_name)
    torch.cuda.set_device(args.gpu)
    seed_everything(args.seed)
    model = build_model(args)
    train_set, test_set = load_npz(args.train), load_npz(args.test)
    print('------ len(train_dataset)', len(train_set))
    print('------ len(val_dataset)', len(test_set))
    return run_cls(model, train_set, test_set, args)


if __name__ == "__main__":
    main()
