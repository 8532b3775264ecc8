"""Loop control of the reference's train() (main_cls.py:155-234, main_partseg.py:164-257) as pure functions, and the device record
the two runs (ppt_amd/recognition.py, ppt_amd/partseg.py) keep their per-step figures in.

    for data_iter, schedule_index, metered in epoch_plan(len(loader), epoch, args.data_ratio, args.update_freq): ...
    avg = meter_average(rec[0], rec[2])
"""
import torch


def epoch_plan(n_batches, epoch, data_ratio=1.0, update_freq=1):
    """One entry (data_iter, schedule_index, metered) per batch the reference processes in `epoch`, in order
    (main_cls.py:160, :172-185, :209; the same lines are main_partseg.py:169, :186-200, :235):

      * batch `data_iter` runs unless data_iter > n_batches * data_ratio (:173-174).  The product is a Python float and is NOT
        rounded: 10 * 0.3 is 3.0000000000000004, so batches 0..3 run; 4 * 0.5 is 2.0, so batches 0..2 do;
      * schedule_index = (n_batches // update_freq) * epoch + data_iter // update_freq (:160, :181-183): the entry of the
        per-iteration learning-rate schedule, which has epochs * (n_batches // update_freq) entries (main_cls.py:90-91);
      * metered = (data_iter + 1) % update_freq == 0 (:209): the steps whose loss and accuracy enter the epoch's meters.

    The reference zeroes the gradients and steps the optimizer on EVERY batch (:179, :198): update_freq changes only the schedule
    index and which steps are metered.  That is reproduced as it is -- it is not gradient accumulation, and is not turned into it.

    One deviation: where n_batches % update_freq != 0 the reference indexes one past the end of its schedule in the last epoch
    and raises IndexError; the callers clamp the index to the schedule's last entry, as Trainer.step does."""
    n_batches, epoch, update_freq = int(n_batches), int(epoch), int(update_freq)
    if n_batches < 0 or epoch < 0 or update_freq < 1:
        raise ValueError("epoch_plan: n_batches >= 0, epoch >= 0, update_freq >= 1")
    iters_per_epoch = n_batches // update_freq
    limit = n_batches * data_ratio
    plan = []
    for data_iter in range(n_batches):
        if data_iter > limit:
            break
        plan.append((data_iter, iters_per_epoch * epoch + data_iter // update_freq, (data_iter + 1) % update_freq == 0))
    return plan


def clamp_index(index, length):
    """the stated deviation of epoch_plan: an index past the end of the schedule reads its last entry"""
    return min(int(index), int(length) - 1)


def meter_average(sum, count, world_sums=None):
    """AverageMeter.avg at the end of train() (utils/utils.py:333-348).  On a single process: sum / count (:337).  Under a process
    group, world_sums = every rank's [sum, count]: ProgressMeter.synchronize has all-reduced them in float64 (:342-344) and the
    meter then holds `self.sum = int(t[0])` (:346) -- the summed value TRUNCATED to an integer -- over the summed count.  The
    truncation is the reference's behaviour (its distributed train_loss / train_acc are whole numbers over the count) and is kept
    here so that the two logs agree; validate()'s figures do not go through it (ppt_amd/evaluate.py)."""
    if world_sums is None:
        return sum / count
    t = torch.tensor([[float(s), float(c)] for s, c in world_sums], dtype=torch.float64).sum(0).tolist()
    return int(t[0]) / t[1]


class TrainMeters:
    """The epoch's record on the device (ops.METER_KEYS): one meter launch per step, one read per epoch."""

    def __init__(self, device):
        from . import ops
        self.rec = torch.zeros(ops.METER_REC, dtype=torch.float64, device=device)
        self.scratch = torch.zeros(ops.METER_SCRATCH, dtype=torch.int32, device=device)      # part-seg: all zero between calls

    def reset(self):
        self.rec.zero_()

    @staticmethod
    def _loss(loss):
        loss = loss.detach()
        return loss if loss.dtype == torch.float32 and loss.is_contiguous() else loss.float().contiguous()

    @staticmethod
    def _logits(logits):
        logits = logits.detach()                              # (fp32 and contiguous in every mode today: no launch is added)
        return logits if logits.dtype == torch.float32 and logits.is_contiguous() else logits.float().contiguous()

    def cls(self, logits, labels, loss, weight=1.0, metered=True):
        from . import ops
        ops.train_meter_cls(self._logits(logits), labels.contiguous(), self._loss(loss), self.rec, weight, metered)

    def partseg(self, logits, labels, loss, part_start, part_count, weight=1.0, metered=True):
        from . import ops
        ops.train_meter_partseg(self._logits(logits), labels.contiguous(), self._loss(loss), part_start, part_count, self.rec,
                                self.scratch, weight, metered)

    def read(self, extra=None):
        """THE read of the epoch's train side -> {key: float}; raises FloatingPointError where the reference's per-step finite
        check (main_cls.py:205-207) would have stopped the run inside the epoch, or a label left its range.  extra: a device
        tensor that travels in the same copy (widened to double: what .item() gives for fp32), returned as a list under 'extra'."""
        from . import ops
        vec = self.rec if extra is None else torch.cat([self.rec, extra.detach().double().reshape(-1).to(self.rec.device)])
        host = vec.cpu().tolist()
        out = dict(zip(ops.METER_KEYS, host))
        out["extra"] = host[ops.METER_REC:]
        if out["nonfinite"]:
            raise FloatingPointError(f"Loss was not finite in {int(out['nonfinite'])} of {int(out['calls'])} steps, stopping training")
        if out["bad_labels"]:
            raise FloatingPointError(f"{int(out['bad_labels'])} of {int(out['calls'])} steps saw a label outside its range (the "
                                     "criterion's loss is NaN there), stopping training")
        return out


def order_draws(device):
    """Call after a step has been queued: the next step's ahead stage (graphs.AheadStage on the grouping stream: FPS starts, in part
    segmentation the whole frozen backbone with its DropPath draws) starts behind THIS step's forward on the caller's stream.
    Why: both are hipGraph replays that draw from torch's default generator, and every captured graph reads the generator's seed
    and offset from ONE pair of device words that each replay refills on its own stream just before it launches.  With the host
    running a step ahead -- which is the point of keeping the meters on the device -- the next stage's refill can land while this
    step's decoder (its dropout sits at the end of the graph) has not drawn yet, and the step then draws from the wrong offset:
    valid random numbers, but not the ones the same seed gives a loop that reads its loss back in every step.  One stream
    dependency, no host wait; the ahead stage keeps its overlap with this step's backward and optimizer (the text stream)."""
    from . import graphs
    graphs.shared_group_stream(device).wait_stream(torch.cuda.current_stream(device))


def gather_sums(sum, count, world_size):
    """every rank's [sum, count] in rank order (one collective), or None on a single process: meter_average's world_sums"""
    import torch.distributed as dist
    if world_size <= 1 or not (dist.is_available() and dist.is_initialized()):
        return None
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    mine = torch.tensor([float(sum), float(count)], dtype=torch.float64, device=dev)
    out = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(out, mine)
    return [t.cpu().tolist() for t in out]
