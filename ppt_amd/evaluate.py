"""validate() on the device: the loops of main_cls.py:237-299 and main_partseg.py:260-367 without their host round trips.

The reference turns logits and labels into figures with `.item()` calls per batch, per sample and per part (main_cls.py:273-284,
main_partseg.py:300-344: several hundred device reads per batch of 16).  Here a batch costs ONE launch of csrc/metrics.hip that
writes a small integer record per sample into a device buffer; nothing is read back and nothing synchronises until `result()`,
which makes one copy and repeats the reference's final arithmetic on the host, from the integers, in the reference's order --
`acc`, `mean_inst_iou`, `mean_class_iou`, the category IoUs and the per-class accuracies are bit-equal to what the reference
returns for the same logits; `loss` is the same sum of row losses accumulated in double instead of fp32.

    import models.ULIP_models as models
    validate = models.validate                 # main_cls.py;  main_partseg.py: validate = models.validate_partseg

Under a process group each rank validates its shard and `result()` makes one collective; the figures are those of the UNION of
the shards.  The reference instead all-reduces its meters and truncates the summed value to an integer (`self.sum = int(t[0])`,
utils/utils.py:346), which reports an accuracy of (whole samples) / count -- a bug, not reproduced here.
"""
import collections

import numpy as np
import torch
from torch import nn

from . import ops


def _check_criterion(criterion):
    """-> label_smoothing.  Only nn.CrossEntropyLoss as main_cls.py:52 / main_partseg.py builds it is covered."""
    if not isinstance(criterion, nn.CrossEntropyLoss):
        raise NotImplementedError(f"validate: criterion must be an nn.CrossEntropyLoss, got {type(criterion).__name__}")
    if criterion.weight is not None:
        raise NotImplementedError("validate: a class-weighted CrossEntropyLoss is not covered by the metric kernels")
    if criterion.reduction != "mean":
        raise NotImplementedError(f"validate: reduction={criterion.reduction!r} (only 'mean')")
    if criterion.ignore_index != -100:
        raise NotImplementedError("validate: a changed ignore_index is not covered by the metric kernels")
    return float(criterion.label_smoothing)


def _gather(vec, process_group):
    """ONE collective: every rank's vector, in rank order -> [world, len] (summed by the caller in that fixed order)"""
    import torch.distributed as dist
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(process_group) == "nccl" else torch.device("cpu")
    mine = vec.to(dev)
    out = [torch.empty_like(mine) for _ in range(dist.get_world_size(process_group))]
    dist.all_gather(out, mine, group=process_group)
    return torch.stack(out).cpu()


def _default_group():
    import torch.distributed as dist
    return dist.group.WORLD if dist.is_available() and dist.is_initialized() else None       # utils.is_dist_avail_and_initialized


def _raise_on_bad_labels(flags, what):
    bad = int(((flags & ops.METRIC_BAD_LABEL) != 0).sum())
    if bad:
        raise ValueError(f"validate: {bad} {what} with a label outside the class range (nn.CrossEntropyLoss raises a device "
                         "assert there): the data is corrupt")


class _Records:
    """Device buffer of int32 records, `width` per sample, that grows by doubling.  Every size comes from tensor shapes, which
    the host knows: appending reads nothing back."""

    def __init__(self, width):
        self.width, self.buf, self.n, self.batches = width, None, 0, []

    def reserve(self, rows, device):
        need = self.n + rows
        if self.buf is None or self.buf.shape[0] < need or self.buf.device != device:
            cap = max(256, 2 * (0 if self.buf is None else self.buf.shape[0]))
            while cap < need:
                cap *= 2
            new = torch.empty((cap, self.width), dtype=torch.int32, device=device)
            if self.n:
                new[:self.n].copy_(self.buf[:self.n])
            self.buf = new
        return self.buf[self.n:need]

    def commit(self, rows, batch):
        self.n += rows
        self.batches.append(batch)

    def host(self):
        if self.n == 0:
            return np.zeros((0, self.width), np.int32)
        return self.buf[:self.n].cpu().numpy()                 # THE device -> host copy of the epoch


def _as_inputs(logits, labels):
    logits = logits.detach()
    if logits.dtype != torch.float32 or not logits.is_contiguous() or logits.data_ptr() % 16:
        logits = logits.float().clone(memory_format=torch.contiguous_format)
    labels = labels.detach()
    if labels.dtype != torch.int64 or not labels.is_contiguous():
        labels = labels.long().contiguous()
    return logits, labels


def accuracy(output, target, topk=(1,)):
    """utils/utils.py:376-398 on the rank the metric kernel writes: (res, correct) with res[i] = [1] fp32, the share of samples
    whose target is among the topk[i] largest logits, and correct [maxk, B] bool.  Device tensors; no host read.  Equal logits
    rank by index (the lower index first), where torch.topk leaves the order open."""
    maxk = max(topk)
    B = target.size(0)
    logits, labels = _as_inputs(output, target)
    rec = torch.empty((B, ops.CLS_REC), dtype=torch.int32, device=logits.device)
    ops.cls_metrics(logits, labels, 0.0, rec)
    correct = rec[:, 1].unsqueeze(0) == torch.arange(maxk, device=rec.device, dtype=torch.int32).unsqueeze(1)
    res = []
    for k in topk:
        correct_k = correct[:k].reshape(-1).float().sum(0, keepdim=True)
        res.append(correct_k.mul_(1.0 / B))
    return res, correct


# ---- recognition --------------------------------------------------------------------------------------------------------------
def finalize_cls(records, batch_sizes, classnames=None, process_group=None, num_classes=None):
    """The host half of ClsMetrics.result(): records [n, 4] int32 as ppt_cls_metrics writes them (loss bits, rank, flags, label)
    and the batch sizes in order -> the dict of validate().  Without a process group this is main_cls.py:270-299 statement by
    statement: per batch `correct.float().sum() * (1 / B)` in fp32 and the batch's mean loss, meters that hold
    `sum += val * B` as Python floats, per-class counts keyed by name in order of first appearance."""
    rec = np.ascontiguousarray(np.asarray(records, dtype=np.int32).reshape(-1, ops.CLS_REC))
    loss = rec[:, 0].copy().view(np.float32).astype(np.float64)
    rank, flags, label = rec[:, 1], rec[:, 2], rec[:, 3]
    _raise_on_bad_labels(flags, "samples")
    assert sum(batch_sizes) == rec.shape[0], "batch sizes do not add up to the number of records"
    nonfinite = int(((flags & ops.METRIC_NONFINITE) != 0).sum())
    name = (lambda c: classnames[c]) if classnames is not None else str

    if process_group is not None:
        C = num_classes if num_classes is not None else len(classnames) if classnames is not None else None
        if C is None:
            raise ValueError("finalize_cls under a process group needs num_classes: the per-class table has one length on every rank")
        head = torch.tensor([rec.shape[0], int((rank == 0).sum()), int((rank < 5).sum()), nonfinite], dtype=torch.int64)
        loss_bits = torch.tensor([float(loss.sum())], dtype=torch.float64).view(torch.int64)          # (the double travels as its bits)
        per = np.zeros((2, C), np.int64)
        np.add.at(per[0], label, 1)
        np.add.at(per[1], label[rank == 0], 1)
        vec = torch.cat([head, loss_bits, torch.from_numpy(per.reshape(-1))])
        allv = _gather(vec, process_group)
        tot = allv[:, :4].sum(0)
        n, c1, c5, nonfinite = (int(v) for v in tot)
        loss_sum = 0.0
        for r in range(allv.shape[0]):                          # rank order: the same bits on every rank
            loss_sum += float(allv[r, 4:5].contiguous().view(torch.float64))
        per = allv[:, 5:].sum(0).numpy().reshape(2, C)
        per_class = collections.OrderedDict((name(c), int(per[1, c]) / int(per[0, c])) for c in range(C) if per[0, c])
        return {'acc': c1 / n if n else 0, 'loss': loss_sum / n if n else 0, 'acc5': c5 / n if n else 0,
                'per_class_acc': per_class, 'n': n, 'nonfinite_rows': nonfinite}

    top1_sum = top5_sum = loss_sum = 0.0
    count = 0
    stats, hits = collections.defaultdict(int), collections.defaultdict(int)
    o = 0
    for B in batch_sizes:
        r, lb = rank[o:o + B], label[o:o + B]
        # utils.accuracy: correct[:k].reshape(-1).float().sum(0, keepdim=True).mul_(1.0 / batch_size), then .item()
        acc1 = torch.tensor([float((r == 0).sum())], dtype=torch.float32).mul_(1.0 / B).item()
        acc5 = torch.tensor([float((r < 5).sum())], dtype=torch.float32).mul_(1.0 / B).item()
        top1_sum += acc1 * B                                    # AverageMeter.update(val, n): sum += val * n
        top5_sum += acc5 * B
        loss_sum += float(loss[o:o + B].sum() / B) * B
        count += B
        for c, hit in zip(lb.tolist(), (r == 0).tolist()):
            stats[name(c)] += 1
            if hit:
                hits[name(c)] += 1
        o += B
    per_class = collections.OrderedDict((k, hits[k] / stats[k]) for k in stats)
    return {'acc': top1_sum / count if count else 0, 'loss': loss_sum / count if count else 0,
            'acc5': top5_sum / count if count else 0, 'per_class_acc': per_class, 'n': count, 'nonfinite_rows': nonfinite}


class ClsMetrics:
    """Recognition metrics of one validation pass.  update(logits [B, C], labels [B]) queues one kernel on the current stream
    and returns; result() -> {'acc', 'loss', 'acc5', 'per_class_acc', 'n', 'nonfinite_rows'} ('acc' is a share in [0, 1], as
    utils.accuracy returns it).  A label outside [0, C) makes result() raise ValueError (the stance of health.BIT_LABEL).
    `nonfinite_rows` counts rows with a non-finite logit; what such a row is ranked as is unspecified.
    process_group: see the module docstring -- one collective, the figures of the union of the shards, and NOT the reference's
    `int(sum)` truncation (utils/utils.py:346)."""

    def __init__(self, num_classes, label_smoothing, classnames=None, process_group=None):
        self.num_classes, self.label_smoothing = int(num_classes), float(label_smoothing)
        self.classnames = None if classnames is None else list(classnames)
        self.process_group = process_group
        self.records = _Records(ops.CLS_REC)

    def reset(self):
        self.records = _Records(ops.CLS_REC)

    def update(self, logits, labels):
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"ClsMetrics: logits {tuple(logits.shape)} for {self.num_classes} classes")
        logits, labels = _as_inputs(logits, labels.reshape(-1))
        B = logits.shape[0]
        ops.cls_metrics(logits, labels, self.label_smoothing, self.records.reserve(B, logits.device))
        self.records.commit(B, B)

    def result(self):
        return finalize_cls(self.records.host(), self.records.batches, self.classnames, self.process_group, self.num_classes)


# ---- part segmentation --------------------------------------------------------------------------------------------------------
def part_tables(category2part):
    """category2part {name: [part ids]} -> (part_start [P], part_count [P]) int32 numpy tables: for each part id its category's
    first part and number of parts.  The kernel masks the arg-max to the RANGE [start, start + count): a category whose parts are
    not a contiguous ascending range raises ValueError."""
    P = sum(len(v) for v in category2part.values())
    start, count = np.full(P, -1, np.int32), np.zeros(P, np.int32)
    for cat, parts in category2part.items():
        parts = [int(p) for p in parts]
        if not parts or parts != list(range(parts[0], parts[0] + len(parts))):
            raise ValueError(f"PartsegMetrics: the parts of category {cat!r} are not a contiguous ascending range: {parts}")
        for p in parts:
            if not 0 <= p < P or start[p] >= 0:
                raise ValueError(f"PartsegMetrics: part {p} of category {cat!r} is outside [0, {P}) or belongs to two categories")
            start[p], count[p] = parts[0], len(parts)
    return start, count


def finalize_partseg(records, batches, category2part, process_group=None):
    """The host half of PartsegMetrics.result(): records [n, 32] int32 as ppt_partseg_metrics writes them and the (B, N) of every
    batch in order -> the dict of validate_partseg().  Without a process group this is main_partseg.py:307-358 statement by
    statement on the integer counts: batch accuracy `correct / (B * N)` in fp32, a part's IoU 1 when ground truth and prediction
    are both absent and else the int / int division in fp32, a cloud's figure the fp32 mean over its category's parts, category and
    overall figures torch.mean over fp32 tensors.  A category without a cloud gives NaN, and so does mean_class_iou then (the
    reference's mean of an empty tensor); 'category_counts' lets a caller do otherwise.
    A ragged batch (PartsegMetrics.update(..., lengths=)) is listed as (B, Nmax, R), R the number of points that exist: R stands
    where B * N stands for a uniform batch, in the batch accuracy and in the batch's mean loss."""
    rec = np.ascontiguousarray(np.asarray(records, dtype=np.int32).reshape(-1, ops.PARTSEG_REC))
    _raise_on_bad_labels(rec[:, 3], "clouds")
    batches = [(b[0], b[1], b[2] if len(b) > 2 else b[0] * b[1]) for b in batches]            # (B, N, points)
    assert sum(b[0] for b in batches) == rec.shape[0], "batch sizes do not add up to the number of records"
    nonfinite = int(((rec[:, 3] & ops.METRIC_NONFINITE) != 0).sum())
    loss = rec[:, 4].copy().view(np.float32).astype(np.float64)
    by_start = {int(parts[0]): cat for cat, parts in category2part.items()}
    shape_ious = {cat: [] for cat in category2part}
    acc_sum = loss_sum = 0.0
    count = 0
    correct_pts = total_pts = 0
    o = 0
    for B, N, points in batches:
        correct = int(rec[o:o + B, 2].sum())
        acc = (torch.tensor(correct) / points).item()            # main_partseg.py:307-308: int64 tensor / int -> fp32
        acc_sum += acc * B
        loss_sum += float(loss[o:o + B].sum() / points) * B
        count += B
        correct_pts += correct
        total_pts += points
        for i in range(o, o + B):
            cat = by_start[int(rec[i, 0])]
            part_ious = [.0 for _ in range(len(category2part[cat]))]
            for j in range(len(part_ious)):
                gt, pred, both = (int(v) for v in rec[i, 8 + 3 * j:11 + 3 * j])
                union = gt + pred - both
                part_ious[j] = 1 if union == 0 else torch.tensor(both) / torch.tensor(union)       # :338-343
            shape_ious[cat].append(torch.mean(torch.tensor(part_ious)))                            # :344
        o += B
    counts = collections.OrderedDict((cat, len(v)) for cat, v in shape_ious.items())

    if process_group is not None:
        cats = list(category2part)
        vec = torch.tensor([count, correct_pts, total_pts, nonfinite, float(loss.sum())]
                           + [float(torch.stack(shape_ious[c]).double().sum()) if shape_ious[c] else 0.0 for c in cats]
                           + [float(counts[c]) for c in cats], dtype=torch.float64)
        allv = _gather(vec, process_group)
        tot = torch.zeros_like(allv[0])
        for r in range(allv.shape[0]):                          # rank order: the same bits on every rank
            tot += allv[r]
        tot = tot.tolist()
        n, correct_pts, total_pts, nonfinite = (int(v) for v in tot[:4])
        sums, cnts = tot[5:5 + len(cats)], [int(v) for v in tot[5 + len(cats):]]
        cat_iou = collections.OrderedDict((c, s / k if k else float('nan')) for c, s, k in zip(cats, sums, cnts))
        return {'acc': correct_pts / total_pts if total_pts else 0, 'loss': tot[4] / total_pts if total_pts else 0,
                'mean_inst_iou': sum(sums) / sum(cnts) if sum(cnts) else float('nan'),
                'mean_class_iou': float(np.mean(list(cat_iou.values()))) if cats else float('nan'),
                'category_ious': cat_iou, 'category_counts': collections.OrderedDict(zip(cats, cnts)), 'n': n,
                'nonfinite_rows': nonfinite}

    all_inst_ious = []
    category_ious = collections.OrderedDict()
    for cat in shape_ious:                                      # :349-358
        all_inst_ious += shape_ious[cat]
        category_ious[cat] = torch.mean(torch.tensor(shape_ious[cat]))
    mean_inst_iou = torch.mean(torch.tensor(all_inst_ious))
    mean_class_iou = torch.mean(torch.tensor(list(category_ious.values())))
    return {'acc': acc_sum / count if count else 0, 'loss': loss_sum / count if count else 0,
            'mean_inst_iou': mean_inst_iou.item(), 'mean_class_iou': mean_class_iou.item(),
            'category_ious': collections.OrderedDict((c, v.item()) for c, v in category_ious.items()),
            'category_counts': counts, 'n': count, 'nonfinite_rows': nonfinite}


class PartsegMetrics:
    """Part-segmentation metrics of one validation pass.  update(logits [B, N, P], labels [B, N]) queues one kernel on the
    current stream and returns; update(..., lengths=) takes a padded ragged batch: cloud b is its first lengths[b] rows, nothing
    behind them is read or counted (labels and logits there may be anything), accuracy and loss are over the points that exist; result() -> {'acc', 'loss', 'mean_inst_iou', 'mean_class_iou', 'category_ious',
    'category_counts', 'n', 'nonfinite_rows'}.  A cloud's category is the one its point 0's label belongs to
    (main_partseg.py:302, :326).  `nonfinite_rows` counts CLOUDS with a non-finite logit; their predictions are unspecified.
    A label outside [0, P) makes result() raise ValueError.  process_group: one collective of the per-category float64 IoU sums
    and counts; the figures are those of the union of the shards (and not utils/utils.py:346's truncated meters)."""

    def __init__(self, category2part, label_smoothing, process_group=None):
        self.category2part = collections.OrderedDict((k, [int(p) for p in v]) for k, v in category2part.items())
        self.label_smoothing = float(label_smoothing)
        self.process_group = process_group
        self.start, self.count = part_tables(self.category2part)
        self.num_parts, self.max_parts = len(self.start), int(self.count.max())
        self.records = _Records(ops.PARTSEG_REC)
        self._tables = self._partial = None

    def reset(self):
        self.records = _Records(ops.PARTSEG_REC)

    def update(self, logits, labels, lengths=None, total_rows=None):
        """lengths: a host sequence (validated: B entries, 1 <= length <= N) or a device int32 tensor [B]; for the latter pass
        total_rows = sum(lengths) where the host knows it -- otherwise the sum is read from the device here, ONE host read."""
        if logits.dim() != 3 or logits.shape[2] != self.num_parts:
            raise ValueError(f"PartsegMetrics: logits {tuple(logits.shape)} for {self.num_parts} parts")
        logits, labels = _as_inputs(logits, labels)
        B, N, _ = logits.shape
        dev = logits.device
        batch = (B, N)
        if lengths is not None:
            from . import engine
            lengths, R = engine.cloud_lengths(lengths, B, N, dev, total_rows=total_rows)
            batch = (B, N, R)
        if self._tables is None or self._tables[0].device != dev:
            # (host -> device, queued without waiting: the numpy arrays live as long as this object)
            self._tables = tuple(torch.from_numpy(t).to(dev, non_blocking=True) for t in (self.start, self.count))
        need = B * ops.partseg_metrics_chunks(N)
        if self._partial is None or self._partial.numel() < need or self._partial.device != dev:
            self._partial = torch.empty((need,), dtype=torch.float32, device=dev)
        ops.partseg_metrics(logits, labels, self.label_smoothing, self._tables[0], self._tables[1], self.max_parts,
                            self.records.reserve(B, dev), self._partial, lengths=lengths)
        self.records.commit(B, batch)

    def result(self):
        return finalize_partseg(self.records.host(), self.records.batches, self.category2part, self.process_group)


# ---- the drop-ins -------------------------------------------------------------------------------------------------------------
def _to_device(t, gpu):
    # a tensor that is on the device already (DevicePrefetcher, DeviceBatchLoader) is passed on as the SAME object: it carries the
    # event that marks it complete, and the model's input-only stages order themselves behind that event (graphs.ready_event)
    if t.is_cuda:
        return t
    return t.cuda(gpu, non_blocking=True)


def to_categorical(label, num_classes):
    """utils/utils.py:401-412 with the one-hot built on the device: label [...] int -> [..., num_classes] fp32"""
    return torch.eye(num_classes, device=label.device)[label.long()]


def validate(test_loader, model, criterion, args):
    """Drop-in for main_cls.validate (main_cls.py:237-299): the same batch tuples (pc, target, ...), model.eval(), no grad; returns
    {'acc', 'loss'} with the reference's meanings plus 'per_class_acc' (name -> accuracy: what the reference only prints), 'acc5',
    'n', 'nonfinite_rows'.  test_loader: a DataLoader, a DevicePrefetcher or a DeviceBatchLoader.  One kernel per batch, no
    device read before the end.  Only criterion.label_smoothing is read; a weight, another reduction or ignore_index raise
    NotImplementedError.  Class names: args.classnames (label -> name), else the label's number."""
    smoothing = _check_criterion(criterion)
    classnames = getattr(args, 'classnames', None)
    metrics = None
    model.eval()
    with torch.no_grad():
        for inputs in test_loader:
            pc = _to_device(inputs[0], args.gpu)
            target = _to_device(inputs[1], args.gpu)
            pred = model(pc)
            if metrics is None:
                metrics = ClsMetrics(pred.shape[-1], smoothing, classnames, _default_group())
            metrics.update(pred, target)
    if metrics is None:
        raise ValueError("validate: the loader yielded no batch")
    out = metrics.result()
    print(','.join(out['per_class_acc'].keys()))                # main_cls.py:294-295
    print(','.join([str(value) for value in out['per_class_acc'].values()]))
    return out


def validate_partseg(test_loader, model, criterion, args):
    """Drop-in for main_partseg.validate (main_partseg.py:260-367): batch tuples (pc, cls_label, part_label, ...), the one-hot
    class label built on the device, model.eval(), no grad; `test_loader.dataset.category2part` gives the part ranges (a
    DeviceBatchLoader: pass `args.category2part`).  Returns {'acc', 'loss', 'mean_inst_iou', 'mean_class_iou'} with the reference's
    meanings plus 'category_ious', 'category_counts', 'n', 'nonfinite_rows'.
    A loader that marks itself ragged (`test_loader.ragged`: DeviceBatchLoader(recipe="shapenetpart", ragged=True), whole shapes)
    yields a fourth element, lengths [B] i32: it goes to model.forward_ragged and to the metrics, and every figure is over the
    points that exist (part labels behind a cloud's end are never read).  The labels' padding is -100, the criterion's
    default ignore_index (the only one _check_criterion accepts)."""
    ragged = bool(getattr(test_loader, 'ragged', False))
    smoothing = _check_criterion(criterion)
    category2part = getattr(args, 'category2part', None)
    if category2part is None:
        category2part = test_loader.dataset.category2part
    metrics = PartsegMetrics(category2part, smoothing, _default_group())
    num_shape_classes = len(category2part)
    model.eval()
    with torch.no_grad():
        for inputs in test_loader:
            pc = _to_device(inputs[0], args.gpu)
            cls_label = _to_device(inputs[1], args.gpu)
            part_label = _to_device(inputs[2], args.gpu)
            if ragged:
                lengths = _to_device(inputs[3], args.gpu)
                total = getattr(inputs[3], '_ppt_total', None)          # the loader's host count: no device read per batch
                part_pred = model.forward_ragged(pc, to_categorical(cls_label, num_shape_classes), lengths, total_rows=total)
                metrics.update(part_pred, part_label, lengths=lengths, total_rows=total)
                continue
            part_pred = model(pc, to_categorical(cls_label, num_shape_classes))
            metrics.update(part_pred, part_label)
    out = metrics.result()
    for cat, iou in out['category_ious'].items():
        print('Category:', cat, ' ||  Category IoU:', iou)
    return out
