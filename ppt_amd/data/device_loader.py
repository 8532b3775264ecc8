"""A dataset that lives on the device and a loader that produces its batches there ("device-resident dataset").

What the reference's datasets do per sample, every epoch, in DataLoader workers (data/dataset_3d.py):

    ModelNet / ModelNet_fs (:291-326)   farthest point sampling N -> npoints from a fresh random start, pc_normalize, and for the
                                        train split translate_pointcloud + np.random.shuffle
    ScanObjectNN (:406-419)             the first num_points rows (no normalisation), and for the train split translate + shuffle
    ShapeNetPart (:734-757)             pc_normalize, then np.random.choice(len, npoints, replace=True) rows of the cloud and of its
                                        per-point part labels
    ShapeNet (:576-607)                 farthest point sampling N -> npoints (or, for a cloud of npoints rows, a shuffle of its rows),
                                        pc_norm, then random_point_dropout, random_scale_point_cloud, shift_point_cloud,
                                        rotate_perturbation_point_cloud, rotate_point_cloud (recipe "shapenet55"; what
                                        data/ShapeNet-55.yaml configures)

ModelNet40 at 8192 points is under 1 GB; the raw clouds simply stay in device memory (`DeviceCloudSet`).  `DeviceBatchLoader` then
produces a batch with one batched launch of the path's FPS kernel (csrc/fps.hip), one launch of csrc/cloud_prep.hip for
everything after it and, where augmentations are asked for, one launch of csrc/cloud_augment.hip -- no workers, no pickling, no host copy of a cloud -- `ahead` batches in front of the consumer on the grouping
stream (graphs.shared_group_stream), each yielded tensor carrying its completion event like a DevicePrefetcher batch.

The random draws come from one of two places:

    draws="numpy"   the host draws from `np.random.RandomState([seed, epoch, rank])`, sample after sample in batch order, each sample
                    in the reference's order (`numpy_draws`): randint(0, N) when the stored cloud has more rows than npoints, then
                    for the train split uniform(2/3, 3/2, 3), uniform(-0.2, 0.2, 3), permutation(npoints); for part-seg
                    choice(len, npoints, replace=True).  Given the same generator state a batch is bit-identical to what the
                    reference's Dataset.__getitem__ returns (tests/test_datapipe_gpu.py against tests/golden/g_datapipe.npz).
    draws="device"  csrc/cloud_prep.hip: ppt_cloud_draws, Philox4x32-10 keyed by `seed` with the counter (dataset index, epoch, draw,
                    block): a sample's draws do not depend on the batch size, the number of ranks or the batch it lands in, and
                    the launching thread does no per-sample work.

Augmentations (ppt_amd/data/augment.py; csrc/cloud_augment.hip).  `augment=` takes a tuple of stage names out of ("dropout", "scale",
"shift", "rotate_perturbation", "rotate", "jitter") and is valid with every recipe: the stages are applied to the recipe's finished
cloud (after its own translate and shuffle, before the height column) as if the reference functions were called on pc[None] in that
order, and their draws follow the recipe's own draws in that order -- in numpy mode from the same generator (dropout: random(),
random(npoints); scale: uniform(0.8, 1.25, 1); shift: uniform(-0.1, 0.1, (1, 3)); rotate_perturbation: randn(3); rotate: uniform();
jitter: randn(1, npoints, 3)), in device mode from ppt_cloud_draws_aug (slots 4-10 of the same counter).  Recipe "shapenet55" with
train=True chains the first five itself (ShapeNet.__getitem__ always augments; here the test split takes the normalised sample as
it is) and yields (pc, target).  Its row selection: FPS from a fresh randint(0, rows) start when the cloud has more rows than
npoints; otherwise the reference's random_sample, which shuffles ONE persistent arange(npoints) cumulatively -- in numpy mode the
loader owns that array for its lifetime, as the reference's dataset object does; in device mode every (index, epoch) gets a fresh
Philox permutation instead (a uniformly random order either way; the cumulative state is what a worker process would not share).
Clouds of differing length under FPS (`ragged=True`, recipes "modelnet" and "shapenet55"): the batch still takes one draw launch,
one FPS launch and one cloud_prep launch -- ppt_fps_ragged_f32 walks every cloud's own row count, and each cloud's rows are the ones a
set of that length alone would give.  A "modelnet" cloud of exactly npoints rows keeps the reference's treatment (no FPS, the rows
as stored, no randint drawn for it); "shapenet55" refuses a ragged set that holds one (it would need random_sample's persistent
permutation for some rows of the batch and FPS for the others).
Not covered: the rendered images, the captions and their random.choice, normals.
"""
import collections
import math

import numpy as np
import torch

from .augment import KERNEL_STAGE, SHAPENET_CHAIN, check_stages, host_stage_draws, kernel_stage

RECIPES = ("modelnet", "scanobjectnn", "shapenetpart", "shapenet55")
FPS_RECIPES = ("modelnet", "shapenet55")
KERNEL_PARAMS = {key for _, key in KERNEL_STAGE.values()}      # mask, scale, shift, perturb, rotate, noise: the draws a stage reads
MAX_ROWS = 16384          # csrc/fps.hip: N <= 16384
MAX_NPOINTS = 8192        # csrc/cloud_prep.hip: one cloud of the batch in LDS


def epoch_indices(n_items, epoch=0, shuffle=True, seed=0, drop_last=False, rank=0, world_size=1):
    """The dataset indices rank `rank` visits in epoch `epoch`, in order: torch.utils.data.DistributedSampler's rule (permutation
    from a torch.Generator seeded with seed + epoch, padding by wrap-around or truncation to a multiple of world_size,
    then rank::world_size); world_size = 1 is the plain shuffled / sequential order."""
    if not 0 <= rank < world_size:
        raise ValueError(f"rank {rank} outside [0, {world_size})")
    if drop_last and n_items % world_size != 0:
        num = math.ceil((n_items - world_size) / world_size)
    else:
        num = math.ceil(n_items / world_size)
    total = num * world_size
    if shuffle:
        g = torch.Generator()
        g.manual_seed(int(seed) + int(epoch))
        idx = torch.randperm(n_items, generator=g).tolist()
    else:
        idx = list(range(n_items))
    if not drop_last:
        pad = total - len(idx)
        idx += idx[:pad] if pad <= len(idx) else (idx * math.ceil(pad / len(idx)))[:pad]
    else:
        idx = idx[:total]
    return np.asarray(idx[rank:total:world_size], dtype=np.int64)


def numpy_draws(rs, recipe, train, rows, npoints, augment=(), permutation=None):
    """One sample's draws from the np.random.RandomState `rs`, in the order the reference's __getitem__ makes them.  -> dict with
    the ones this recipe / split needs of start (int), scale [3] f64, shift [3] f64, perm [npoints], sel [npoints].
    "shapenet55" (ShapeNet.__getitem__, :581-595): randint(0, rows) when npoints < rows, otherwise a shuffle of `permutation` (the
    dataset's persistent arange(npoints), :545 / :572, changed in place; None: a fresh one) whose head is `sel`; then for the train
    split random(), random(npoints), uniform(0.8, 1.25, 1), uniform(-0.1, 0.1, (1, 3)), randn(3), uniform().
    augment: stage names (ppt_amd.data.augment.STAGES) whose draws follow, as the reference function of each makes them for pc[None].
    Augmentation draws are keyed aug_ratio, aug_u [npoints], aug_mask [npoints] u8, aug_scale (a number), aug_shift [3], aug_angles [3],
    aug_perturb [3, 3], aug_angle (a number), aug_rotate [3, 3], aug_noise [npoints, 3]."""
    d = {}
    stages = tuple(augment)
    if recipe == "shapenetpart":
        d["sel"] = rs.choice(rows, npoints, replace=True)                     # dataset_3d.py:752
    elif recipe == "shapenet55":
        if npoints < rows:
            d["start"] = rs.randint(0, rows)                                  # :50, inside farthest_point_sample
        else:
            if permutation is None:
                permutation = np.arange(npoints)
            rs.shuffle(permutation)                                           # :572
            d["sel"] = permutation[:npoints].copy()
        if train:
            stages = SHAPENET_CHAIN + stages
    else:
        if recipe == "modelnet" and npoints < rows:
            d["start"] = rs.randint(0, rows)                                  # :50, inside farthest_point_sample
        if train:
            d["scale"] = rs.uniform(low=2. / 3., high=3. / 2., size=[3])      # :156
            d["shift"] = rs.uniform(low=-0.2, high=0.2, size=[3])             # :157
            d["perm"] = rs.permutation(npoints)                               # np.random.shuffle(cloud): the same swaps, applied to arange
    for stage in stages:
        for k, v in host_stage_draws(rs, stage, 1, npoints).items():
            d["aug_" + k] = v[0]
    return d


def add_height(pc):
    """data/dataset_3d.py:311-314 (`use_height`, what PointNeXt reads) on a batch: pc [B,n,3] f32 -> [B,n,4], column 3 = y minus the
    cloud's smallest y, both in fp32.  A device batch takes one launch (ops.cloud_height); a host tensor the same two torch operations."""
    if pc.is_cuda:
        from .. import ops
        return ops.cloud_height(pc.contiguous())
    y = pc[:, :, 1:2]
    return torch.cat([pc, y - y.min(dim=1, keepdim=True)[0]], dim=2)


def _rows_of(a):
    return [np.asarray(x) for x in a] if isinstance(a, (list, tuple)) else None


class DeviceCloudSet:
    """The raw clouds of a dataset, uploaded once.

    points   [M, Nmax, C >= 3] float32 array / tensor, or a list of M arrays [N_i, C] (padded to the longest; `lengths` is then
             derived).  xyz = the first three columns; further columns (normals) stay resident but no recipe reads them.
    labels   [M] integer class labels.
    seg      [M, Nmax] int32 per-point part labels (or a list of [N_i]) -- a part-segmentation set.  Its clouds are normalised ONCE
             here, on the host, with ppt_amd.data.pc_normalize.  The reference (dataset_3d.py:750) re-normalises its cached array
             on every access, so from the second epoch on it normalises an already normalised cloud and the values drift by
             rounding; that is not reproduced -- every epoch sees the first access's values.
    lengths  [M] valid rows per cloud (None: all Nmax).
    Nmax <= 16384 (the FPS kernel's limit).  float32 only."""

    def __init__(self, points, labels, seg=None, lengths=None, device=None):
        from .dataset_3d import pc_normalize
        ragged = _rows_of(points)
        if ragged is not None:
            for x in ragged:
                self._check_dtype(x.dtype)
            if lengths is not None:
                raise ValueError("lengths is derived from a list of clouds; do not give both")
            lengths = np.asarray([x.shape[0] for x in ragged], dtype=np.int32)
            C = ragged[0].shape[1]
            pts = np.zeros((len(ragged), int(lengths.max()), C), dtype=np.float32)
            for i, x in enumerate(ragged):
                pts[i, :x.shape[0]] = x
            if seg is not None:
                sg = np.zeros(pts.shape[:2], dtype=np.int32)
                for i, s in enumerate(_rows_of(seg)):
                    sg[i, :len(s)] = s
                seg = sg
        else:
            pts = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
            self._check_dtype(pts.dtype)
        if pts.ndim != 3 or pts.shape[2] < 3:
            raise ValueError(f"points must be [M, Nmax, C >= 3], got {pts.shape}")
        M, Nmax, _ = pts.shape
        if Nmax > MAX_ROWS:
            raise ValueError(f"DeviceCloudSet: clouds of at most {MAX_ROWS} rows (got {Nmax}): the FPS kernel's limit")
        labels = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels).reshape(-1).astype(np.int64)
        if labels.shape[0] != M:
            raise ValueError(f"{labels.shape[0]} labels for {M} clouds")
        if lengths is not None:
            lengths = np.asarray(lengths).astype(np.int32).reshape(-1)
            if lengths.shape[0] != M or lengths.min() < 1 or lengths.max() > Nmax:
                raise ValueError("lengths must be [M] with 1 <= length <= Nmax")
        if seg is not None:
            seg = np.ascontiguousarray(np.asarray(seg.cpu() if torch.is_tensor(seg) else seg).astype(np.int32))
            if seg.shape != (M, Nmax):
                raise ValueError(f"seg must be {(M, Nmax)}, got {seg.shape}")
            pts = np.array(pts, dtype=np.float32, copy=True)
            for i in range(M):
                L = Nmax if lengths is None else int(lengths[i])
                pts[i, :L, 0:3] = pc_normalize(pts[i, :L, 0:3])
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.lengths_host = lengths                                            # numpy copy: the host-side draws need the row counts
        self.points = torch.from_numpy(np.ascontiguousarray(pts)).to(self.device)
        self.labels = torch.from_numpy(labels).to(self.device)
        self.seg = None if seg is None else torch.from_numpy(seg).to(self.device)
        self.lengths = None if lengths is None else torch.from_numpy(lengths).to(self.device)

    @staticmethod
    def _check_dtype(dt):
        if dt != np.float32:
            raise TypeError(f"DeviceCloudSet: float32 clouds only (got {dt}): the reference's datasets hold float32 arrays and a float64 "
                            "array would be sampled and normalised in float64 arithmetic, which the fp32 kernels do not reproduce")

    def __len__(self):
        return self.points.shape[0]

    def subset(self, indices):
        """A new DeviceCloudSet over the clouds `indices` (host integers, e.g. data.fewshot.fewshot_indices; repeats allowed), in
        that order: index_select on the device, `seg` and `lengths` follow, no cloud travels through the host."""
        idx = np.asarray(indices.cpu() if torch.is_tensor(indices) else indices).reshape(-1).astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError(f"DeviceCloudSet.subset: indices outside [0, {len(self)})")
        item = torch.from_numpy(idx).to(self.device)
        new = object.__new__(DeviceCloudSet)
        new.device = self.device
        new.lengths_host = None if self.lengths_host is None else self.lengths_host[idx]
        new.points = self.points.index_select(0, item)
        new.labels = self.labels.index_select(0, item)
        new.seg = None if self.seg is None else self.seg.index_select(0, item)
        new.lengths = None if self.lengths is None else self.lengths.index_select(0, item)
        return new

    def rows(self, idx):
        """valid rows of the clouds `idx` (host array)"""
        if self.lengths_host is None:
            return np.full(len(idx), self.points.shape[1], dtype=np.int32)
        return self.lengths_host[idx]


class DeviceBatchLoader:
    """Iterate a DeviceCloudSet in batches made on the device.  Yields device tensors with the shapes and dtypes the reference's
    default collate gives: (pc [B, npoints, 3] f32, target [B] i64) for "modelnet" / "scanobjectnn", (pc, cls [B, 1] i32,
    seg [B, npoints] i64) for "shapenetpart" (seg already `.long()`, as main_partseg.py:207 makes it).  use_height=True (the
    reference's --use_height, what PointNeXt reads): pc is [B, npoints, 4], `add_height` applied to the finished cloud.
    Recipe "shapenet55" yields (pc, target) and, for train=True, carries ShapeNet's five augmentations; augment=(stage names) adds
    augmentations to any recipe (the module text says how); with either, the height column comes out of the augmentation launch.

    Order: `epoch_indices` -- DistributedSampler(shuffle, seed, drop_last) for (rank, world_size); drop_last also drops an
    incomplete last batch, as DataLoader(drop_last=True) does.  set_epoch(e) as with the sampler.
    Batch i + `ahead` is queued on graphs.shared_group_stream() before batch i is yielded.  Every yielded tensor is a fresh allocation
    made under that stream, record_stream-ed on the consumer's stream, and carries its completion event as `_ppt_ready`
    (graphs.wait_inputs: the model's input-only stages start behind it on their own stream).  The iteration never synchronises.
    No stream is created here: see DevicePrefetcher._stream for what a further stream does to the two-stream schedule.

    recipe "shapenetpart" with ragged=True is the WHOLE-SHAPE mode: no `sel` draw (np.random.choice(len, npoints, replace=True) labels
    a resample with duplicates, not the shape), every stored row of every cloud.  It yields (pc [B, Nmax_set, 3], cls [B, 1] i32,
    seg [B, Nmax_set] i64 with -100 behind each cloud's end, lengths [B] i32) -- what ULIP_PointBERT_partseg.forward_ragged(pc, onehot, lengths)
    and a criterion with ignore_index = -100 take; `npoints` is not used.  lengths carries the batch's total row count as the host
    integer `lengths._ppt_total` (validate_partseg passes it on, so no batch costs a device read).  One launch per batch
    (cloud_prep; the part-seg recipe has no scale / shift draws); `.ragged` is True.  Rows of pc behind a cloud's end repeat its
    last row.  No augmentation stages and no height column in this mode."""

    def __init__(self, cloud_set, batch_size, npoints, recipe, train, shuffle=True, drop_last=False, seed=0, draws="device", rank=0,
                 world_size=1, ahead=2, use_height=False, augment=None, ragged=False):
        if recipe not in RECIPES:
            raise ValueError(f"recipe must be one of {RECIPES}, got {recipe!r}")
        if draws not in ("device", "numpy"):
            raise ValueError(f"draws must be 'device' or 'numpy', got {draws!r}")
        if not 1 <= int(npoints) <= MAX_NPOINTS:
            raise ValueError(f"npoints must be in [1, {MAX_NPOINTS}], got {npoints}")
        if int(batch_size) < 1 or int(ahead) < 1:
            raise ValueError("batch_size and ahead must be at least 1")
        self.set, self.batch_size, self.npoints, self.recipe, self.train = cloud_set, int(batch_size), int(npoints), recipe, bool(train)
        self.shuffle, self.drop_last, self.seed, self.draws = bool(shuffle), bool(drop_last), int(seed), draws
        self.rank, self.world_size, self.ahead, self.epoch = int(rank), int(world_size), int(ahead), 0
        self.use_height = bool(use_height)     # pc [B, npoints, 4]: the height column, taken after augmentation and shuffle (dataset_3d.py:306-314)
        self.augment = () if augment is None else check_stages(augment)
        own = SHAPENET_CHAIN if recipe == "shapenet55" and self.train else ()
        self._aug_stages = check_stages(own + self.augment, f"recipe {recipe!r} with augment")      # () = today's launches, nothing more
        if len(self._aug_stages) + self.use_height > 8:
            raise ValueError("at most 8 augmentation stages in one launch, the height column included")
        self._permutation = np.arange(self.npoints)      # "shapenet55", numpy draws: ShapeNet.permutation (:545), shuffled cumulatively
        epoch_indices(1, rank=self.rank, world_size=self.world_size)          # validates rank / world_size
        rows = cloud_set.rows(np.arange(len(cloud_set)))
        if recipe == "shapenetpart":
            if cloud_set.seg is None:
                raise ValueError("recipe 'shapenetpart' needs a DeviceCloudSet with seg")
        else:
            if rows.min() < self.npoints:
                raise ValueError(f"recipe {recipe!r}: every cloud needs at least npoints = {self.npoints} rows (shortest: {rows.min()})")
            if recipe in FPS_RECIPES and rows.min() != rows.max() and not ragged:
                raise ValueError(f"recipe {recipe!r}: the batched FPS launch walks one row count for all its clouds; give clouds of one "
                                 "length (ModelNet's are), e.g. one DeviceCloudSet per length, or pass ragged=True (one FPS launch "
                                 "that takes every cloud's own length)")
        # ragged: the set's lengths differ and the FPS launch takes them (ops.fps(lengths=)); a uniform set is today's path
        self._ragged = bool(ragged) and recipe in FPS_RECIPES and rows.min() != rows.max()
        self.ragged = self._whole = bool(ragged) and recipe == "shapenetpart"          # whole shapes: batches carry lengths
        if self._whole:
            if self._aug_stages or self.use_height:
                raise ValueError("recipe 'shapenetpart', ragged: no augmentation stages and no height column on whole shapes")
            if cloud_set.points.shape[1] > MAX_NPOINTS:
                raise ValueError(f"recipe 'shapenetpart', ragged: the set's clouds are padded to {cloud_set.points.shape[1]} rows, "
                                 f"over the {MAX_NPOINTS} one batch row may have")
        self._exact = self._ragged and bool((rows == self.npoints).any())     # clouds of exactly npoints rows: no FPS for those
        if self._exact and recipe == "shapenet55":
            raise ValueError(f"recipe 'shapenet55', ragged: a cloud of exactly npoints = {self.npoints} rows takes random_sample's "
                             "persistent permutation, not FPS; keep such clouds in a set of their own")
        if self._ragged:
            self._fps_rows = int(rows.max())
        else:
            self._fps_rows = int(rows[0]) if recipe in FPS_RECIPES and rows[0] > self.npoints else 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self):
        """this rank's dataset indices for the current epoch"""
        return epoch_indices(len(self.set), self.epoch, self.shuffle, self.seed, self.drop_last, self.rank, self.world_size)

    def __len__(self):
        n = len(epoch_indices(len(self.set), 0, False, 0, self.drop_last, self.rank, self.world_size))
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    def _recipe_draws(self):
        """which of ppt_cloud_draws' outputs the recipe itself needs"""
        part, sn = self.recipe == "shapenetpart", self.recipe == "shapenet55"
        translate = self.train and self.recipe in ("modelnet", "scanobjectnn")
        return dict(start=self._fps_rows > 0, affine=translate, perm=translate or (sn and not self._fps_rows), sel=part and not self._whole)

    def plan(self):
        """The launches one batch takes, in order (names of ppt_amd.ops functions); numpy draws add one host-to-device copy instead
        of the draw launches."""
        p = []
        if self.draws == "device":
            p += ["cloud_draws"] if any(self._recipe_draws().values()) else []
            p += ["cloud_draws_aug"] if self._aug_stages else []
        p += ["fps"] if self._fps_rows else []
        p.append("cloud_prep")
        if self._aug_stages:
            p.append("cloud_augment")     # the height column, if any, is its last stage
        elif self.use_height:
            p.append("cloud_height")
        return tuple(p)

    # ---- one batch, queued on the current (= the grouping) stream ------------------------------------------------------------
    def _host_draws(self, rs, idx):
        """numpy mode: the batch's draws in ONE pinned buffer (a single asynchronous copy), viewed per array on the device."""
        B, n = len(idx), self.npoints
        rows = self.set.rows(idx)
        per = [numpy_draws(rs, self.recipe, self.train, int(r), n, self.augment, self._permutation) for r in rows]
        parts = {}
        if any("start" in d for d in per):                # (ragged: a cloud of exactly npoints rows draws none and is not sampled)
            parts["start"] = np.asarray([d.get("start", 0) for d in per], dtype=np.int64)
        if "scale" in per[0]:
            parts["scale"] = np.stack([d["scale"] for d in per]).astype(np.float64)
            parts["shift"] = np.stack([d["shift"] for d in per]).astype(np.float64)
        if "sel" in per[0]:
            parts["sel"] = np.stack([d["sel"] for d in per]).astype(np.int64)
        for k in per[0]:
            if k.startswith("aug_") and k[4:] in KERNEL_PARAMS:                            # what the kernel reads: f64, but for the mask
                parts[k] = np.stack([np.asarray(d[k]) for d in per])
        if "perm" in per[0]:
            parts["perm"] = np.stack([d["perm"] for d in per]).astype(np.int32)            # after the 8-byte arrays: 4-byte items
        if "aug_mask" in parts:
            parts["aug_mask"] = parts.pop("aug_mask")                                      # last: single bytes
        if not parts:
            return {}
        total = sum(a.nbytes for a in parts.values())
        pin = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        host, off, spans = pin.numpy(), 0, {}
        for k, a in parts.items():
            host[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
            spans[k] = (off, a.nbytes, a.shape, a.dtype)
            off += a.nbytes
        dev = pin.to(self.set.device, non_blocking=True)
        tdt = {np.dtype(np.int64): torch.int64, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
               np.dtype(np.uint8): torch.uint8}
        return {k: dev[o:o + nb].view(tdt[np.dtype(dt)]).view(*shape) for k, (o, nb, shape, dt) in spans.items()}

    def _produce(self, item, idx, rs):
        from .. import ops
        s, n = self.set, self.npoints
        part = self.recipe == "shapenetpart"
        if self._whole:
            # every stored row: rows behind a cloud's end come out as copies of its last row (cloud_prep clamps), their labels -100
            rows_all = s.points.shape[1]
            pc, seg = ops.cloud_prep(s.points, item, rows_all, lengths=s.lengths, seg_src=s.seg)
            rows = s.rows(idx).astype(np.int32)
            lens = torch.full((len(idx),), rows_all, dtype=torch.int32, device=pc.device) if s.lengths is None else s.lengths.index_select(0, item)
            seg.masked_fill_(torch.arange(rows_all, device=pc.device).unsqueeze(0) >= lens.unsqueeze(1), -100)
            lens._ppt_total = int(rows.sum())
            return (pc, s.labels.index_select(0, item).to(torch.int32).view(-1, 1), seg, lens)
        want = self._recipe_draws()
        if self.draws == "numpy":
            d = self._host_draws(rs, idx)
        else:
            d = {}                        # (a test split that takes the stored rows as they are: nothing is drawn)
            if any(want.values()):
                rows = None if s.lengths is None else s.lengths.index_select(0, item)
                d = ops.cloud_draws(item, n, self.seed, self.epoch, rows=rows, rows_all=s.points.shape[1], **want)
            if self._aug_stages:
                aug = ops.cloud_draws_aug(item, n, self.seed, self.epoch, **{st: True for st in self._aug_stages})
                d.update({"aug_" + k: v for k, v in aug.items()})
        sel = d.get("sel")
        if self.recipe == "shapenet55" and not self._fps_rows:
            sel = d["perm"].to(torch.int64) if sel is None else sel      # random_sample: the rows in shuffled order, normalised in that order
            d = {k: v for k, v in d.items() if k != "perm"}
        if self._fps_rows:
            xyz = s.points.index_select(0, item)
            if xyz.shape[1] != self._fps_rows or xyz.shape[2] != 3:
                xyz = xyz[:, :self._fps_rows, :3].contiguous()
            if self._ragged:
                lens = s.lengths.index_select(0, item)
                start = d.get("start")    # numpy draws, a batch made of npoints-row clouds only: none of them drew a start
                if start is None:
                    start = torch.zeros(len(idx), dtype=torch.int64, device=xyz.device)
                sel, _ = ops.fps(xyz, n, start, lengths=lens)
                if self._exact:           # dataset_3d.py:300-303: a cloud of npoints rows is taken as stored
                    sel = torch.where((lens == n).unsqueeze(1), torch.arange(n, device=sel.device).unsqueeze(0), sel)
            else:
                sel, _ = ops.fps(xyz, n, d["start"])
        out = ops.cloud_prep(s.points, item, n, sel=sel, lengths=s.lengths, normalize=self.recipe in FPS_RECIPES, scale=d.get("scale"),
                             shift=d.get("shift"), perm=d.get("perm"), seg_src=s.seg if part else None)
        target = s.labels.index_select(0, item)
        if self._aug_stages:              # one more launch: the stages in order, the height column in its tail
            aug = {k[4:]: v for k, v in d.items() if k.startswith("aug_")}
            pc = ops.cloud_augment(out[0] if part else out, [kernel_stage(st, aug) for st in self._aug_stages], height=self.use_height)
            return (pc, target.to(torch.int32).view(-1, 1), out[1]) if part else (pc, target)
        if part:
            return (add_height(out[0]) if self.use_height else out[0], target.to(torch.int32).view(-1, 1), out[1])
        return (add_height(out) if self.use_height else out, target)

    def __iter__(self):
        from .. import graphs
        dev = self.set.device
        if dev.type != "cuda":
            raise RuntimeError("DeviceBatchLoader runs on the HIP device (libppt_hip.so: ppt_cloud_prep_f32); there is no CPU path")
        order = self.indices()
        nb = len(self)
        group = graphs.shared_group_stream(dev)
        rs = np.random.RandomState([self.seed, self.epoch, self.rank]) if self.draws == "numpy" else None
        with torch.cuda.stream(group):
            order_dev = torch.from_numpy(order).pin_memory().to(dev, non_blocking=True)      # the epoch's order: one copy, up front
        queue = collections.deque()
        state = {"next": 0}

        def put():
            i = state["next"]
            if i >= nb:
                return
            state["next"] = i + 1
            lo, hi = i * self.batch_size, min((i + 1) * self.batch_size, len(order))
            with torch.cuda.stream(group):
                batch = self._produce(order_dev[lo:hi], order[lo:hi], rs)
                ev = torch.cuda.Event()
                ev.record(group)
            for t in batch:
                t._ppt_ready = ev
            queue.append((batch, ev))
        for _ in range(self.ahead):
            put()
        while queue:
            batch, ev = queue.popleft()
            cur = torch.cuda.current_stream(dev)
            cur.wait_event(ev)
            for t in batch:
                t.record_stream(cur)
            put()
            yield batch
