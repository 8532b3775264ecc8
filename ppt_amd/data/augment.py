"""The reference's point-cloud augmentations (data/dataset_3d.py:63-153) on device batches, by their reference names.

    rotate_point_cloud (:63)   random_point_dropout (:83)   random_scale_point_cloud (:92)   shift_point_cloud (:105)
    jitter_point_cloud (:118)  rotate_perturbation_point_cloud (:131)

Each takes pc [B, n, 3] float32 on the device and returns a NEW tensor (the reference's dropout / scale / shift work in place and
return their argument); one launch of csrc/cloud_augment.hip does the arithmetic, numpy's operation by operation.  The draws come
from one of two places, as in device_loader.py:

    rs=np.random.RandomState   the reference's draws in the reference's order for a [B, n, 3] batch (`host_stage_draws`): given the
                               same generator state the result is bit-identical to the reference function's -- for the two
                               rotations up to the last bit of numpy's BLAS product, see tests/test_augment_gpu.py.
    seed=, epoch=, index=      ppt_cloud_draws_aug: Philox4x32-10 with the counter (index[b], epoch, slot, block); index [B] i64
                               device tensor (None: 0 .. B-1).  A sample's draws do not depend on the batch it is in.

jitter_point_cloud returns float32: the reference returns the float64 array `clip(sigma * randn) + batch_data`; here that sum is
rounded once to float32, the dtype every consumer converts to anyway (`torch.from_numpy(data).float()`).

`DeviceBatchLoader(augment=(...))` chains the same stages inside the loader's own launch; ShapeNet's chain (:590-595) is the
"shapenet55" recipe.
"""
import numpy as np
import torch

STAGES = ("dropout", "scale", "shift", "rotate_perturbation", "rotate", "jitter")
SHAPENET_CHAIN = ("dropout", "scale", "shift", "rotate_perturbation", "rotate")               # ShapeNet.__getitem__, :591-595
# stage name -> (the kernel's stage, the draw that parameterises it)
KERNEL_STAGE = {"dropout": ("dropout", "mask"), "scale": ("scale", "scale"), "shift": ("shift", "shift"),
                "rotate_perturbation": ("rotate", "perturb"), "rotate": ("rotate", "rotate"), "jitter": ("jitter", "noise")}
DEFAULTS = dict(max_dropout=0.875, scale_low=0.8, scale_high=1.25, shift_range=0.1, angle_sigma=0.06, angle_clip=0.18,
                jitter_sigma=0.01, jitter_clip=0.05)


def check_stages(names, what="augment"):
    """-> the tuple of stage names; ValueError for an unknown or a repeated one (a repeated stage would repeat its device draws)"""
    names = tuple(names)
    for s in names:
        if s not in STAGES:
            raise ValueError(f"{what}: unknown stage {s!r}; one of {STAGES}")
    if len(set(names)) != len(names):
        raise ValueError(f"{what}: a stage may appear once, got {names}")
    return names


def perturbation_matrix(angles):
    """dataset_3d.py:141-150, statement by statement"""
    Rx = np.array([[1, 0, 0], [0, np.cos(angles[0]), -np.sin(angles[0])], [0, np.sin(angles[0]), np.cos(angles[0])]])
    Ry = np.array([[np.cos(angles[1]), 0, np.sin(angles[1])], [0, 1, 0], [-np.sin(angles[1]), 0, np.cos(angles[1])]])
    Rz = np.array([[np.cos(angles[2]), -np.sin(angles[2]), 0], [np.sin(angles[2]), np.cos(angles[2]), 0], [0, 0, 1]])
    return np.dot(Rz, np.dot(Ry, Rx))


def up_axis_matrix(angle):
    """dataset_3d.py:74-78"""
    cosval, sinval = np.cos(angle), np.sin(angle)
    return np.array([[cosval, 0, sinval], [0, 1, 0], [-sinval, 0, cosval]])


def host_stage_draws(rs, stage, B, n, **mag):
    """The draws the reference function of `stage` makes for a [B, n, 3] batch, from the np.random.RandomState `rs`, in its order.
    -> dict of numpy arrays, named as ops.cloud_draws_aug names them (dropout also keeps its uniforms as `u` [B, n])."""
    m = dict(DEFAULTS, **mag)
    if stage == "dropout":                                                             # :85-87, per cloud: random(), random(n)
        ratio, u = np.empty(B), np.empty((B, n))
        for b in range(B):
            ratio[b] = rs.random_sample() * m["max_dropout"]
            u[b] = rs.random_sample((n,))
        return {"ratio": ratio, "u": u, "mask": (u <= ratio[:, None]).astype(np.uint8)}
    if stage == "scale":
        return {"scale": rs.uniform(m["scale_low"], m["scale_high"], B)}               # :100
    if stage == "shift":
        return {"shift": rs.uniform(-m["shift_range"], m["shift_range"], (B, 3))}      # :113
    if stage == "rotate_perturbation":                                                 # :140, per cloud: randn(3)
        angles = np.stack([np.clip(m["angle_sigma"] * rs.randn(3), -m["angle_clip"], m["angle_clip"]) for _ in range(B)])
        return {"angles": angles, "perturb": np.stack([perturbation_matrix(a) for a in angles])}
    if stage == "rotate":                                                              # :73, per cloud: uniform()
        angle = np.array([rs.uniform() * 2 * np.pi for _ in range(B)])
        return {"angle": angle, "rotate": np.stack([up_axis_matrix(a) for a in angle])}
    if stage == "jitter":
        assert m["jitter_clip"] > 0
        return {"noise": np.clip(m["jitter_sigma"] * rs.randn(B, n, 3), -1 * m["jitter_clip"], m["jitter_clip"])}      # :127
    raise ValueError(f"unknown stage {stage!r}; one of {STAGES}")


def kernel_stage(stage, draws):
    """the ops.cloud_augment stage tuple of `stage`, from a dict of device tensors named as ops.cloud_draws_aug names them"""
    kind, key = KERNEL_STAGE[stage]
    return (kind, draws[key])


def _apply(pc, stage, rs, seed, epoch, index, **mag):
    from .. import ops
    if not torch.is_tensor(pc) or pc.dim() != 3 or pc.shape[2] != 3 or pc.dtype != torch.float32:
        raise ValueError("a [B, n, 3] float32 device tensor is expected")
    if (rs is None) == (seed is None):
        raise ValueError("give either rs= (a numpy RandomState: the reference's draws) or seed= (device draws)")
    pc = pc.contiguous()
    B, n, _ = pc.shape
    key = KERNEL_STAGE[stage][1]
    if rs is not None:
        d = {key: torch.from_numpy(np.ascontiguousarray(host_stage_draws(rs, stage, B, n, **mag)[key])).to(pc.device)}
    else:
        if index is None:
            index = torch.arange(B, dtype=torch.int64, device=pc.device)
        d = ops.cloud_draws_aug(index, n, seed, epoch, **{stage: True}, **mag)
    return ops.cloud_augment(pc, [kernel_stage(stage, d)])


def rotate_point_cloud(batch_data, *, rs=None, seed=None, epoch=0, index=None):
    """dataset_3d.py:63 -- one rotation about the up (y) axis per cloud"""
    return _apply(batch_data, "rotate", rs, seed, epoch, index)


def random_point_dropout(batch_pc, max_dropout_ratio=0.875, *, rs=None, seed=None, epoch=0, index=None):
    """dataset_3d.py:83 -- a random share (below max_dropout_ratio) of each cloud's rows becomes copies of its row 0"""
    return _apply(batch_pc, "dropout", rs, seed, epoch, index, max_dropout=max_dropout_ratio)


def random_scale_point_cloud(batch_data, scale_low=0.8, scale_high=1.25, *, rs=None, seed=None, epoch=0, index=None):
    """dataset_3d.py:92 -- one scale per cloud"""
    return _apply(batch_data, "scale", rs, seed, epoch, index, scale_low=scale_low, scale_high=scale_high)


def shift_point_cloud(batch_data, shift_range=0.1, *, rs=None, seed=None, epoch=0, index=None):
    """dataset_3d.py:105 -- one shift per cloud and axis"""
    return _apply(batch_data, "shift", rs, seed, epoch, index, shift_range=shift_range)


def jitter_point_cloud(batch_data, sigma=0.01, clip=0.05, *, rs=None, seed=None, epoch=0, index=None):
    """dataset_3d.py:118 -- clipped normal noise per coordinate.  float32 (the reference returns float64; see the module text)."""
    if not clip > 0:
        raise ValueError("clip must be positive")
    return _apply(batch_data, "jitter", rs, seed, epoch, index, jitter_sigma=sigma, jitter_clip=clip)


def rotate_perturbation_point_cloud(batch_data, angle_sigma=0.06, angle_clip=0.18, *, rs=None, seed=None, epoch=0, index=None):
    """dataset_3d.py:131 -- a small rotation Rz (Ry Rx) per cloud"""
    return _apply(batch_data, "rotate_perturbation", rs, seed, epoch, index, angle_sigma=angle_sigma, angle_clip=angle_clip)
