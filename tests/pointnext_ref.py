"""CPU restatement of the PointNeXt-S forward (PointNEXT(): models/pointnext/pointnext-s.yaml; backbone/pointnext.py:81-170,
311-443, layers/group.py:177-272, classification/cls_base.py:78-140), written from the semantics of its three compiled ops
(sampling_gpu.cu:100-216, ball_query_gpu.cu:15-51) -- not from the code under test.

The index stand-ins are uncontracted fp32 (numpy float32 arithmetic, one rounding per operation): no machine here runs the
extension's CUDA, whose expressions nvcc contracts into FMAs by default, so the reference pins no rounding of its own and index
equality between these stand-ins and the device kernels is the contract.

The tensor arithmetic runs in `dtype` (fp32 or fp64); `round_op` (None, torch.float16, torch.bfloat16) rounds both operands of
every matrix product to that format first -- the arithmetic model of the 16-bit operand modes."""
import numpy as np
import torch

RADII = []
_r = 0.15
for _ in range(4):          # PointNextEncoder._to_full_list: x 1.5 after every strided stage, in Python floats
    RADII.append(_r)
    _r *= 1.5
NSAMPLE = 32
EPS, MOMENTUM = 1e-5, 0.1


def fps_from_zero(xyz, S):
    """furthest_point_sampling_kernel: start at index 0, running minimum initialised to 1e10, direct-form fp32 distance
    (dx*dx + dy*dy) + dz*dz, FIRST maximum on ties.  xyz [B,N,3] float32 array -> [B,S] int64."""
    xyz = np.asarray(xyz, np.float32)
    B, N, _ = xyz.shape
    out = np.zeros((B, S), np.int64)
    for b in range(B):
        p = xyz[b]
        mind = np.full((N,), 1e10, np.float32)
        cur = 0
        for j in range(1, S):
            d = p - p[cur]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            mind = np.minimum(mind, d2)
            cur = int(np.argmax(mind))
            out[b, j] = cur
    return out


def ball_query_lt(xyz, center, radius, K):
    """ball_query_kernel_fast: first K indices in ascending order with (dx*dx + dy*dy) + dz*dz < float32(r) * float32(r) (strict),
    padded with the first hit; zeros when nothing hits.  xyz [B,N,3], center [B,S,3] float32 arrays -> [B,S,K] int64."""
    xyz, center = np.asarray(xyz, np.float32), np.asarray(center, np.float32)
    B, N, _ = xyz.shape
    S = center.shape[1]
    r2 = np.float32(radius) * np.float32(radius)
    out = np.zeros((B, S, K), np.int64)
    for b in range(B):
        d = center[b][:, None, :] - xyz[b][None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        for s in range(S):
            hits = np.nonzero(d2[s] < r2)[0][:K]
            if hits.size:
                out[b, s, :hits.size] = hits
                out[b, s, hits.size:] = hits[0]
    return out


def group_indices(xyz):
    """The four (FPS indices [B,S], neighbour indices [B,S,K]) pairs of a cloud batch xyz [B,N,3] float32."""
    out, p = [], np.asarray(xyz, np.float32)
    for r in RADII:
        ci = fps_from_zero(p, p.shape[1] // 2)
        q = np.take_along_axis(p, ci[:, :, None], 1)
        out.append((ci, ball_query_lt(p, q, r, NSAMPLE)))
        p = q
    return out


def cloud_height(pc):
    """data/dataset_3d.py:311-314 on a batch: [B,N,3] float32 -> [B,N,4]."""
    pc = np.asarray(pc, np.float32)
    return np.concatenate([pc, pc[:, :, 1:2] - pc[:, :, 1:2].min(axis=1, keepdims=True)], axis=2)


def forward(sd, pc4, train, drop_masks=None, dtype=torch.float32, round_op=None, indices=None, prefix=""):
    """-> (out [B,256] `dtype`, {running-statistics key: updated value}, indices).  sd: name -> tensor (not modified)."""
    D = dtype
    pc4 = torch.as_tensor(pc4, dtype=torch.float32)
    B, N, _ = pc4.shape
    stats = {}

    def R(t):
        return t if round_op is None else t.to(round_op).to(D)

    def W(key):
        w = sd[prefix + key].detach().to(D)
        return w.reshape(w.shape[0], -1)

    def mm(x, key):
        return R(x) @ R(W(key)).t()

    def bn(y, q):
        """BatchNorm over every leading dimension of y [..., C]."""
        g, be = sd[prefix + q + "weight"].to(D), sd[prefix + q + "bias"].to(D)
        rm, rv = sd[prefix + q + "running_mean"].to(D), sd[prefix + q + "running_var"].to(D)
        if train:
            flat = y.reshape(-1, y.shape[-1])
            n = flat.shape[0]
            mean, var = flat.mean(0), flat.var(0, unbiased=False)
            stats[prefix + q + "running_mean"] = (1 - MOMENTUM) * rm + MOMENTUM * mean
            stats[prefix + q + "running_var"] = (1 - MOMENTUM) * rv + MOMENTUM * var * (n / max(n - 1, 1))
        else:
            mean, var = rm, rv
        return (y - mean) / torch.sqrt(var + EPS) * g + be

    xyz = pc4[..., :3].contiguous()
    if indices is None:
        indices = group_indices(xyz.numpy())
    e = "encoder.encoder."
    f = mm(pc4.to(D), e + "0.0.convs.0.0.weight") + sd[prefix + e + "0.0.convs.0.0.bias"].to(D)        # [B,N,32]
    p = xyz
    bi = torch.arange(B).view(B, 1)
    for i, (r, (ci, ni)) in enumerate(zip(RADII, indices)):
        q = f"{e}{i + 1}.0."
        ci, ni = torch.as_tensor(ci), torch.as_tensor(ni)
        new_p = p[bi, ci]                                                   # [B,S,3] fp32
        ident = mm(f[bi, ci], q + "skipconv.0.weight") + sd[prefix + q + "skipconv.0.bias"].to(D)
        dp = (p[bi.view(B, 1, 1), ni].to(D) - new_p.to(D)[:, :, None, :]) / float(np.float32(r))     # [B,S,K,3]
        fj = f[bi.view(B, 1, 1), ni]                                        # [B,S,K,C]
        y = torch.relu(bn(mm(torch.cat([dp, fj], -1), q + "convs.0.0.weight"), q + "convs.0.1."))
        y = bn(mm(y, q + "convs.1.0.weight"), q + "convs.1.1.")
        f = torch.relu(y.max(dim=2)[0] + ident)
        p = new_p
    q = e + "5.0."
    y = torch.cat([p.to(D), f], -1)                                         # GroupAll: [absolute xyz | features]
    y = torch.relu(bn(mm(y, q + "convs.0.0.weight"), q + "convs.0.1."))
    y = torch.relu(bn(mm(y, q + "convs.1.0.weight"), q + "convs.1.1."))
    x = y.max(dim=1)[0]                                                     # [B,512]
    for j, m in ((0, 0), (2, 1)):
        h = f"prediction.head.{j}."
        x = torch.relu(bn(mm(x, h + "0.weight"), h + "1."))
        if train and drop_masks is not None:
            x = x * torch.as_tensor(drop_masks[m]).to(D)
    return x, stats, indices
