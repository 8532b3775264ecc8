"""A torch reference for part segmentation on a padded ragged batch (tests/test_ragged_partseg_{cpu,gpu}.py).

The part of the model that works on fixed anchor sets -- grouping, tokenizer, the 12 blocks, propagation_1/2, dgcnn_pro_1/2 -- is the
CPU oracle's own functions, fed with each cloud's FPS / kNN results at its own length.  The N-dependent tail is written out here,
in float64, on rows this file packs itself: [one-hot | xyz | 3-NN interpolation], propagation_0's two conv + BatchNorm + ReLU
layers, conv1 + bn1 + ReLU, dropout mask, projection, logits -- BatchNorm over the R = sum(lengths) rows that exist."""
import numpy as np
import torch

from oracle import oracle as O


def three_nn_f64(xyz1, xyz2):
    """3 nearest sources of every target by squared distance (torch.cdist, float64), ties to the lower index -> (idx [N,3],
    weights [N,3] = (1 / (d + 1e-8)) normalised: pointnet2_utils.py:333-347)"""
    d = torch.cdist(xyz1.double(), xyz2.double()) ** 2
    order = torch.argsort(d, dim=1, stable=True)[:, :3]
    dd = torch.gather(d, 1, order)
    recip = 1.0 / (dd + 1e-8)
    return order, recip / recip.sum(dim=1, keepdim=True)


def conv_bn_relu_f64(x, sd, conv, bn, train, new_stats=None, eps=1e-5, momentum=0.1):
    """relu(bn(conv(x))) over rows x [M, K] in float64; train: biased batch statistics over the M rows, running buffers with the
    unbiased variance into new_stats"""
    w = sd[conv + "weight"]
    y = x @ w.reshape(w.shape[0], -1).double().t() + sd[conv + "bias"].double()
    if train:
        mean, var = y.mean(0), y.var(0, unbiased=False)
        if new_stats is not None:
            n = y.shape[0]
            new_stats[bn + "running_mean"] = (1 - momentum) * sd[bn + "running_mean"].double() + momentum * mean.detach()
            new_stats[bn + "running_var"] = (1 - momentum) * sd[bn + "running_var"].double() + momentum * var.detach() * (n / (n - 1))
    else:
        mean, var = sd[bn + "running_mean"].double(), sd[bn + "running_var"].double()
    return torch.relu((y - mean) / torch.sqrt(var + eps) * sd[bn + "weight"].double() + sd[bn + "bias"].double())


def fp_tail_f64(sd, p, xyz1_list, xyz2, points1_list, points2, train, new_stats=None):
    """PointNetFeaturePropagation on packed targets: xyz1_list / points1_list one [n_b, 3] / [n_b, D1] tensor per cloud, xyz2
    [B,S,3], points2 [B,S,D2] -> [R, C] float64"""
    rows = []
    for b, (x1, p1) in enumerate(zip(xyz1_list, points1_list)):
        idx, w = three_nn_f64(x1, xyz2[b])
        interp = (points2[b].double()[idx] * w[..., None]).sum(dim=1)
        rows.append(torch.cat([p1.double(), interp], dim=1))
    x = torch.cat(rows)
    for j in range(2):
        x = conv_bn_relu_f64(x, sd, f"{p}mlp_convs.{j}.", f"{p}mlp_bns.{j}.", train, new_stats)
    return x


def fp_exact_rows(sd, p, xyz1, xyz2, points1, points2, train):
    """fp_tail_f64 on a UNIFORM batch, reshaped to [B,N,C]: what tests/decoder_ref.py's fp_exact computes"""
    B, N, _ = xyz1.shape
    out = fp_tail_f64(sd, p, [xyz1[b] for b in range(B)], xyz2, [points1[b] for b in range(B)], points2, train)
    return out.reshape(B, N, -1)


def partseg_logits_ragged(sd, pc, lengths, onehot, fps_starts, embedding, name_lengths, eot_pos, train=False, dp_masks=None,
                          drop_mask=None, new_stats=None, prefix="point_encoder."):
    """ULIP part-seg on the padded batch pc [B,Nmax,3] (numpy; rows >= lengths[b] never looked at) -> packed logits [R,C] float64.
    drop_mask [B,Nmax,128] padded.  sd may hold tensors that require grad."""
    B = len(lengths)
    clouds = [np.ascontiguousarray(pc[b:b + 1, :n]) for b, n in enumerate(lengths)]
    s0, s1, s2 = (np.asarray(s) for s in fps_starts)
    nb, ce, c1, c2 = [], [], [], []
    for b, c in enumerate(clouds):
        _, nb_b, ce_b = O.group(c, O.fps(c, 512, s0[b:b + 1]), 32)
        nb.append(nb_b); ce.append(ce_b)
        c1.append(np.take_along_axis(c, O.fps(c, 512, s1[b:b + 1])[:, :, None], axis=1))
        c2.append(np.take_along_axis(c, O.fps(c, 256, s2[b:b + 1])[:, :, None], axis=1))
    nb, ce, c1, c2 = (np.concatenate(a) for a in (nb, ce, c1, c2))
    x, pos = O.point_tokens(sd, torch.from_numpy(nb), torch.from_numpy(ce), train, prefix, new_stats)
    feats = []
    for l in range(12):
        dp = dp_masks[l] if dp_masks is not None else (None, None)
        x = O.vit_block(sd, f"{prefix}blocks.blocks.{l}.", x + pos, 6, dp[0], dp[1])
        if l in (3, 7, 11):
            feats.append(O.layer_norm(x, sd[prefix + "norm.weight"], sd[prefix + "norm.bias"])[:, 1:])
    f2 = O.feature_propagation(sd, prefix + "propagation_2.", c2, ce, torch.from_numpy(c2), feats[1], train, new_stats)
    f1 = O.feature_propagation(sd, prefix + "propagation_1.", c1, ce, torch.from_numpy(c1), feats[0], train, new_stats)
    f2 = O.dgcnn_propagation(sd, prefix + "dgcnn_pro_2.", ce, feats[2], c2, f2)
    f1 = O.dgcnn_propagation(sd, prefix + "dgcnn_pro_1.", c2, f2, c1, f1)
    xyz = [torch.from_numpy(c[0]) for c in clouds]
    p1 = [torch.cat([onehot[b][None].expand(len(x_), -1), x_], dim=1) for b, x_ in enumerate(xyz)]
    f0 = fp_tail_f64(sd, prefix + "propagation_0.", xyz, torch.from_numpy(c1), p1, f1, train, new_stats)
    y = conv_bn_relu_f64(f0, sd, prefix + "conv1.", prefix + "bn1.", train, new_stats)
    if drop_mask is not None:
        y = y * torch.cat([drop_mask[b, :n] for b, n in enumerate(lengths)]).double()
    prompts = O.splice_prompts(embedding, sd["prompt_learner.learnable_tokens"], name_lengths, "middle")
    te = O.text_tower(sd, prompts, eot_pos).double()
    te = te / te.norm(dim=-1, keepdim=True)
    return sd["logit_scale"].double().exp() * (y @ sd["pc_projection"].double()) @ te.t()
