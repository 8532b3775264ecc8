#!/usr/bin/env python3
"""Generate tests/golden/g_pointnext.npz by running the UPSTREAM REFERENCE's PointNEXT() (models/pointnext/pointnext.py: BaseCls of
pointnext-s.yaml) on the CPU.  Build container only (see make_golden.py).

    python tests/golden/make_golden_pointnext.py

The reference reaches FPS, the ball query and the grouping gather through its compiled extension `pointnet2_batch_cuda`; that module
is replaced in sys.modules by an empty stand-in and the three entry points used on this path (furthest_point_sample, ball_query,
grouping_operation) by the uncontracted fp32 restatements of tests/pointnext_ref.py / a torch gather.  No machine here runs the
extension's CUDA and nvcc contracts its distance expressions into FMAs by default, so the reference pins no rounding of its own: the
stand-ins ARE the fixture's index semantics.  Four imports that are not installed (multimethod, termcolor, shortuuid, easydict) are
stubbed in sys.modules; the yaml is turned into an EasyConfig by hand (EasyConfig.load relies on multimethod's overloading).
Weights come from ppt_amd.weights.pointnext_spec (name-keyed generator) and are not stored.

Stored: the clouds of the N = 200 cases, the injected Dropout masks, the reference outputs, every running statistic the train cases
update, the four (FPS, ball query) index tensors of the N = 200 eval case, and per case
  ref_err_*: max |reference fp32 - fp64 restatement| / max |reference|  (outputs; for train also over the running statistics),
  e16_{f16,bf16}_*: the same for the restatement with operands rounded to IEEE half / bf16 against the fp64 restatement."""
import os
import sys
import types

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_import as R                     # noqa: E402
import pointnext_ref as P                  # noqa: E402
from ppt_amd import weights as W           # noqa: E402

torch.set_num_threads(8)


def clouds_200(B, seed):
    """B clouds of 200 points with height; cloud 1 carries 25 % exact duplicates; cloud 2 has point 1 at distance exactly
    float32(0.15) from point 0 -- FPS starts at 0, so point 0 is a centre of stage 1 -- along x: `<` leaves it out, `<=` takes it."""
    pc, _ = W.synth_clouds(B, 200, seed=seed)
    rng = np.random.default_rng(seed)
    if B > 1:
        dst = rng.choice(200, size=50, replace=False)
        src = rng.choice(np.setdiff1d(np.arange(200), dst), size=50, replace=False)
        pc[1, dst] = pc[1, src]
    if B > 2:
        pc[2, 0, 0] = 0.0
        pc[2, 1] = pc[2, 0]
        pc[2, 1, 0] = np.float32(0.15)
    return P.cloud_height(pc)


def build_reference():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    mod("multimethod", multimethod=lambda f: f)
    mod("shortuuid", uuid=lambda: "0")
    mod("pointnet2_batch_cuda")
    with R.reference_context():
        pdir = os.path.join(R.REF_ROOT, "models", "pointnext", "PointNeXt")
        sys.path.insert(0, pdir)
        try:
            from openpoints.utils import EasyConfig
            from openpoints.models import build_model_from_cfg
            from openpoints.models.layers import group as G
            from openpoints.models.backbone import pointnext as PN

            def fps(xyz, npoint):
                return torch.from_numpy(P.fps_from_zero(xyz.detach().numpy(), npoint)).int()

            def ball_query(radius, nsample, xyz, new_xyz):
                return torch.from_numpy(P.ball_query_lt(xyz.detach().numpy(), new_xyz.detach().numpy(), radius, nsample)).int()

            def grouping_operation(features, idx):              # features [B,C,N], idx [B,S,K] -> [B,C,S,K]
                B, C, _ = features.shape
                _, S, K = idx.shape
                return torch.gather(features, 2, idx.long().view(B, 1, S * K).expand(B, C, S * K)).view(B, C, S, K)
            PN.furthest_point_sample = fps
            G.ball_query = ball_query
            G.grouping_operation = grouping_operation

            def easy(d):
                c = EasyConfig()
                for k, v in d.items():
                    dict.__setitem__(c, k, easy(v) if isinstance(v, dict) else v)
                return c
            cfg = easy(yaml.safe_load(open(os.path.join(R.REF_ROOT, "models", "pointnext", "pointnext-s.yaml"))))
            model = build_model_from_cfg(cfg.model)
        finally:
            sys.path.remove(pdir)
    return model


class InjectedDropout(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.mask = None

    def forward(self, x):
        return x * self.mask if self.training and self.mask is not None else x


def main():
    ref = build_reference()
    sd = W.synth_state_dict(W.pointnext_spec(prefix=""), seed=0)
    assert list(ref.state_dict().keys()) == list(sd.keys()), "weights.pointnext_spec is not the reference's key list"
    assert sum(p.numel() for p in ref.parameters()) == 1363264
    drops = [InjectedDropout(), InjectedDropout()]
    ref.prediction.head[1], ref.prediction.head[3] = drops
    rsd0 = ref.state_dict()                  # (names and shapes as the reference's module tree has them)
    out = {"keys": np.array(list(rsd0.keys())), "shapes": np.array([str(tuple(v.shape)) for v in rsd0.values()])}

    pc_a = P.cloud_height(W.synth_clouds(2, 1024, seed=101)[0])
    pc_b = clouds_200(3, seed=102)
    pc_c = clouds_200(8, seed=103)
    rng = np.random.default_rng(7)
    masks = ((rng.random((8, 512)) >= 0.5).astype(np.float32) * 2.0, (rng.random((8, 256)) >= 0.5).astype(np.float32) * 2.0)
    out.update(pc_n200=pc_b, pc_train=pc_c, drop1=masks[0], drop2=masks[1])

    # train_b3: three clouds of 200 points leave 3 x 12 = 36 rows in the GroupAll stage -- a ragged last 32-row BatchNorm partial
    for tag, pc, train in (("eval_n1024", pc_a, False), ("eval_n200", pc_b, False), ("train", pc_c, True), ("train_b3", pc_b, True)):
        ref.load_state_dict(sd)
        ref.train(train)
        mk = tuple(m[:pc.shape[0]] for m in masks) if train else None
        for d, m in zip(drops, mk or (None, None)):
            d.mask = torch.from_numpy(m) if train else None
        with torch.no_grad():
            y = ref(torch.from_numpy(pc)).numpy()
        assert y.shape == (pc.shape[0], 256)
        y64, st64, idx = P.forward(sd, pc, train, mk, dtype=torch.float64)
        y32, st32, _ = P.forward(sd, pc, train, mk, dtype=torch.float32, indices=idx)
        scale = np.abs(y).max()
        err = np.abs(y - y64.numpy()).max() / scale
        rest = np.abs(y32.numpy() - y).max() / scale
        if train:
            rsd = ref.state_dict()
            for k, v in st64.items():
                r = rsd[k].numpy().copy()          # (the buffer itself is rewritten by the next case)
                out[f"stat.{tag}.{k}"] = r
                err = max(err, np.abs(r - v.numpy()).max() / np.abs(r).max())
                rest = max(rest, np.abs(st32[k].numpy() - r).max() / np.abs(r).max())
            assert int(rsd["encoder.encoder.1.0.convs.0.1.num_batches_tracked"]) == 1
        out[tag] = y
        out["ref_err_" + tag] = np.float64(err)
        print(f"{tag}: max|ref| {scale:.4g}  ref_err {err:.3g}  fp32 restatement vs reference {rest:.3g} ({rest / err:.2f} x ref_err)")
        assert rest <= 4 * err, "the fp32 restatement is not the reference"
        for name, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
            y16, _, _ = P.forward(sd, pc, train, mk, dtype=torch.float64, round_op=dt, indices=idx)
            e16 = (y16 - y64).abs().max().item() / y64.abs().max().item()
            out[f"e16_{name}_{tag}"] = np.float64(e16)
            print(f"   e16 {name}: {e16:.3g}")
        if tag == "eval_n200":
            for i, (ci, ni) in enumerate(idx):
                out[f"fps{i}"], out[f"ball{i}"] = ci.astype(np.int16), ni.astype(np.int16)
            # the boundary point: inside with <=, outside with <
            d = pc[2, 1, :3] - pc[2, 0, :3]
            assert (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] == np.float32(0.15) * np.float32(0.15) and 1 not in idx[0][1][2, 0]
            print("   balls: mean distinct", [float(np.mean([len(set(r)) for r in ni.reshape(-1, ni.shape[-1])])) for _, ni in idx])
    np.savez_compressed(os.path.join(HERE, "g_pointnext.npz"), **out)
    print("wrote g_pointnext.npz", os.path.getsize(os.path.join(HERE, "g_pointnext.npz")), "bytes")


if __name__ == "__main__":
    main()
