"""Time the mini-PointNet kernels at C2's size (524 288 points = 16 384 groups), alone on the chip, and digest their outputs:
  conv12:   ppt_mini_pointnet_conv12 (csrc/mpn1.hip)
  conv3:    ppt_mini_pointnet_conv3, y3 written, with and without the BatchNorm partials (csrc/mpn3.hip)
  stats:    ppt_mini_pointnet_conv3 with store = False (the training step's statistics pass)
  conv4:    ppt_mini_pointnet_conv4 (csrc/mpn4.hip), y3 read back
  unfused:  conv3 + conv4
  fused:    ppt_mini_pointnet_conv34 (csrc/mpn34.hip)
Usage: python tools/mpn34_bench.py [groups] [reps] [--dtype float16|bfloat16] [--rounds R]
Each figure is the median (minimum in brackets) over R rounds of HIP events around `reps` back-to-back launches.  The sha256 lines
digest every output of an op on seeded inputs: two builds of the library (PPT_HIP_LIB selects one) compute the same bits exactly
when the lines are equal."""
import argparse
import hashlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppt_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("groups", nargs="?", type=int, default=16384)
ap.add_argument("reps", nargs="?", type=int, default=20)
ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16"])
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
tiles, reps, T = a.groups, a.reps, getattr(torch, a.dtype)
M = 32 * tiles
g = torch.Generator().manual_seed(0)
y2 = torch.randn(M, 256, generator=g).cuda().to(T)
w3b = (torch.randn(512, 256, generator=g) * 0.06).cuda().to(T)
w4 = (torch.randn(256, 512, generator=g) * 0.04).cuda().to(T)
gterm = torch.randn(tiles, 512, generator=g).cuda()
sc, sh = (0.5 + torch.rand(512, generator=g)).cuda(), (0.1 * torch.randn(512, generator=g)).cuda()
b4 = torch.zeros(256).cuda()
pts = (torch.randn(M, 3, generator=g) * 0.3).cuda()
w1, b1 = torch.randn(128, 3, generator=g).cuda(), (0.1 * torch.randn(128, generator=g)).cuda()
sc1, sh1 = (1.0 + 0.1 * torch.randn(128, generator=g)).cuda(), (0.1 * torch.randn(128, generator=g)).cuda()
w2 = (torch.randn(256, 128, generator=g) / 128 ** 0.5).cuda().to(T)
b2 = (0.1 * torch.randn(256, generator=g)).cuda()
w4t = ops.mpn34_retile(w4)
st = (torch.empty(tiles, 512, device="cuda"), torch.empty(tiles, 512, device="cuda"))
y3 = ops.mini_pointnet_conv3(y2, w3b, gterm)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(us), min(us)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def conv3_stats_out():
    st[0].zero_(), st[1].zero_()
    y = ops.mini_pointnet_conv3(y2, w3b, gterm, st)
    return (y, st[0], st[1])


def stats_only_out():
    st[0].zero_(), st[1].zero_()
    ops.mini_pointnet_conv3(y2, w3b, gterm, st, store=False)
    return (st[0], st[1])


OPS = {
    "conv12": lambda: ops.mini_pointnet_conv12(pts, w1, b1, sc1, sh1, w2, b2),
    "conv3": lambda: ops.mini_pointnet_conv3(y2, w3b, gterm, st),
    "conv3_eval": lambda: ops.mini_pointnet_conv3(y2, w3b, gterm),
    "stats": lambda: ops.mini_pointnet_conv3(y2, w3b, gterm, st, store=False),
    "conv4": lambda: ops.mini_pointnet_conv4(y3, sc, sh, w4, b4),
    "unfused": lambda: ops.mini_pointnet_conv4(ops.mini_pointnet_conv3(y2, w3b, gterm, st), sc, sh, w4, b4),
    "fused": lambda: ops.mini_pointnet_conv34(y2, w3b, gterm, w4t, b4),
}
DIGESTS = {"conv12": lambda: OPS["conv12"](), "conv3": conv3_stats_out, "conv3_eval": lambda: (OPS["conv3_eval"](),),
           "stats": stats_only_out, "conv4": lambda: (OPS["conv4"](),), "fused": lambda: (OPS["fused"](),)}

lib = os.environ.get("PPT_HIP_LIB") or "(this tree's)"
print(f"library {lib} | {a.dtype} | groups {tiles} | {reps} launches x {a.rounds} rounds")
for name, fn in DIGESTS.items():
    print(f"sha256 {name:<10} {digest(*fn())}")
t = {name: timed(fn) for name, fn in OPS.items()}
for name, (med, lo) in t.items():
    print(f"us {name:<10} {med:8.1f} ({lo:.1f})")
t_u, t_3, t_s, t_f = t["unfused"][0], t["conv3"][0], t["stats"][0], t["fused"][0]
fl = 2.0 * M * 512 * 272 + 2.0 * M * 256 * 512
print(f"groups {tiles}: unfused conv3 + conv4 {t_u:.1f} us (conv3 alone {t_3:.1f}) | statistics pass {t_s:.1f} us | fused {t_f:.1f} us "
      f"= {fl / t_f * 1e-6:.0f} TFLOP/s executed | train: stats + fused {t_s + t_f:.1f} vs {t_u:.1f} us; eval: fused {t_f:.1f} vs {t_u:.1f} us")
