"""Times the two kernels behind ppt_amd/viz.py (csrc/render.hip) at the shapes of a validation-batch sheet:

    ops.render_balls     32 clouds x 3 views = 96 geometries, K = 3 colourings, 800 x 800 pictures, n = 2048 points, radius 13
    ops.partseg_predict  logits 32 x 2048 x 50

    python tools/viz_time.py [--reps 20] [--out FILE.json]

Device events around `reps` back-to-back calls after a warm-up, the median of 5 such windows.  The clouds are seeded points in
the unit ball through viz.camera, i.e. pictures as dense as a real sheet's.  Beside each time: the bytes the call must write
(3 G K H W for the pictures, 4 B N for the predictions) and must read, and the rate they amount to; the HBM rate of the same run
(a device-to-device copy of 1 GiB) gives the bytes-based floor.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, V, K, SIZE, N, RADIUS, P = 32, 3, 3, 800, 2048, 13, 50


def window_ms(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ppt_amd import evaluate, ops, viz
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time on a CPU"
    g = torch.Generator(device="cuda").manual_seed(0)
    xyz = torch.randn(B, N, 3, device="cuda", generator=g)
    xyz = xyz / xyz.norm(dim=-1, keepdim=True) * torch.rand(B, N, 1, device="cuda", generator=g) ** (1 / 3)
    ixyz = viz.camera(xyz, viz.views_from_mouse(viz.DEFAULT_VIEWS_MOUSE), SIZE).reshape(B * V, N, 3).contiguous()
    colors = torch.rand(B * V, K, N, 3, device="cuda", generator=g) * 255
    G = B * V
    out = torch.empty((G, K, SIZE, SIZE, 3), dtype=torch.uint8, device="cuda")
    ws = torch.empty(ops.render_balls_workspace_bytes(G, N, SIZE, SIZE, RADIUS), dtype=torch.uint8, device="cuda")
    logits = torch.randn(B, N, P, device="cuda", generator=g)
    anchor = torch.randint(0, P, (B,), device="cuda", generator=g)
    c2p = {"c%d" % i: list(range(5 * i, 5 * i + 5)) for i in range(10)}
    start, count = (torch.from_numpy(t).cuda() for t in evaluate.part_tables(c2p))
    pred = torch.empty((B, N), dtype=torch.int32, device="cuda")

    def render():
        ops.render_balls(ixyz, colors, SIZE, SIZE, RADIUS, out=out, workspace=ws)

    def predict():
        ops.partseg_predict(logits, anchor, start, count, pred=pred)

    big = torch.empty(1 << 28, dtype=torch.float32, device="cuda")          # 1 GiB
    dst = torch.empty_like(big)
    big.normal_()
    for _ in range(3):
        dst.copy_(big)
    copy_ms = float(np.median([window_ms(lambda: dst.copy_(big), 10) for _ in range(5)]))
    hbm = 2 * big.numel() * 4 / (copy_ms * 1e-3)                           # bytes / s, read + write
    del big, dst

    res = dict(hbm_copy_TBps=hbm / 1e12, reps=a.reps)
    for name, fn, wr, rd in (("render_balls", render, 3 * G * K * SIZE * SIZE, G * N * 12 + G * K * N * 12),
                             ("partseg_predict", predict, 4 * B * N, 4 * B * N * P)):
        for _ in range(5):                                                  # warm-up: code objects, the pattern table's upload
            fn()
        torch.cuda.synchronize()
        t = [window_ms(fn, a.reps) for _ in range(5)]
        us = float(np.median(t)) * 1e3
        res[name] = dict(us=us, us_all=[round(x * 1e3, 2) for x in t], bytes_written=wr, bytes_read=rd,
                         written_GBps=wr / us / 1e3, floor_us=(wr + rd) / hbm * 1e6, floor_fraction=(wr + rd) / hbm * 1e6 / us)
    res["render_balls"]["shape"] = dict(G=G, K=K, H=SIZE, W=SIZE, n=N, radius=RADIUS)
    res["render_balls"]["covered_share"] = float((out[:, 0] != 255).any(-1).float().mean())
    res["partseg_predict"]["shape"] = [B, N, P]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
