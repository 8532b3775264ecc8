"""Times ops.nearest_rows (csrc/nearest.hip) against the reference's own sequence, torch.cdist + argsort + slice
(interpret_prompt.py:34-37), at the real shape: Q = 32 prompt tokens, the 49408 x 512 CLIP token table, k = 10.

    python tools/nearest_time.py [--reps 200] [--out FILE.json]

Device events around `reps` back-to-back calls after a warm-up, both orders (ours first, ATen first) so that neither side always
follows the other, the median of 5 such windows.  Two table settings:
  cold   5 copies of the table (506 MB, beyond the 256 MiB Infinity Cache) visited in turn: every call reads its table from HBM;
  warm   one table (101 MB) read again and again: it stays on the die, which is what a single interpret_prompt call does NOT see.
The HBM rate is measured in the same run: a device-to-device copy of 1 GiB (2 GiB of traffic per call).  The floor of the kernel
is the table's bytes over that rate.  The ids of both sequences are compared at the end.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

Q, V, D, K = 32, 49408, 512, 10


def window_ms(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ppt_amd import ops
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time on a CPU"
    g = torch.Generator(device="cuda").manual_seed(0)
    tables = [torch.randn(V, D, device="cuda", generator=g) * 0.02 for _ in range(5)]
    q = torch.randn(Q, D, device="cuda", generator=g) * 0.02
    q[0] = tables[0][V - 1]
    ws = torch.empty(ops.nearest_rows_workspace_bytes(Q, V, D, K), dtype=torch.uint8, device="cuda")

    def ours(i, n):
        return ops.nearest_rows(q, tables[i % n], K, workspace=ws)

    def aten(i, n):
        distance = torch.cdist(q, tables[i % n])
        return torch.argsort(distance, dim=1)[:, :K], distance

    big = torch.empty(1 << 28, dtype=torch.float32, device="cuda")          # 1 GiB
    dst = torch.empty_like(big)
    big.normal_()
    for _ in range(3):
        dst.copy_(big)
    copy_ms = float(np.median([window_ms(lambda i: dst.copy_(big), 10) for _ in range(5)]))
    hbm = 2 * big.numel() * 4 / (copy_ms * 1e-3)                           # bytes / s, read + write
    del big, dst

    out = dict(shape=[Q, V, D, K], reps=a.reps, table_bytes=V * D * 4, hbm_copy_TBps=hbm / 1e12)
    floor_us = V * D * 4 / hbm * 1e6
    out["floor_us"] = floor_us
    for name, n in (("cold", 5), ("warm", 1)):
        for i in range(10):                                                 # warm-up: code objects, allocator, cdist's algorithm choice
            ours(i, n); aten(i, n)
        torch.cuda.synchronize()
        t_ours, t_aten = [], []
        for w in range(5):
            for first in ((ours, aten) if w % 2 == 0 else (aten, ours)):
                (t_ours if first is ours else t_aten).append(window_ms(lambda i: first(i, n), a.reps))
        o, t = float(np.median(t_ours)) * 1e3, float(np.median(t_aten)) * 1e3
        out[name] = dict(nearest_rows_us=o, nearest_rows_us_all=[round(x * 1e3, 2) for x in t_ours], cdist_argsort_us=t,
                         cdist_argsort_us_all=[round(x * 1e3, 2) for x in t_aten], speedup=t / o, floor_fraction=floor_us / o)
    # the two sequences name the same rows (the expanded form may swap near-ties: counted, not asserted)
    idx, dist = ours(0, 1)
    ref_idx, distance = aten(0, 1)
    out["ids_equal_share"] = float((idx.long() == ref_idx).float().mean())
    out["max_abs_dist_diff"] = float((dist - torch.gather(distance, 1, idx.long())).abs().max())
    out["query0_dist"] = [float(dist[0, 0]), float(distance[0, V - 1])]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
