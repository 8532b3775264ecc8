"""Time the t-SNE kernels (csrc/tsne.hip) and the whole ppt_amd.tsne.tsne() run on the device, against their floors.

    python tools/tsne_time.py [--cases 2468x40,2882x15,11400x512] [--out FILE.json]

Per case (synthetic blobs, as many classes as a logit row has columns, at most 40): the affinities call, microseconds per
iteration of the descent (device events around one ppt_tsne_steps call of 250 iterations, with and without the check every 50)
in the exaggerated stage from the random start and in the late stage on the finished embedding, and the whole default run
(host clock around tsne(), which ends in a device synchronise) -- each the median of three after a warm-up.  The floors are
computed from the shape:
  P bytes      N^2 * 4 per iteration over the rate of the level P sits in (the L2s while an eighth of P fits one of them, the
               Infinity Cache up to 256 MiB, HBM beyond);
  pair rate    N^2 pairs over the vector rate of the pair loop as compiled: 94 single-issue VALU instructions (2 cycles per
               wave-instruction and SIMD) and 4 v_rcp_f32 (4) for 4 x 64 pairs, 1024 SIMDs at 2.4 GHz;
  launches     2 per iteration times the 1.45 us dependent-launch boundary.
One JSON line per case; needs a GPU (there is no CPU path)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ppt_amd import ops, tsne as T  # noqa: E402

L2_BYTES, L2_RATE, MALL_BYTES, MALL_RATE, HBM_RATE = 4 << 20, 34.5e12, 256 << 20, 8.6e12, 6.3e12
PAIR_CYCLES_PER_256 = 94 * 2 + 4 * 4
LAUNCH_GAP_US = 1.45


def blobs(n, d, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    k = min(d, 40)
    centres = torch.randn(k, d, generator=g) * 4.0
    labels = torch.arange(n) % k
    return (centres[labels] + torch.randn(n, d, generator=g)).cuda(), labels


def timed(fn, repeats=3):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), out


def floors(n):
    p_bytes = n * n * 4
    level, rate = ("L2", L2_RATE) if p_bytes / 8 <= L2_BYTES else ("Infinity Cache", MALL_RATE) if p_bytes <= MALL_BYTES else ("HBM", HBM_RATE)
    return {"p_bytes": p_bytes, "p_level": level, "p_us": p_bytes / rate * 1e6,
            "pair_us": n * n / 256.0 * PAIR_CYCLES_PER_256 / (1024 * 2.4e9) * 1e6, "launch_us": 2 * LAUNCH_GAP_US, "launches_per_iteration": 2}


def run_case(n, d):
    x, _ = blobs(n, d)
    perplexity, lr, span = 30.0, T.auto_learning_rate(n, 12.0), 250
    aff_ms, aff_all = timed(lambda: ops.tsne_affinities(x, perplexity))
    P, _, pstats = ops.tsne_affinities(x, perplexity)
    ws = torch.empty(ops.tsne_steps_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    stats = torch.zeros((span // 50 + 1, 2), dtype=torch.float32, device="cuda")
    Y_end, info = T.tsne(x, perplexity=perplexity)
    res = {"n": n, "d": d, "affinities_ms": aff_ms, "affinities_ms_all": aff_all, "floors": floors(n), "kl": info["kl_divergence"]}
    for stage, y0, t0 in (("exaggerated", torch.from_numpy(T.random_init(n, 0)).cuda(), 0), ("late", Y_end, 750)):
        for every in (0, 50):
            def steps():
                y = y0.clone()
                ops.tsne_steps(P, pstats, y, torch.zeros_like(y), torch.ones_like(y), t0, span, lr=lr, check_every=every, stats=stats,
                               workspace=ws)
            ms, _ = timed(steps)
            res[f"us_per_iteration_{stage}_check{every}"] = ms * 1e3 / span
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        T.tsne(x, perplexity=perplexity)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t) * 1e3)
    res["default_run_ms"], res["default_run_ms_all"] = statistics.median(walls), walls
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2468x40,2882x15,11400x512")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tsne_time: needs a GPU (a timing taken elsewhere says nothing about the device)")
    lines = []
    for case in a.cases.split(","):
        n, d = (int(v) for v in case.split("x"))
        lines.append(json.dumps(run_case(n, d)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
