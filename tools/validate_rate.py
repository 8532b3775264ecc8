#!/usr/bin/env python3
"""What the device metrics cost validate(): clouds/s of ppt_amd.evaluate.validate (C2 eval size) and validate_partseg (C5 eval
size) over a resident batch, against the same loop WITHOUT metrics -- the bare eval forward `bench.py --eval` times.

    python tools/validate_rate.py [--batches 64] [--repeats 5]                 # both loops of both configurations, interleaved
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/validate_rate.py --stage trace
    python tools/validate_rate.py --stage kernels --stats DIR/**/*_kernel_stats.csv   # the two metric kernels' rows of that trace

One process, one model per configuration; after two warm-up passes the two loops alternate `--repeats` times, each block of
`--batches` batches timed with the host clock and ending in a device synchronise (validate's ends in result(), its one copy).
The last line is one JSON object; profiles/r09_validate.md is written from it.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def setup(config):
    import torch
    import bench
    from ppt_amd import weights as W
    cfg = bench.CONFIGS[config]
    model = bench.build_model(cfg["dataset"], cfg["head_type"], model=cfg.get("model", "ULIP_PointBERT"), task=cfg.get("task", "cls"))
    model.eval()
    model.eval_inputs_ready = True                   # the batch is resident and complete (as bench.py --eval vouches)
    B, N = cfg["batch"], cfg["npoints"]
    pc = torch.from_numpy(W.synth_clouds(B, N, seed=1234)[0]).cuda()
    g = torch.Generator().manual_seed(0)
    if cfg.get("task") == "partseg":
        c2p = SHAPENETPART
        cls = (torch.arange(B) % 16).view(B, 1)
        starts = torch.tensor([v[0] for v in c2p.values()])[cls.view(-1)]
        counts = torch.tensor([len(v) for v in c2p.values()])[cls.view(-1)]
        part = starts.view(B, 1) + (torch.rand(B, N, generator=g) * counts.view(B, 1)).long()
        batch = (pc, cls.cuda(), part.cuda())
    else:
        batch = (pc, torch.randint(0, len(model.prompt_learner.name_lengths), (B,), generator=g).cuda())
    args = argparse.Namespace(gpu=torch.cuda.current_device(), classnames=None,
                              category2part=SHAPENETPART if cfg.get("task") == "partseg" else None)
    return cfg, model, batch, args


SHAPENETPART = {'Airplane': [0, 1, 2, 3], 'Bag': [4, 5], 'Cap': [6, 7], 'Car': [8, 9, 10, 11], 'Chair': [12, 13, 14, 15],
                'Earphone': [16, 17, 18], 'Guitar': [19, 20, 21], 'Knife': [22, 23], 'Lamp': [24, 25, 26, 27], 'Laptop': [28, 29],
                'Motorbike': [30, 31, 32, 33, 34, 35], 'Mug': [36, 37], 'Pistol': [38, 39, 40], 'Rocket': [41, 42, 43],
                'Skateboard': [44, 45, 46], 'Table': [47, 48, 49]}


def loops(config, batches):
    """-> (bare, with_metrics): two callables that run `batches` batches and return seconds"""
    import contextlib
    import io
    import torch
    from ppt_amd import evaluate
    cfg, model, batch, args = setup(config)
    partseg = cfg.get("task") == "partseg"
    loader = [batch] * batches
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.3)
    onehot = evaluate.to_categorical(batch[1], 16) if partseg else None

    def bare():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for b in loader:
                logits = model(b[0], onehot) if partseg else model(b[0])
        torch.cuda.synchronize()
        assert logits is not None
        return time.perf_counter() - t0

    def with_metrics():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            out = (evaluate.validate_partseg if partseg else evaluate.validate)(loader, model, crit, args)
        torch.cuda.synchronize()
        assert out["n"] == batches * cfg["batch"] and out["nonfinite_rows"] == 0, out
        return time.perf_counter() - t0
    return cfg, bare, with_metrics


def stage_loops(a):
    import torch
    torch.cuda.set_device(0)
    from ppt_amd import graphs
    graphs.shared_text_stream()
    graphs.shared_group_stream()
    out = {}
    for config in a.configs:
        cfg, bare, with_metrics = loops(config, a.batches)
        for _ in range(2):
            bare(), with_metrics()
        tb, tm = [], []
        for _ in range(a.repeats):
            tb.append(bare())
            tm.append(with_metrics())
        n = a.batches * cfg["batch"]
        rb, rm = [n / t for t in tb], [n / t for t in tm]
        mb, mm = statistics.median(rb), statistics.median(rm)
        out[config] = {"clouds_per_s_forward_only": [round(v) for v in rb], "clouds_per_s_validate": [round(v) for v in rm],
                       "median_forward_only": round(mb), "median_validate": round(mm),
                       "spread_forward_only_pct": round(100 * (max(rb) - min(rb)) / mb, 2),
                       "overhead_pct": round(100 * (mb / mm - 1), 2), "batch": cfg["batch"], "npoints": cfg["npoints"],
                       "batches": a.batches}
        print(config, out[config], flush=True)
    print(json.dumps(out), flush=True)


def stage_trace(a):
    import torch
    torch.cuda.set_device(0)
    from ppt_amd import graphs
    graphs.shared_text_stream()
    graphs.shared_group_stream()
    for config in a.configs:
        _, _, with_metrics = loops(config, a.batches)
        for _ in range(3):
            with_metrics()


def stage_kernels(a):
    rows = []
    for path in a.stats:
        with open(path) as fh:
            rows += [r for r in csv.DictReader(fh) if "metrics_kernel" in r.get("Name", "")]
    out = {r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                     "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)} for r in rows}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", default="loops", choices=["loops", "trace", "kernels"])
    ap.add_argument("--configs", nargs="+", default=["C2", "C5"])
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stats", nargs="*", default=[])
    a = ap.parse_args()
    {"loops": stage_loops, "trace": stage_trace, "kernels": stage_kernels}[a.stage](a)
