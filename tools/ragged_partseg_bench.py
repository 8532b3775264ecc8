"""Dev tool: what ragged part segmentation costs and whether it moved the uniform path (profiles/r27_ragged_partseg.md).

    bash tools/build_variant.sh parent            # at the commit to compare with -> tools/_build/libppt_parent.so
    python tools/ragged_partseg_bench.py kernels --base tools/_build/libppt_parent.so     # uniform launches, two builds in ONE process
    python tools/ragged_partseg_bench.py steps                                            # C5 train step + validate_partseg 16 x 2048
    python tools/ragged_partseg_bench.py whole                                            # whole-shape validation against resampled-2048

`kernels` alternates the two libraries window by window as tools/index_bench.py does (uniform entry points only, called through
ctypes, so a base build without the packed symbols loads): knn_group k = 3 with 512 sources and 2048 queries, three_nn_interp_fwd,
scatter_rows_bwd and partseg_metrics at 16 x 2048.  `steps` uses nothing a parent checkout lacks: run it in a checkout of each commit,
alternating, and compare the medians with the parent's own spread.  `whole` needs this commit: a set of shapes with 2 .. 3 k
points each through validate_partseg as ragged whole-shape batches and as resampled 2048-point batches, with the share of device
time in the packed-row kernels (ops.KernelProfiler)."""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from ppt_amd import weights as W
from ppt_amd._lib import _SIGNATURES
from ppt_amd.ops import PPT_F16 as F16

c_void_p = ctypes.c_void_p


def p(t):
    return None if t is None else c_void_p(t.data_ptr())


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def window(fn, launches):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(launches):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / launches


UNIFORM = ("ppt_knn_group_f32", "ppt_three_nn_interp_fwd", "ppt_scatter_rows_bwd", "ppt_partseg_metrics")


def load(path):
    L = ctypes.CDLL(os.path.abspath(path))
    for name in UNIFORM:
        getattr(L, name).restype, getattr(L, name).argtypes = _SIGNATURES[name]
    return L


def kernels(a):
    libs = {"base": load(a.base), "new": load(a.new)}
    B, N, S, D2, P = 16, 2048, 512, 384, 50
    pc, _ = W.synth_clouds(B, N, seed=3)
    pc = torch.from_numpy(pc).cuda()
    src = pc[:, :S].contiguous()
    g = torch.Generator(device="cuda").manual_seed(1)
    idx = torch.empty((B, N, 3), dtype=torch.int64, device="cuda")
    dist = torch.empty((B, N, 3), dtype=torch.float32, device="cuda")
    p1 = torch.randn(B, N, 19, device="cuda", generator=g)
    p2 = torch.randn(B, S, D2, device="cuda", generator=g)
    ld = 408
    rows = torch.empty((B * N, ld), dtype=torch.float16, device="cuda")
    wgt = torch.empty((B, N, 3), dtype=torch.float32, device="cuda")
    d_rows = torch.randn(B * N, ld, device="cuda", generator=g)
    d_src = torch.empty((B, S, D2), dtype=torch.float32, device="cuda")
    logits = torch.randn(B, N, P, device="cuda", generator=g)
    labels = torch.randint(0, 4, (B, N), device="cuda", generator=g)
    start = torch.zeros(P, dtype=torch.int32, device="cuda")
    count = torch.full((P,), 4, dtype=torch.int32, device="cuda")
    rec = torch.empty((B, 32), dtype=torch.int32, device="cuda")
    partial = torch.empty(B * 8, dtype=torch.float32, device="cuda")
    cases = {
        "knn_group k=3 512 src 2048 q": lambda L: L.ppt_knn_group_f32(p(src), p(pc), B, S, N, 3, p(idx), None, p(dist), stream()),
        "three_nn_interp_fwd f16": lambda L: L.ppt_three_nn_interp_fwd(p(p1), 19, p(p2), D2, p(idx), p(dist), B, N, S, p(rows), F16, ld, p(wgt), stream()),
        "scatter_rows_bwd": lambda L: L.ppt_scatter_rows_bwd(p(idx), p(wgt), p(d_rows), ld, 19, B, 3 * N, 3, S, D2, p(d_src), stream()),
        "partseg_metrics": lambda L: L.ppt_partseg_metrics(p(logits), p(labels), 0.2, B, N, P, p(start), p(count), 4, p(rec), p(partial), stream()),
    }
    out = []
    for name, fn in cases.items():
        for L in libs.values():
            assert fn(L) == 0, name
            window(lambda: fn(L), 5)
        med = {"base": [], "new": []}
        for _ in range(a.rounds):
            for k, L in libs.items():
                med[k].append(float(np.median([window(lambda: fn(L), a.launches) for _ in range(a.windows)])))
        row = dict(kernel=name, base_us=[round(x, 2) for x in med["base"]], new_us=[round(x, 2) for x in med["new"]],
                   base_median=round(float(np.median(med["base"])), 2), new_median=round(float(np.median(med["new"])), 2),
                   base_min=round(min(med["base"]), 2), base_max=round(max(med["base"]), 2))
        row["new_within_base_spread"] = bool(row["new_median"] <= row["base_max"])
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def _partseg_model():
    from ppt_amd.models import ULIP_models as M
    args = SimpleNamespace(classnames=M.dataset_classnames("shapenetpart"), template_init='', class_name_position='middle',
                           num_learnable_prompt_tokens=32, gpu=0, task='partseg', head_type=0, evaluate_3d=False, ulip2=False,
                           synthetic_weights=True)
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.ULIP_PointBERT_partseg(args)
    m.load_state_dict(W.ulip_partseg_state_dict(seed=0), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding(50, seed=0)
    return m.cuda()


def _category2part():
    from ppt_amd.partseg import shapenetpart_category2part
    return shapenetpart_category2part()


def steps(a):
    """C5 train step (Trainer.step, 16 x 2048) and validate_partseg over 4 batches of 16 x 2048: ms, median of `rounds` windows"""
    from ppt_amd import evaluate
    from ppt_amd.train import Trainer
    m = _partseg_model()
    c2p = _category2part()
    B, N = 16, 2048
    pc = torch.from_numpy(W.synth_clouds(B, N, seed=55)[0]).cuda()
    g = torch.Generator().manual_seed(5)
    cls = torch.randint(0, 16, (B, 1), generator=g)
    cats = list(c2p.values())
    part = torch.stack([torch.tensor(cats[int(c)])[torch.randint(0, len(cats[int(c)]), (N,), generator=g)] for c in cls[:, 0]]).cuda()
    onehot = evaluate.to_categorical(cls.cuda()[:, 0], 16)
    m.train()
    tr = Trainer(m, lr=1e-3, label_smoothing=0.2, distributed=False)
    tr.extra_inputs = (onehot,)
    for _ in range(12):
        tr.step(pc, part)
    tr.finish()
    torch.cuda.synchronize()
    train_ms = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.launches):
            tr.step(pc, part)
        tr.finish()
        torch.cuda.synchronize()
        train_ms.append((time.perf_counter() - t0) * 1e3 / a.launches)
    loader = type("L", (list,), {})([(pc, cls.cuda(), part)] * 4)
    loader.dataset = SimpleNamespace(category2part=c2p)
    args = SimpleNamespace(gpu=0)
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.2)
    val_ms = []
    for i in range(a.rounds + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            evaluate.validate_partseg(loader, m, crit, args)
        torch.cuda.synchronize()
        if i >= 2:
            val_ms.append((time.perf_counter() - t0) * 1e3)
    row = dict(train_step_ms=[round(x, 3) for x in train_ms], train_step_median=round(float(np.median(train_ms)), 3),
               validate_4x16x2048_ms=[round(x, 2) for x in val_ms], validate_median=round(float(np.median(val_ms)), 2))
    print(json.dumps(row), flush=True)
    return row


def whole(a):
    """validate_partseg over `shapes` shapes of 2 .. 3 k points: ragged whole-shape batches against resampled-2048 batches"""
    from ppt_amd import evaluate, ops
    from ppt_amd.data import DeviceBatchLoader, DeviceCloudSet
    m = _partseg_model()
    c2p = _category2part()
    cats = list(c2p.values())
    rng = np.random.default_rng(11)
    lens = rng.integers(2000, 3001, a.shapes)
    cls = rng.integers(0, 16, a.shapes)
    clouds = [W.synth_clouds(1, int(n), seed=100 + i)[0][0] for i, n in enumerate(lens)]
    seg = [np.asarray(cats[c])[rng.integers(0, len(cats[c]), n)].astype(np.int32) for c, n in zip(cls, lens)]
    cset = DeviceCloudSet(clouds, cls, seg=seg)
    args = SimpleNamespace(gpu=0, category2part=c2p)
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.2)
    res = {"shapes": int(a.shapes), "points": int(lens.sum()), "Nmax": int(lens.max())}
    for name, kw in (("whole_shapes", dict(ragged=True)), ("resampled_2048", dict())):
        loader = DeviceBatchLoader(cset, 16, 2048, "shapenetpart", False, shuffle=False, **kw)
        times = []
        for i in range(a.rounds + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                out = evaluate.validate_partseg(loader, m, crit, args)
            torch.cuda.synchronize()
            if i >= 2:
                times.append(time.perf_counter() - t0)
        t = float(np.median(times))
        pts = int(lens.sum()) if kw else a.shapes * 2048
        res[name] = dict(seconds=[round(x, 4) for x in times], median_s=round(t, 4), clouds_per_s=round(a.shapes / t, 1),
                         points_per_s=round(pts / t), acc=out["acc"], mean_inst_iou=out["mean_inst_iou"])
    # share of device time in the packed-row kernels, one profiled pass
    ops.profiler = ops.KernelProfiler()
    loader = DeviceBatchLoader(cset, 16, 2048, "shapenetpart", False, shuffle=False, ragged=True)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    with contextlib.redirect_stdout(io.StringIO()):
        evaluate.validate_partseg(loader, m, crit, args)
    e.record()
    torch.cuda.synchronize()
    summ = ops.profiler.summary()
    ops.profiler = None
    res["profiled_pass_ms"] = round(s.elapsed_time(e), 2)
    res["profiled_families_ms"] = {k: round(v["ms"], 3) for k, v in sorted(summ.items(), key=lambda kv: -kv[1]["ms"])[:12]}
    new = ("knn_group_packed", "three_nn_interp_packed", "pack_rows", "unpack_rows", "partseg_metrics_ragged")
    res["new_kernels_ms"] = {k: round(summ[k]["ms"], 3) for k in new if k in summ}
    res["new_kernels_share"] = round(sum(res["new_kernels_ms"].values()) / res["profiled_pass_ms"], 4)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "steps", "whole"))
    ap.add_argument("--base")
    ap.add_argument("--new", default=os.path.join(ROOT, "ppt_amd", "csrc", "libppt_hip.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--shapes", type=int, default=64)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mode == "kernels" and not a.base:
        ap.error("kernels needs --base")
    result = {"kernels": kernels, "steps": steps, "whole": whole}[a.mode](a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
