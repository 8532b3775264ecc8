#!/usr/bin/env python3
"""What feeding costs: the device-resident loader (ppt_amd.data.DeviceBatchLoader) alone, and a C2 Trainer.step loop under three
feeds.  The table of profiles/r08_datapipe.md comes from this tool.

    python tools/datapipe_bench.py                     # both stages, each as a child process under its own time limit
    python tools/datapipe_bench.py --stage loader      # (a) loader alone: clouds/s and host ms per batch, both draw modes, per recipe
    python tools/datapipe_bench.py --stage loader --recipes modelnet,shapenet55 --draws device --window 0.5
    python tools/datapipe_bench.py --stage loader --recipes modelnet --augment rotate,jitter --draws device --window 0.5
                                                       # the augmentations (profiles/r22_augment.md): timed windows of >= 0.5 s
    python tools/datapipe_bench.py --stage steps       # (b) the step loop under resident / worker / device-loader feeding
    python tools/datapipe_bench.py --stage trace       # a short device-loader step loop, to run under rocprofv3 --kernel-trace --stats

(a) B = 32, 8192 -> 1024 (ScanObjectNN: the first 1024 of 2048 rows; ShapeNetPart: choice of 2048 from ragged clouds of up to 2900
rows; ShapeNet-55: ModelNet's clouds through recipe "shapenet55", i.e. FPS + ShapeNet's five augmentations).  --augment adds the named
stages (DeviceBatchLoader(augment=...)) to every recipe measured.  --window S: a timed repeat runs whole epochs until S seconds have
passed (default: one epoch per repeat).  Clock: host clock around whole epochs, ending in a device synchronise.  "host ms" is the time the launching thread spends
inside next() per batch -- the draws (numpy mode), the launches, the event.
(b) the three feeds ALTERNATE inside one process, after a warm-up of every feed; each timed block ends in a device synchronise:
    resident  the same resident batch every step, vouched ready (Trainer.inputs_ready): no feeding at all -- the yardstick
    workers   DataLoader(num_workers=8, pin_memory) over a Dataset that does the reference's ModelNet __getitem__ with
              ppt_amd.data.farthest_point_sample (start_fps_service) + DevicePrefetcher
    device    DeviceBatchLoader(draws="device") over the same clouds
Prints one line per measurement and a JSON summary line at the end of each stage.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, NPOINTS, ROWS = 32, 1024, 8192
STAGE_LIMIT_S = {"loader": 240, "steps": 420}


def synth_set(m, rows, seed=3):
    import numpy as np
    pc = np.random.default_rng(seed).random((m, rows, 3), dtype=np.float32) * 2 - 1
    return pc, (np.arange(m) % 40).astype(np.int64)


def stage_loader(a):
    import numpy as np
    import torch
    from ppt_amd.data import DeviceBatchLoader, DeviceCloudSet
    m = 32 * a.batches
    pc, lab = synth_set(m, ROWS)
    r = np.random.default_rng(0)
    lens = r.integers(2100, 2900, size=m)
    make = {"modelnet": lambda: (DeviceCloudSet(pc, lab), NPOINTS),
            "scanobjectnn": lambda: (DeviceCloudSet(pc[:, :2048].copy(), lab), NPOINTS),
            "shapenetpart": lambda: (DeviceCloudSet([pc[i, :L] for i, L in enumerate(lens)], lab % 16,
                                                    seg=[r.integers(0, 50, L).astype(np.int32) for L in lens]), 2048),
            "shapenet55": lambda: (DeviceCloudSet(pc, lab), NPOINTS)}
    recipes = list(make) if a.recipes == "all" else a.recipes.split(",")
    extra = {"augment": tuple(a.augment.split(","))} if a.augment else {}     # (no keyword at all without --augment)
    res = []
    for recipe in recipes:
        s, n = make[recipe]()
        for draws in (("device", "numpy") if a.draws == "both" else (a.draws,)):
            ld = DeviceBatchLoader(s, B, n, recipe, True, seed=1, draws=draws, **extra)
            for _ in ld:                                      # warm-up: code objects, allocator, pinned pool
                pass
            rates, host_ms = [], []
            batch_ms, epoch = [], 0
            for rep in range(a.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                spent, nb = 0.0, 0
                while True:                                   # whole epochs, each ending in a device synchronise
                    epoch += 1
                    ld.set_epoch(epoch)
                    it = iter(ld)
                    while True:
                        h0 = time.perf_counter()
                        batch = next(it, None)
                        spent += time.perf_counter() - h0
                        if batch is None:
                            break
                        nb += 1
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if dt >= a.window:
                        break
                rates.append(nb * B / dt)
                host_ms.append(1e3 * spent / nb)
                batch_ms.append(1e3 * dt / nb)
            row = dict(recipe=recipe, draws=draws, npoints=n, augment=list(extra.get("augment", ())), window_s=a.window,
                       clouds_per_s=[round(x) for x in rates], ms_per_batch=[round(x, 4) for x in batch_ms],
                       host_ms_per_batch=[round(x, 3) for x in host_ms])
            print(f"loader-alone {recipe:13s} draws={draws:6s} n={n} augment={a.augment or '-'}: clouds/s {row['clouds_per_s']}  "
                  f"ms/batch {row['ms_per_batch']}  host ms/batch {row['host_ms_per_batch']}", flush=True)
            res.append(row)
    print("DATAPIPE_LOADER " + json.dumps(res), flush=True)


def build_trainer():
    import bench
    import torch
    from ppt_amd.train import Trainer
    cfg = bench.CONFIGS["C2"]
    model = bench.build_model(cfg["dataset"], cfg["head_type"])
    model.train()
    tr = Trainer(model, lr=3e-3, label_smoothing=0.2, distributed=False)
    tr.group_ahead_when_frozen = True
    torch.cuda.synchronize()
    return tr


class WorkerSet:
    """The reference's ModelNet item (data/dataset_3d.py:291-315) on ppt_amd.data.farthest_point_sample: what a DataLoader worker
    does per sample today."""

    def __init__(self, pc, lab):
        self.pc, self.lab = pc, lab

    def __len__(self):
        return len(self.lab)

    def __getitem__(self, i):
        import numpy as np
        from ppt_amd import data as PD
        p = PD.farthest_point_sample(self.pc[i], NPOINTS)[:, 0:3]
        p = PD.pc_normalize(p)
        s, t = np.random.uniform(2. / 3., 3. / 2., 3), np.random.uniform(-0.2, 0.2, 3)
        p = np.add(np.multiply(p, s), t).astype("float32")
        np.random.shuffle(p)
        return p, int(self.lab[i])


def stage_steps(a, trace=False):
    import numpy as np
    import torch
    from ppt_amd import data as PD
    m = 32 * a.batches
    pc, lab = synth_set(m, ROWS)
    tr = build_trainer()
    dset = PD.DeviceCloudSet(pc, lab)
    dev_loader = PD.DeviceBatchLoader(dset, B, NPOINTS, "modelnet", True, seed=1, draws="device")
    first = next(iter(PD.DeviceBatchLoader(dset, B, NPOINTS, "modelnet", True, seed=1, draws="device")))
    torch.cuda.synchronize()
    res_pc, res_lab = first[0].clone(), first[1].clone()     # plain resident tensors (no event attached)
    epoch = [0]

    def run_resident():
        tr.inputs_ready = True
        for _ in range(a.batches):
            tr.step(res_pc, res_lab)
        return a.batches, 0.0

    def fed(it):
        tr.inputs_ready = False
        spent, nb = 0.0, 0
        while True:
            h0 = time.perf_counter()
            batch = next(it, None)
            spent += time.perf_counter() - h0
            if batch is None:
                return nb, spent
            tr.step(batch[0], batch[1])
            nb += 1

    def run_device():
        epoch[0] += 1
        dev_loader.set_epoch(epoch[0])
        return fed(iter(dev_loader))
    feeds = {"resident": run_resident, "device": run_device}
    if not trace:
        PD.start_fps_service()
        wl = torch.utils.data.DataLoader(WorkerSet(pc, lab), batch_size=B, shuffle=True, num_workers=8, pin_memory=True,
                                         persistent_workers=True, timeout=300)
        feeds = {"resident": run_resident, "workers": lambda: fed(iter(PD.DevicePrefetcher(wl))), "device": run_device}
    for name, fn in feeds.items():                            # warm-up: graphs captured, workers forked, caches filled
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        print(f"warm-up {name} done", flush=True)
    out = {k: dict(ms_per_step=[], clouds_per_s=[], host_ms_per_batch=[]) for k in feeds}
    for rep in range(1 if trace else a.repeats):
        for name, fn in feeds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nb, spent = 0, 0.0
            for _ in range(a.epochs if name != "workers" else 1):
                k, s = fn()
                nb, spent = nb + k, spent + s
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            o = out[name]
            o["ms_per_step"].append(round(1e3 * dt / nb, 4)); o["clouds_per_s"].append(round(nb * B / dt))
            o["host_ms_per_batch"].append(round(1e3 * spent / nb, 4))
            print(f"rep {rep} {name:9s}: {nb} steps, {1e3 * dt / nb:.4f} ms/step, {nb * B / dt:.0f} clouds/s, "
                  f"loader host ms/batch {1e3 * spent / nb:.4f}", flush=True)
    tr.finish()
    torch.cuda.synchronize()
    if not trace:
        del wl
        PD.stop_fps_service()
    base = out["resident"]["ms_per_step"]
    summary = {k: dict(v, median_ms=float(np.median(v["ms_per_step"])), spread_pct=round(100 * (max(v["ms_per_step"]) - min(v["ms_per_step"]))
                                                                                       / float(np.median(v["ms_per_step"])), 2))
               for k, v in out.items()}
    for k, v in summary.items():
        v["vs_resident_pct"] = round(100 * (v["median_ms"] / float(np.median(base)) - 1), 2)
    print("DATAPIPE_STEPS " + json.dumps(summary), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", default="all", choices=["all", "loader", "steps", "trace"])
    ap.add_argument("--batches", type=int, default=32, help="batches of 32 clouds in the synthetic set (one epoch)")
    ap.add_argument("--epochs", type=int, default=4, help="epochs per timed block of the resident / device feeds")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--recipes", default="all", help="loader stage: comma-separated recipes (default: every recipe)")
    ap.add_argument("--draws", default="both", choices=["both", "device", "numpy"], help="loader stage: the draw modes to time")
    ap.add_argument("--augment", default="", help="loader stage: comma-separated augmentation stages added to each recipe, e.g. rotate,jitter")
    ap.add_argument("--window", type=float, default=0.0, help="loader stage: seconds a timed repeat lasts at least (whole epochs)")
    a = ap.parse_args()
    if a.stage == "all":
        for st in ("loader", "steps"):                        # a fresh process per stage; a stage that fails ends the run
            cmd = [sys.executable, os.path.abspath(__file__), "--stage", st, "--batches", str(a.batches), "--epochs", str(a.epochs),
                   "--repeats", str(a.repeats), "--recipes", a.recipes, "--draws", a.draws, "--augment", a.augment,
                   "--window", str(a.window)]
            r = subprocess.run(cmd, timeout=STAGE_LIMIT_S[st])
            if r.returncode != 0:
                sys.exit(f"stage {st} exited with {r.returncode}")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("datapipe_bench: no HIP device; nothing is measured without one")
    {"loader": stage_loader, "steps": stage_steps, "trace": lambda x: stage_steps(x, trace=True)}[a.stage](a)


if __name__ == "__main__":
    main()
