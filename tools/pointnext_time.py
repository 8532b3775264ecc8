"""Times the PointNeXt-S point encoder (ppt_amd/models/pointnext) and a prompt-only ULIP_PN_NEXT training step, per precision mode:

    encoder eval / train     PointNEXT() forward on a resident batch of 32 x 1024 clouds with height, eager and replayed from its hipGraph
    step                     train.Trainer.step of ULIP_PN_NEXT (ModelNet40 names, frozen encoder in train mode, prompt tokens training)
    launches                 calls into libppt_hip.so per eager forward, by entry point (ATen launches in between are not counted)

    python tools/pointnext_time.py [--batch 32] [--npoints 1024] [--window 0.5] [--out FILE.json]

Synthetic weights and clouds; host clock around a window of calls that ends in a device synchronise, after warm-up calls that also
capture the graphs; a candidate's window holds as many calls as fill `--window` seconds (counted from a trial window of 20); the
candidates of a mode alternate in five rounds; median, min and max of the per-call time in milliseconds.  The mixed mode is timed in
both operand formats (engine.POINTNEXT_F16: IEEE half, the default, and bf16).  Prints one
JSON line (profiles/r21_pointnext.md).
"""
import argparse
import collections
import contextlib
import io
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--npoints", type=int, default=1024)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of work per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ppt_amd import _lib, engine, graphs, ops, weights as W
    from ppt_amd.models import ULIP_models as M
    from ppt_amd.models.pointnext.pointnext import PointNEXT
    from ppt_amd.train import Trainer
    assert torch.cuda.is_available(), "pointnext_time.py measures on the GPU"
    B, N = a.batch, a.npoints
    pc = ops.cloud_height(torch.from_numpy(W.synth_clouds(B, N, seed=7)[0]).cuda())
    label = (torch.arange(B, device="cuda") % 40)
    sd = W.synth_state_dict(W.pointnext_spec(prefix=""), seed=0)

    def window(fn, reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / reps

    def stats(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    res = {"batch": B, "npoints": N, "window_s": a.window, "rounds": a.rounds, "modes": {}}
    for tag in ("fp32", "split16", "mixed16", "mixed16_bf16"):
        mode = "mixed16" if tag.startswith("mixed16") else tag
        engine.POINTNEXT_F16 = tag != "mixed16_bf16"
        cands = {}
        for train in (False, True):
            for graphed in (False, True):
                m = PointNEXT()
                m.load_state_dict(sd)
                m.cuda().train(train)
                m.precision = torch.bfloat16 if mode == "mixed16" else torch.float32
                m.split16 = mode == "split16"
                m.use_hip_graphs = graphed
                cands[("train" if train else "eval") + ("_graph" if graphed else "_eager")] = (lambda m=m: m(pc))
        names = M.dataset_classnames("modelnet40")
        args = SimpleNamespace(classnames=names, template_init='', class_name_position='middle', num_learnable_prompt_tokens=32, gpu=0,
                               task='cls', head_type=0, evaluate_3d=False, ulip2=False, synthetic_weights=True)
        with contextlib.redirect_stdout(io.StringIO()):
            u = M.ULIP_PN_NEXT(args)
        u.load_state_dict(W.ulip_pn_next_state_dict(seed=0), strict=False)
        u.prompt_learner.embedding = W.synth_prompt_embedding(len(names), seed=0)
        u.cuda().train()
        u.set_precision(mode)
        tr = Trainer(u, distributed=False)
        tr.inputs_ready = True
        cands["step"] = lambda: tr.step(pc, label)
        for fn in cands.values():                                   # warm-up: eager calls, captures, first replays
            for _ in range(graphs.WARMUP_CALLS + 3):
                fn()
        torch.cuda.synchronize()
        reps = {k: max(20, int(a.window / (window(fn, 20) * 1e-3)) + 1) for k, fn in cands.items()}
        times = {k: [] for k in cands}
        for _ in range(a.rounds):
            for k, fn in cands.items():
                times[k].append(window(fn, reps[k]))
        tr.finish()
        row = {k: stats(v) for k, v in times.items()}
        row["calls_per_window"] = reps
        row["clouds_per_s_eval_graph"] = round(B / (row["eval_graph"]["median"] * 1e-3), 1)
        row["clouds_per_s_step"] = round(B / (row["step"]["median"] * 1e-3), 1)
        # launches of one eager forward, by entry point
        for train in (False, True):
            m = PointNEXT()
            m.load_state_dict(sd)
            m.cuda().train(train)
            m.precision = torch.bfloat16 if mode == "mixed16" else torch.float32
            m.split16 = mode == "split16"
            m.use_hip_graphs = False
            m(pc)
            count, real = collections.Counter(), _lib.check

            def check(rc, name, count=count, real=real):
                count[name] += 1
                return real(rc, name)
            _lib.check = check
            try:
                m(pc)
            finally:
                _lib.check = real
            row["launches_train" if train else "launches_eval"] = {"total": sum(count.values()), **dict(sorted(count.items()))}
        row["operands"] = str(engine.POINTNEXT_F16 and "float16" or "bfloat16") if mode == "mixed16" else "float32"
        res["modes"][tag] = row
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
