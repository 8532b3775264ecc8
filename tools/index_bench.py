"""Dev tool: the three index kernels every encoder starts with (FPS, kNN grouping, multi-radius ball query), timed like for like
between two builds of libppt_hip.so loaded into ONE process and alternated window by window:

    bash tools/build_variant.sh parent            # at the commit to compare with -> tools/_build/libppt_parent.so
    python tools/index_bench.py --base tools/_build/libppt_parent.so [--new ppt_amd/csrc/libppt_hip.so] [--ragged] [--out x.json]

Every shape gets `--rounds` rounds of (base, new, base, new ...) windows of `--launches` launches each, timed with device events
after a warm-up of both.  Per build: the median window of every round, in us per launch; `base_spread` is the range of the base
build's own round medians, the yardstick for "no slower".  The uniform entry points are called directly (ctypes), so a base build
without the ragged symbols loads.  --ragged adds, for the new build only, one ragged FPS / kNN / ball-query launch (B 32, lengths
uniform in [1024, 8192], Nmax 8192) against the same clouds as 32 single-cloud launches and against a uniform launch at Nmax."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from ppt_amd import weights as W
from ppt_amd._lib import _SIGNATURES, BallMulti      # the package's one binding of the signatures and of struct ppt_ball_multi

c_void_p = ctypes.c_void_p


def p(t):
    return c_void_p(t.data_ptr())


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: error {rc}")


RADII = ((0.1, 16), (0.2, 32), (0.4, 128))


class Case:
    """one launch of one entry point on fixed buffers; lengths=None: the uniform entry point"""

    def __init__(self, kind, B, N, M, lengths=None, seed=3):
        pc, start = W.synth_clouds(B, N, seed=seed)
        self.kind, self.B, self.N, self.M = kind, B, N, M
        self.pc, self.start = torch.from_numpy(pc).cuda(), torch.from_numpy(start).cuda()
        self.lengths = None if lengths is None else torch.from_numpy(np.asarray(lengths, dtype=np.int32)).cuda()
        if lengths is not None:
            self.start = torch.from_numpy(start % np.asarray(lengths)).cuda()
        self.idx = torch.empty((B, M), dtype=torch.int64, device="cuda")
        self.ctr = self.pc[:, :M].contiguous()                   # centres for kNN / ball query: the clouds' first M rows
        self.out3 = torch.empty((B, M, 3), dtype=torch.float32, device="cuda")
        if kind == "knn":
            self.nb = torch.empty((B, M, 32, 3), dtype=torch.float32, device="cuda")
        if kind == "ball":
            self.q = BallMulti()
            self.q.n = 3
            self.keep = []
            for j, (r, K) in enumerate(RADII):
                i = torch.empty((B, M, K), dtype=torch.int64, device="cuda")
                g = torch.empty((B, M, K, 3), dtype=torch.float32, device="cuda")
                self.keep += [i, g]
                self.q.r2[j], self.q.K[j], self.q.idx[j], self.q.gxyz[j] = float(np.float32(r * r)), K, i.data_ptr(), g.data_ptr()

    def launch(self, L):
        B, N, M, ln = self.B, self.N, self.M, self.lengths
        if self.kind == "fps":
            if ln is None:
                check(L.ppt_fps_f32(p(self.pc), B, N, M, p(self.start), p(self.idx), p(self.out3), stream()), "fps")
            else:
                check(L.ppt_fps_ragged_f32(p(self.pc), B, N, M, p(self.start), p(ln), p(self.idx), p(self.out3), stream()), "fps ragged")
        elif self.kind == "knn":
            if ln is None:
                check(L.ppt_knn_group_f32(p(self.pc), p(self.ctr), B, N, M, 32, None, p(self.nb), None, stream()), "knn")
            else:
                check(L.ppt_knn_group_ragged_f32(p(self.pc), p(self.ctr), B, N, M, 32, p(ln), None, p(self.nb), None, stream()), "knn ragged")
        else:
            if ln is None:
                check(L.ppt_ball_query_multi_f32(p(self.pc), p(self.ctr), B, N, M, ctypes.byref(self.q), stream()), "ball")
            else:
                check(L.ppt_ball_query_multi_ragged_f32(p(self.pc), p(self.ctr), B, N, M, p(ln), ctypes.byref(self.q), stream()), "ball ragged")


def window(fn, launches):
    """us per call of fn() over one window of `launches` calls"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(launches):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / launches


def load(path):
    L = ctypes.CDLL(os.path.abspath(path))
    for name in ("ppt_fps_f32", "ppt_knn_group_f32", "ppt_ball_query_multi_f32", "ppt_fps_ragged_f32", "ppt_knn_group_ragged_f32",
                 "ppt_ball_query_multi_ragged_f32"):
        if hasattr(L, name):                    # (a base build from before the ragged forms lacks those)
            getattr(L, name).restype, getattr(L, name).argtypes = _SIGNATURES[name]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True)
    ap.add_argument("--new", default=os.path.join(ROOT, "ppt_amd", "csrc", "libppt_hip.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    libs = {"base": load(a.base), "new": load(a.new)}
    result = {"uniform": [], "ragged": []}
    for kind, B, N, M in (("fps", 32, 1024, 512), ("fps", 64, 2048, 512), ("fps", 32, 8192, 512), ("knn", 32, 1024, 512), ("ball", 32, 8192, 512)):
        case = Case(kind, B, N, M)
        for L in libs.values():
            window(lambda: case.launch(L), 5)
        med = {"base": [], "new": []}
        for _ in range(a.rounds):
            for name, L in libs.items():
                med[name].append(float(np.median([window(lambda: case.launch(L), a.launches) for _ in range(a.windows)])))
        row = dict(kind=kind, B=B, N=N, M=M, base_us=[round(x, 2) for x in med["base"]], new_us=[round(x, 2) for x in med["new"]],
                   base_median=round(float(np.median(med["base"])), 2), new_median=round(float(np.median(med["new"])), 2),
                   base_spread=round(max(med["base"]) - min(med["base"]), 2))
        row["new_within_base_spread"] = bool(row["new_median"] <= max(med["base"]))
        result["uniform"].append(row)
        print(json.dumps(row), flush=True)
    if a.ragged:
        L = libs["new"]
        B, Nmax, M = 32, 8192, 512
        lengths = np.random.default_rng(5).integers(1024, Nmax + 1, size=B)
        for kind in ("fps", "knn", "ball"):
            rag, uni = Case(kind, B, Nmax, M, lengths=lengths), Case(kind, B, Nmax, M)
            singles = [Case(kind, 1, int(n), M, seed=100 + i) for i, n in enumerate(lengths)]
            fns = {"ragged_one_launch": lambda: rag.launch(L), "uniform_at_Nmax": lambda: uni.launch(L),
                   "single_cloud_launches": lambda: [c.launch(L) for c in singles]}
            row = dict(kind=kind, B=B, Nmax=Nmax, M=M, lengths_mean=float(lengths.mean()))
            for name, fn in fns.items():
                window(fn, 3)
                row[name + "_us"] = round(float(np.median([window(fn, 10) for _ in range(5)])), 2)
            result["ragged"].append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
