"""Times the default linear-probe protocol (5 shot counts x 10 seeds x (7 + 2 x 8) fits = 1 150 fits) on synthetic
ModelNet40-sized banks: 9 843 x 768 train, 2 468 x 768 test, 40 classes, Gaussian classes as in tests/logreg_ref.make_banks
with class means of scale 0.12.

    python tools/linprobe_time.py                      # the device protocol (ppt_amd.probe.linear_probe), needs the GPU
    python tools/linprobe_time.py --sklearn --num_run 2   # the reference's solver on the CPU, same banks, same protocol code

Device: wall clock around a device synchronisation, kernel time per launch from events around the two entry points, the
iteration histogram from the info records.  sklearn: wall clock; states the core count.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def banks(d=768, K=40, n_train=9843, n_test=2468, scale=0.12, seed=0):
    rng = np.random.RandomState(seed)
    mu = rng.randn(K, d) * scale

    def bank(n):
        y = np.arange(n) % K
        return (mu[y] + rng.randn(n, d)).astype(np.float32), y.astype(np.int64)

    return bank(n_train), bank(n_test)


class SklearnFit:
    """the batched fit-and-score of ppt_amd.probe over sklearn.LogisticRegression, as linear_probe.py:55-57 calls it"""

    def __init__(self, train, test):
        self.train, self.test, self.fits, self.iters = train, test, 0, []

    def __call__(self, train_rows, val_rows, Cs):
        from sklearn.linear_model import LogisticRegression
        (Xtr, ytr), (Xte, yte) = self.train, self.test
        Cs = np.asarray(Cs)
        val_acc, test_acc = np.zeros(Cs.shape), np.zeros(Cs.shape)
        for r in range(Cs.shape[0]):
            for g in range(Cs.shape[1]):
                clf = LogisticRegression(solver="lbfgs", max_iter=1000, penalty="l2", C=Cs[r, g]).fit(Xtr[train_rows[r]], ytr[train_rows[r]])
                hit = clf.predict(Xte) == yte
                val_acc[r, g], test_acc[r, g] = hit[val_rows[r]].mean(), hit.mean()
                self.fits += 1
                self.iters.append(int(clf.n_iter_[0]))
        return val_acc, test_acc, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--num_run", type=int, default=10)
    ap.add_argument("--num_step", type=int, default=8)
    a = ap.parse_args()
    train, test = banks()
    from ppt_amd import probe
    out = dict(num_run=a.num_run, num_step=a.num_step, train=list(train[0].shape), test=list(test[0].shape))
    if a.sklearn:
        fit = SklearnFit(train, test)
        t0 = time.perf_counter()
        res = probe.linear_probe(train, test, num_run=a.num_run, num_step=a.num_step, fit=fit)
        out.update(solver="sklearn lbfgs, fp32 features", cores=os.cpu_count(), wall_s=time.perf_counter() - t0, fits=fit.fits,
                   iterations=np.bincount(np.minimum(np.array(fit.iters) // 10, 100)).tolist(), iterations_bin=10)
    else:
        import torch
        from ppt_amd import ops
        events = []

        def timed(fn, name):
            def call(*args, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = fn(*args, **kw)
                e1.record()
                events.append((name, e0, e1))
                return r
            return call

        ops.logreg_fit, ops.logreg_predict = timed(ops.logreg_fit, "fit"), timed(ops.logreg_predict, "predict")
        fit = probe.DeviceFit(train, test)
        probe.linear_probe(train, test, shots=(1,), num_run=2, num_step=1, fit=fit)          # warm-up: module load, allocator
        torch.cuda.synchronize()
        fit.launches.clear(); events.clear()
        t0 = time.perf_counter()
        res = probe.linear_probe(train, test, num_run=a.num_run, num_step=a.num_step, fit=fit)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        infos = [(F, n, info.cpu().numpy()) for F, n, info in fit.launches]
        iters = np.concatenate([i[:, 0] for _, _, i in infos])
        status = np.concatenate([i[:, 2] for _, _, i in infos])
        ms = {}
        for name, e0, e1 in events:
            ms.setdefault(name, []).append(e0.elapsed_time(e1))
        per_launch = [dict(fits=F, rows=n, fit_ms=round(f, 3), predict_ms=round(p, 3), max_iterations=int(i[:, 0].max()))
                      for (F, n, i), f, p in zip(infos, ms["fit"], ms["predict"])]
        out.update(solver="ppt_logreg_fit_f32", wall_s=wall, fits=int(len(iters)), launches=len(infos),
                   fit_ms_total=sum(ms["fit"]), predict_ms_total=sum(ms["predict"]),
                   status_counts=np.bincount(status, minlength=4).tolist(),
                   iterations=np.bincount(np.minimum(iters // 10, 100)).tolist(), iterations_bin=10, per_launch=per_launch)
    out["summary"] = {str(k): [round(v[0], 2), round(v[1], 2)] for k, v in res["summary"].items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
