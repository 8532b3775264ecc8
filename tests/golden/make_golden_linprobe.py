"""Writes tests/golden/g_linprobe.npz: what the linear-probe tests compare against and cannot compute without sklearn.

    python tests/golden/make_golden_linprobe.py          (needs numpy and scikit-learn; the tests need neither sklearn nor this)

Banks: tests/logreg_ref.make_banks() -- K = 5 classes, d = 48, 60 rows per class, train then test from RandomState(0).
For seeds 1-3:
  sel_train_s{seed}_n{shot} / sel_val_s{seed}_n{shot}: the few-shot selections, by the literal numpy calls of the reference's
      linear_probe.py:28-46 (np.random.seed(seed); per label np.random.choice(where(label), size, replace=False); every train
      draw before any validation draw; validation shots {1:1, 2:2, 4:4, 8:4, 16:4}; the validation pool is the test bank, :21);
  for shots {1, 2, 4, 8, 16} and C in {1, 1e-2, 1e-6}, as arrays indexed [seed - 1, shot index, C index]:
      opt_W [3,5,3,K,d], opt_b [3,5,3,K] (f64): the converged optimum -- sklearn lbfgs on float64 features, tol = 1e-12,
      max_iter = 5000, then polished by Newton steps in float64: scipy's L-BFGS-B also stops on its relative-decrease test, which
      leaves max |grad (F / n)| between 2e-9 and 5e-6 on these cases (worst at C = 1e-6); the polish moves no coefficient by more
      than 2.6e-5 and brings the gradient below 1e-9 (2.5e-16; tests/test_probe_cpu.py asserts the bound).  At C = 1e-6, where
      the intercept decides the arg-max, it changes 554 of sklearn's 4 500 test predictions; at C = 1 and 1e-2 none;
      opt_pred [3,5,3,300] (int8): the optimum's predictions on the test bank;  opt_dec [3,5,3,300,K] (f32): its decision
      values there.
"""
import os
import sys

import numpy as np
from sklearn.linear_model import LogisticRegression

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import logreg_ref as R          # noqa: E402

SEEDS, SHOTS, CS = (1, 2, 3), (1, 2, 4, 8, 16), (1.0, 1e-2, 1e-6)
VAL_SHOTS = {1: 1, 2: 2, 4: 4, 8: 4, 16: 4}


def polish(X, y, W, b, C, steps=4):
    """Newton steps on F in float64 from sklearn's answer; the Hessian is singular along a common shift of the intercepts (F does
    not change there), so the step is the least-squares one."""
    n, d = X.shape
    K = W.shape[0]
    Xa = np.concatenate([X, np.ones((n, 1))], 1)
    reg = np.concatenate([np.ones(d), [0.0]]) / C
    for _ in range(steps):
        _, gW, gb = R.objective(X, y, W, b, C)
        Z = R.decision(X, W, b)
        P = np.exp(Z - Z.max(1, keepdims=True))
        P /= P.sum(1, keepdims=True)
        H = np.zeros((K, d + 1, K, d + 1))
        for k in range(K):
            for l in range(K):
                wgt = P[:, k] * ((k == l) - P[:, l])
                H[k, :, l, :] = (Xa * wgt[:, None]).T @ Xa + (np.diag(reg) if k == l else 0)
        step = np.linalg.lstsq(H.reshape(K * (d + 1), -1), -np.concatenate([gW, gb[:, None]], 1).ravel(), rcond=1e-13)[0].reshape(K, d + 1)
        W, b = W + step[:, :d], b + step[:, d]
    return W, b


def main():
    (Xtr, ytr), (Xte, yte) = R.make_banks()
    K, d = 5, Xtr.shape[1]
    out = dict(seeds=np.array(SEEDS), shots=np.array(SHOTS), cs=np.array(CS))
    W = np.zeros((len(SEEDS), len(SHOTS), len(CS), K, d))
    b = np.zeros((len(SEEDS), len(SHOTS), len(CS), K))
    pred = np.zeros((len(SEEDS), len(SHOTS), len(CS), len(yte)), np.int8)
    dec = np.zeros((len(SEEDS), len(SHOTS), len(CS), len(yte), K), np.float32)
    worst, moved, flips = 0.0, 0.0, 0
    for si, seed in enumerate(SEEDS):
        for ni, shot in enumerate(SHOTS):
            np.random.seed(seed)
            sel = []
            for label in np.unique(ytr):
                sel.extend(np.random.choice(np.where(ytr == label)[0], size=shot, replace=False))
            val = []
            for label in np.unique(ytr):
                val.extend(np.random.choice(np.where(yte == label)[0], size=VAL_SHOTS[shot], replace=False))
            out[f"sel_train_s{seed}_n{shot}"] = np.array(sel, np.int64)
            out[f"sel_val_s{seed}_n{shot}"] = np.array(val, np.int64)
            X, y = Xtr[sel].astype(np.float64), ytr[sel]
            for ci, c in enumerate(CS):
                clf = LogisticRegression(solver="lbfgs", penalty="l2", C=c, tol=1e-12, max_iter=5000).fit(X, y)
                Wp, bp = polish(X, y, clf.coef_, clf.intercept_, c)
                moved = max(moved, np.abs(Wp - clf.coef_).max(), np.abs(bp - clf.intercept_).max())
                flips += int((R.predict(Xte, Wp, bp) != clf.predict(Xte.astype(np.float64))).sum())
                W[si, ni, ci], b[si, ni, ci] = Wp, bp
                pred[si, ni, ci] = R.predict(Xte, Wp, bp)
                dec[si, ni, ci] = R.decision(Xte, Wp, bp)
                worst = max(worst, R.grad_max(X, y, Wp, bp, c))
    out.update(opt_W=W, opt_b=b, opt_pred=pred, opt_dec=dec)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g_linprobe.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; worst max|grad(F/n)| at a stored optimum:", worst,
          "; largest coefficient change by the polish:", moved, "; test predictions it changed:", flips)


if __name__ == "__main__":
    main()
