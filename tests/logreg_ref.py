"""Reference arithmetic for the linear-probe tests: the objective of ppt_logreg_fit_f32 (include/ppt_hip.h), its gradient and
its predictions from (W, b) in numpy at a chosen precision, and a plain L-BFGS on them.

    F(W, b) = sum_i ( logsumexp_k z_ik - z_{i, y_i} ) + ||W||^2 / (2 C),      z_i = W x_i + b

`lbfgs(..., dtype=np.float64)` is the solver used where no golden optimum exists; `dtype=np.float32` restates the device
solver's algorithm (10 pairs, Armijo backtracking with c1 = 1e-4 and a 4-ulp slack, first step 1 / ||g||, pairs with
s.y <= eps y.y skipped, the exact intercept step b_k += log(n_k / sum_i p_ik) at the start and after every accepted step) in
numpy's fp32, which is how the margins of tests/test_probe_gpu.py were measured.  Nothing here
imports sklearn or scipy.
"""
import numpy as np

GRID = [1e6, 1e4, 1e2, 1, 1e-2, 1e-4, 1e-6]


def make_banks(K=5, d=48, per=60, scale=0.45, seed=0):
    """the Gaussian banks of tests/golden/make_golden_linprobe.py: (train, test), each (features f32 [K per, d], labels i64)"""
    rng = np.random.RandomState(seed)
    mu = rng.randn(K, d) * scale

    def bank(n):
        y = np.repeat(np.arange(K), n)
        return (mu[y] + rng.randn(K * n, d)).astype(np.float32), y

    train = bank(per)
    test = bank(per)
    return train, test


def decision(X, W, b, dtype=np.float64):
    return X.astype(dtype) @ W.astype(dtype).T + b.astype(dtype)


def predict(X, W, b, dtype=np.float64):
    return decision(X, W, b, dtype).argmax(1)


def objective(X, y, W, b, C, dtype=np.float64):
    """-> (F, dF/dW, dF/db) in `dtype` (sums, not means)"""
    X = X.astype(dtype)
    W = W.astype(dtype)
    Z = X @ W.T + b.astype(dtype)
    m = Z.max(1, keepdims=True)
    E = np.exp(Z - m)
    s = E.sum(1, keepdims=True)
    rows = np.arange(len(y))
    loss = ((m[:, 0] + np.log(s[:, 0])) - Z[rows, y]).sum(dtype=dtype)
    P = E / s
    P[rows, y] -= 1
    invC = dtype(1) / dtype(C)
    F = loss + dtype(0.5) * invC * (W * W).sum(dtype=dtype)
    return F, P.T @ X + W * invC, P.sum(0, dtype=dtype)


def grad_max(X, y, W, b, C):
    """max |grad (F / n)| in fp64: the quantity the solver's stopping rule bounds"""
    _, gW, gb = objective(X, y, W, b, C)
    return max(np.abs(gW).max(), np.abs(gb).max()) / len(y)


def gap_rows(X, W, b, frac=0.03):
    """rows whose top-two logit gap at (W, b) is below `frac` of the row's logit range: predictions there are not determined
    by a solution that is only tol-stationary"""
    Z = decision(X, W, b)
    top = np.sort(Z, 1)
    return (top[:, -1] - top[:, -2]) < frac * (top[:, -1] - top[:, 0])


def lbfgs(X, y, K, C, tol=1e-4, max_iter=1000, dtype=np.float64, m=10):
    """-> (W, b, info) with info = dict(iters, nfev, status, gmax, fmean); status as PPT_LOGREG_*"""
    n, d = X.shape
    ft = dtype
    eps = ft(np.finfo(ft).eps)
    Xd = X.astype(ft)
    x = np.zeros(K * d + K, ft)

    def fg(v):
        F, gW, gb = objective(Xd, y, v[:K * d].reshape(K, d), v[K * d:], C, ft)
        return ft(F), np.concatenate([gW.ravel(), gb]).astype(ft)

    nk = np.bincount(y, minlength=K).astype(ft)

    def intercept_step(v):
        Z = Xd @ v[:K * d].reshape(K, d).T + v[K * d:]
        E = np.exp(Z - Z.max(1, keepdims=True))
        s = (E / E.sum(1, keepdims=True)).sum(0, dtype=ft)
        v = v.copy()
        v[K * d:] += np.where(nk > 0, np.log(np.where(nk > 0, nk, 1) / s), 0).astype(ft)
        return v

    x = intercept_step(x)
    f, g = fg(x)
    nfev, it, status = 2, 0, 1
    S, Y, rho = [], [], []
    gamma = ft(1)
    while True:
        gmax = np.abs(g).max() / ft(n)
        if gmax <= tol:
            status = 0
            break
        if it >= max_iter:
            status = 1
            break
        q = g.copy()
        al = []
        for s_, y_, r_ in zip(reversed(S), reversed(Y), reversed(rho)):
            a = r_ * ft(s_ @ q)
            al.append(a)
            q -= a * y_
        if S:
            q *= gamma
        for (s_, y_, r_), a in zip(zip(S, Y, rho), reversed(al)):
            q += (a - r_ * ft(y_ @ q)) * s_
        dirn = -q
        dg = ft(g @ dirn)
        if not dg < 0:
            if S:
                S, Y, rho = [], [], []
                continue
            status = 2
            break
        alpha = ft(1) / np.sqrt(ft(g @ g)) if not S else ft(1)
        ok = False
        for _ in range(30):
            xn = x + alpha * dirn
            fn, _ = fg(xn)
            nfev += 1
            if fn <= f + ft(1e-4) * alpha * dg + ft(4) * eps * abs(f):
                ok = True
                break
            alpha *= ft(0.5)
        it += 1
        if not ok:
            if S:
                S, Y, rho = [], [], []
                continue
            status = 2
            break
        xn = intercept_step(xn)
        fn, gn = fg(xn)
        nfev += 1
        s_, y_ = xn - x, gn - g
        x, f, g = xn, fn, gn
        sy, yy = ft(s_ @ y_), ft(y_ @ y_)
        if sy > eps * yy:
            S.append(s_); Y.append(y_); rho.append(ft(1) / sy)
            gamma = sy / yy
            if len(S) > m:
                S.pop(0); Y.pop(0); rho.pop(0)
    return x[:K * d].reshape(K, d), x[K * d:], dict(iters=it, nfev=nfev, status=status, gmax=float(np.abs(g).max() / n), fmean=float(f / n))


def make_case(K, d, n, ld=None):
    """the synthetic fit of the solver tests: n rows of d Gaussian features around K class means, every class present; ld > d
    pads the rows with NaN, which any read beyond column d would carry into the result -> (X [n, ld] f32, y [n] i64)"""
    rng = np.random.RandomState(100 + K + d + n)
    mu = rng.randn(K, d) * (0.45 if d < 100 else 0.12)
    y = np.arange(n) % K
    X = (mu[y] + rng.randn(n, d)).astype(np.float32)
    if ld is not None and ld > d:
        X = np.concatenate([X, np.full((n, ld - d), np.nan, np.float32)], 1)
    return X, y.astype(np.int64)
