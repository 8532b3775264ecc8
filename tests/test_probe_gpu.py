"""GPU: the batched logistic solver (csrc/logreg.hip) against fp64 recomputation and the converged optima of
tests/golden/g_linprobe.npz, and the linear-probe protocol and feature extraction of ppt_amd/probe.py on top of it.
No sklearn, no scipy: fp64 arithmetic comes from tests/logreg_ref.py."""
import functools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import logreg_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g_linprobe.npz")
SEEDS, SHOTS, CS = (1, 2, 3), (1, 2, 4, 8, 16), (1.0, 1e-2, 1e-6)
TOL = 1e-4
# (K, d, n, ld): tiny; several row passes; odd d with padded rows; K = 15 (ScanObjectNN); K = 40, d = 768 at 1 and 16 shots
# (the direction in LDS, 10 row passes, 2 row-sums per wave)
SHAPES = [(5, 48, 5, None), (5, 48, 80, None), (3, 37, 9, 40), (15, 256, 15, None), (40, 768, 40, None), (40, 768, 640, None)]


def _info(info):
    info = info.cpu().numpy()
    return dict(iters=info[:, 0], nfev=info[:, 1], status=info[:, 2], gmax=info[:, 3].copy().view(np.float32),
                fmean=info[:, 4].copy().view(np.float32), rest=info[:, 5:])


def _bank_of(X, y, extra=3):
    """a bank that holds the case's rows in reversed order behind `extra` rows of NaN that no fit selects"""
    n = len(y)
    bank = np.concatenate([np.full((extra, X.shape[1]), np.nan, np.float32), X[::-1]])
    labels = np.concatenate([np.zeros(extra, np.int64), y[::-1]])
    rows = (extra + n - 1 - np.arange(n)).astype(np.int32)          # row i of the fit = X[i]
    return torch.from_numpy(bank).cuda(), torch.from_numpy(labels).cuda(), rows


@functools.lru_cache(maxsize=None)
def grid_fit(shape):
    """the seven grid values of C in one launch on one synthetic case; computed once, shared by the tests below"""
    from ppt_amd import ops
    K, d, n, ld = shape
    X, y = R.make_case(K, d, n, ld)
    bank, labels, rows = _bank_of(X, y)
    rows7 = torch.from_numpy(np.tile(rows, (7, 1))).cuda()
    W, b, info = ops.logreg_fit(bank, labels, rows7, R.GRID, K, d=d, tol=TOL, max_iter=1000)
    torch.cuda.synchronize()
    return X[:, :d], y, W.cpu().numpy(), b.cpu().numpy(), _info(info), (bank, labels, rows7)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "K%d-d%d-n%d" % s[:3])
def test_stationary_over_the_grid(shape):
    """every fit of the grid stops converged, and max |grad (F / n)| recomputed in fp64 from the returned (W, b) is within 10 % of
    tol (the fp32 evaluation of the gradient: the numpy fp32 restatement differs from fp64 by <= 4e-8 on these cases)"""
    X, y, W, b, info, _ = grid_fit(shape)
    for f, c in enumerate(R.GRID):
        g = R.grad_max(X, y, W[f], b[f], c)
        print(f"C={c:g}: status {info['status'][f]}, {info['iters'][f]} iterations, {info['nfev'][f]} evaluations, "
              f"fp64 max|grad F/n| {g:.3e} (reported {info['gmax'][f]:.3e})")
    for f, c in enumerate(R.GRID):
        assert info["status"][f] == 0, (c, info["status"][f])
        assert np.isfinite(W[f]).all() and np.isfinite(b[f]).all()
        assert R.grad_max(X, y, W[f], b[f], c) <= 1.1 * TOL, c
        assert (info["rest"][f] == 0).all() and 1 <= info["iters"][f] < info["nfev"][f] <= 31 * info["iters"][f] + 2          # <= 30 trials + the intercept step per iteration


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "K%d-d%d-n%d" % s[:3])
def test_reported_values(shape):
    """info's final F / n and max |grad (F / n)| against fp64 at the returned point.  Margins: 10 x the largest error of the numpy
    fp32 restatement (logreg_ref.lbfgs(dtype=float32)) over these 6 x 7 cases, which is 4.0e-8 for the gradient norm and 3.2e-7
    for F / n (at F / n = 3.6: under one ulp of an fp32 sum of n terms)."""
    X, y, W, b, info, _ = grid_fit(shape)
    n = len(y)
    for f, c in enumerate(R.GRID):
        F64 = R.objective(X, y, W[f], b[f], c)[0] / n
        g64 = R.grad_max(X, y, W[f], b[f], c)
        print(f"C={c:g}: F/n {info['fmean'][f]:.7g} vs {F64:.7g} (diff {abs(info['fmean'][f] - F64):.2e}); "
              f"gmax diff {abs(info['gmax'][f] - g64):.2e}")
    for f, c in enumerate(R.GRID):
        assert abs(info["fmean"][f] - R.objective(X, y, W[f], b[f], c)[0] / n) <= 3.2e-6, c
        assert abs(info["gmax"][f] - R.grad_max(X, y, W[f], b[f], c)) <= 4.0e-7, c


@functools.lru_cache(maxsize=None)
def golden_fits():
    """the 45 golden cases: one solver launch and one prediction launch per shot count (3 seeds x 3 values of C)"""
    from ppt_amd import ops
    G = np.load(GOLDEN)
    (Xtr, ytr), (Xte, yte) = R.make_banks()
    train, labels, test = torch.from_numpy(Xtr).cuda(), torch.from_numpy(ytr).cuda(), torch.from_numpy(Xte).cuda()
    pred, status = {}, {}
    for ni, shot in enumerate(SHOTS):
        rows = np.stack([G[f"sel_train_s{seed}_n{shot}"] for seed in SEEDS for _ in CS]).astype(np.int32)
        W, b, info = ops.logreg_fit(train, labels, torch.from_numpy(rows).cuda(), [c for _ in SEEDS for c in CS], 5, tol=TOL)
        p = ops.logreg_predict(test, W, b).cpu().numpy().reshape(3, 3, -1)
        st = _info(info)["status"].reshape(3, 3)
        for si in range(3):
            for ci in range(3):
                pred[si, ni, ci], status[si, ni, ci] = p[si, ci], st[si, ci]
    return G, Xte, pred, status


@pytest.mark.parametrize("ci", range(3), ids=["C1", "C1e-2", "C1e-6"])
def test_predictions_equal_the_optimums(ci):
    """Predictions on the 300-row test bank equal those of the converged fp64 optimum, except on rows whose top-two logit gap at
    the optimum is below 0.03 of the row's logit range (at most 10 % of the bank), for seeds 1-3 and 1, 2, 4, 8, 16 shots.

    At C = 1e-6 ||W x|| is ~1e-5 and the intercept alone decides the arg-max; a point that is merely tol-stationary does not
    determine it (sklearn at tol = 1e-4, and its tol = 1e-12 answer too, differ from the optimum on 469 rows outside the gap
    rule over the 15 cases, which is why the stored optimum is polished, tests/golden/make_golden_linprobe.py).  The solver's
    exact intercept step is what makes this case hold.  Measured with the numpy fp32 restatement: 0 rows outside the gap rule
    at every C, at most 2 inside it."""
    G, Xte, pred, status = golden_fits()
    worst = 0
    for si in range(3):
        for ni in range(5):
            gap = R.gap_rows(Xte, G["opt_W"][si, ni, ci], G["opt_b"][si, ni, ci])
            wrong = pred[si, ni, ci] != G["opt_pred"][si, ni, ci]
            print(f"seed {SEEDS[si]}, {SHOTS[ni]} shot, C={CS[ci]:g}: status {status[si, ni, ci]}, {wrong.sum()} rows differ, "
                  f"{(wrong & ~gap).sum()} outside the gap rule ({gap.sum()} rows inside it)")
            assert gap.sum() <= 30 and status[si, ni, ci] == 0
            worst = max(worst, int((wrong & ~gap).sum()))
    assert worst == 0


def test_independent_and_deterministic():
    """a fit alone, inside a launch of 7, in a second run and in a permuted launch: the same bytes"""
    from ppt_amd import ops
    shape = SHAPES[3]
    _, _, _, _, _, (bank, labels, rows7) = grid_fit(shape)
    K, d = shape[0], shape[1]

    def run(order):
        W, b, info = ops.logreg_fit(bank, labels, rows7[:len(order)].contiguous(), [R.GRID[i] for i in order], K, d=d, tol=TOL)
        return W.cpu().numpy(), b.cpu().numpy(), info.cpu().numpy()

    base = run(range(7))
    again = run(range(7))
    for a, c in zip(base, again):
        assert a.tobytes() == c.tobytes()
    for f in (0, 3, 6):
        alone = run([f])
        for a, c in zip(base, alone):
            assert a[f].tobytes() == c[0].tobytes(), f
    perm = [4, 0, 6, 2, 5, 1, 3]
    shuffled = run(perm)
    for a, c in zip(base, shuffled):
        assert a[perm].tobytes() == c.tobytes()


def test_iteration_cap():
    from ppt_amd import ops
    K, d, n, _ = SHAPES[5]
    X, y, _, _, _, (bank, labels, rows7) = grid_fit(SHAPES[5])
    W, b, info = ops.logreg_fit(bank, labels, rows7[:1].contiguous(), [1.0], K, d=d, tol=TOL, max_iter=3)
    info = _info(info)
    assert info["status"][0] == 1 and info["iters"][0] == 3
    W, b = W.cpu().numpy()[0], b.cpu().numpy()[0]
    assert np.isfinite(W).all() and np.isfinite(b).all()
    F = R.objective(X, y, W, b, 1.0)[0] / n
    print("F/n after 3 iterations:", F, "reported", info["fmean"][0], "start", np.log(K))
    assert F < np.log(K) and info["fmean"][0] < np.log(K)


def test_bad_label_and_bad_row_stop_their_fit_only():
    from ppt_amd import ops
    K, d, n, _ = SHAPES[1]
    X, y = R.make_case(K, d, n)
    bank, labels, rows = _bank_of(X, y)
    labels = torch.cat([labels, torch.tensor([K, -1], device="cuda")])                    # two rows with labels outside [0, K)
    bank = torch.cat([bank, bank[-2:]])
    N = bank.shape[0]
    rows4 = np.tile(rows, (4, 1))
    rows4[1, 7] = N - 2          # label K
    rows4[2, 0] = N              # a row outside the bank
    rows4[3, n - 1] = N - 1      # label -1
    W, b, info = ops.logreg_fit(bank, labels, torch.from_numpy(rows4).cuda(), [1.0] * 4, K, d=d, tol=TOL)
    info = _info(info)
    assert info["status"].tolist() == [0, 3, 3, 3]
    assert (W[1:] == 0).all() and (b[1:] == 0).all() and (info["iters"][1:] == 0).all()
    assert R.grad_max(X, y, W[0].cpu().numpy(), b[0].cpu().numpy(), 1.0) <= 1.1 * TOL
    pred = ops.logreg_predict(bank, W[:1].contiguous(), b[:1].contiguous(), torch.tensor([3, N, -1, 4], dtype=torch.int32, device="cuda"))
    assert pred[0, 1] == -1 and pred[0, 2] == -1 and 0 <= pred[0, 0] < K


def test_predict_is_the_first_argmax_in_fp32():
    from ppt_amd import ops
    rng = np.random.RandomState(5)
    for K, d, ld, N in ((5, 48, 48, 300), (3, 37, 40, 70), (40, 768, 768, 130), (64, 1024, 1024, 65)):
        X = rng.randn(N, ld).astype(np.float32)
        X[:, d:] = np.nan
        W = rng.randn(2, K, d).astype(np.float32)
        b = rng.randn(2, K).astype(np.float32)
        W[1, K - 1], b[1, K - 1] = W[1, 1], b[1, 1]          # a tie between classes 1 and K - 1: the first wins
        pred = ops.logreg_predict(torch.from_numpy(X).cuda(), torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
        sub = torch.tensor([N - 1, 0, 5], dtype=torch.int32, device="cuda")
        part = ops.logreg_predict(torch.from_numpy(X).cuda(), torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda(), sub).cpu().numpy()
        assert np.array_equal(part, pred[:, [N - 1, 0, 5]])
        for f in range(2):
            Z = R.decision(X[:, :d], W[f], b[f])
            if f == 1:
                Z = Z[:, :K - 1]          # class K - 1 repeats class 1 and may never be named
            top = np.sort(Z, 1)
            clear = (top[:, -1] - top[:, -2]) > 1e-4 * np.abs(Z).max()          # fp32 dot products of d terms: ~1e-6 relative
            assert clear.mean() > 0.9 and np.array_equal(pred[f][clear], Z.argmax(1)[clear])
        assert not (pred[1] == K - 1).any()


def test_protocol_end_to_end(tmp_path):
    from ppt_amd import probe
    train, test = R.make_banks()
    (Xtr, ytr), (Xte, yte) = train, test
    res = probe.linear_probe(train, test, shots=(1, 4, 16), num_run=3, num_step=3, out_dir=str(tmp_path), keep_coef=True)
    for shot in (1, 4, 16):
        for r in range(3):
            tr, va = probe.select_shots(ytr, yte, shot, r + 1)
            assert np.array_equal(res["selections"][shot][r][0], tr) and np.array_equal(res["selections"][shot][r][1], va)
            # the path of C recomputed from the validation accuracies the device reported
            val = res["val"][shot][r]
            c_peak = probe.SEARCH_LIST[int(np.argmax(val["grid"]))]
            lo, hi = np.log10(0.1 * c_peak), np.log10(10 * c_peak)
            for step, ((c, acc), (a_left, a_right)) in enumerate(zip(res["steps"][shot][r], val["steps"])):
                right = a_left < a_right
                assert np.isclose(c, 10 ** (hi if right else lo), rtol=1e-9), (shot, r, step)
                lo, hi = (0.5 * (lo + hi), hi) if right else (lo, 0.5 * (lo + hi))
                # the reported accuracy against fp64 predictions from the returned coefficients
                W, b = (t.numpy() for t in res["coef"][shot][r][step])
                count = (R.predict(Xte, W, b) == yte).sum()
                slack = R.gap_rows(Xte, W, b).sum()
                assert abs(acc / 100 * len(yte) - count) <= slack + 1e-6, (shot, r, step, acc, count, slack)
                assert R.grad_max(Xtr[tr], ytr[tr], W, b, c) <= 1.1 * TOL
        last = [res["steps"][shot][r][-1][1] for r in range(3)]
        assert np.allclose(res["summary"][shot], (np.mean(last), np.std(last)))
    details = open(tmp_path / "mn40-run3-step3_details.txt").read().splitlines()
    assert len(details) == 27
    for line in details:
        assert re.fullmatch(r"modelnet40, seed [123], (1|4|16) shot, weight [0-9.e+-]+, test_acc \d+\.\d\d", line), line
    summary = open(tmp_path / "mn40-run3-step3.txt").read().splitlines()
    assert len(summary) == 3
    for line in summary:
        assert re.fullmatch(r"modelnet40, (1|4|16) Shot, Test acc stat: \d+\.\d\d \(\d+\.\d\d\)", line), line


def test_extract_features():
    """10 clouds in batches of 4, 4 and 2 through the synthetic ULIP_PointBERT's point encoder: the bank equals
    point_encoder.eval()(pc) batch by batch, bit for bit; training flag and precision mode are the caller's afterwards"""
    from ppt_amd import probe, weights as Wt
    from ppt_amd.models import ULIP_models as M
    args = SimpleNamespace(classnames=M.dataset_classnames("modelnet40"), template_init='', class_name_position='middle',
                           num_learnable_prompt_tokens=32, gpu=0, task='cls', head_type=0, evaluate_3d=False, ulip2=False,
                           synthetic_weights=True)
    m = M.ULIP_PointBERT(args)
    m.load_state_dict(Wt.ulip_pointbert_state_dict(seed=0), strict=False)
    m.cuda()
    m.train()
    mode = m.precision_name
    enc = m.point_encoder
    pc_np, start = Wt.synth_clouds(10, 1024, seed=5)
    pc, start = torch.from_numpy(pc_np), torch.from_numpy(start)
    labels = torch.arange(10) % 7
    cuts = [(0, 4), (4, 8), (8, 10)]

    def batches():
        for lo, hi in cuts:
            enc.fps_start = start[lo:hi].cuda()          # the FPS start is a random draw otherwise: pinned for the comparison
            yield pc[lo:hi], labels[lo:hi], "ignored"

    feats, labs = probe.extract_features(enc, batches())
    assert enc.training and m.training and m.precision_name == mode
    assert feats.is_cuda and feats.dtype == torch.float32 and feats.shape[0] == 10 and labs.dtype == torch.int64
    assert labs.cpu().tolist() == labels.tolist()
    enc.eval()
    with torch.no_grad():
        for lo, hi in cuts:
            enc.fps_start = start[lo:hi].cuda()
            want = enc(pc[lo:hi].cuda()).float()
            assert torch.equal(feats[lo:hi], want), (lo, hi)
    assert torch.isfinite(feats).all()
