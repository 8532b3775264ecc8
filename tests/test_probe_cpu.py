"""CPU: the linear probe's host side -- shot selection, the C search's control flow, the bank files, the argument checks of the
solver's entry points -- and the fixture's own consistency.  No GPU, no sklearn."""
import ctypes
import os

import numpy as np
import pytest

import logreg_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g_linprobe.npz")
SEEDS, SHOTS, CS = (1, 2, 3), (1, 2, 4, 8, 16), (1.0, 1e-2, 1e-6)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def banks():
    return R.make_banks()


def test_select_shots_equals_the_stored_draws(golden, banks):
    from ppt_amd import probe
    (_, ytr), (_, yte) = banks
    for seed in SEEDS:
        for shot in SHOTS:
            tr, va = probe.select_shots(ytr, yte, shot, seed)
            assert tr.dtype == np.int64 and np.array_equal(tr, golden[f"sel_train_s{seed}_n{shot}"])
            assert np.array_equal(va, golden[f"sel_val_s{seed}_n{shot}"])
            assert len(tr) == 5 * shot and len(va) == 5 * probe.VAL_SHOTS[shot]


def test_objective_is_stationary_at_the_stored_optimum(golden, banks):
    """max |grad (F / n)| of the objective in include/ppt_hip.h, evaluated in fp64 at sklearn's (polished) optimum: <= 1e-9 on all
    45 cases, i.e. the objective written there is the one sklearn minimises."""
    (Xtr, ytr), _ = banks
    worst = 0.0
    for si, seed in enumerate(SEEDS):
        for ni, shot in enumerate(SHOTS):
            sel = golden[f"sel_train_s{seed}_n{shot}"]
            for ci, c in enumerate(CS):
                worst = max(worst, R.grad_max(Xtr[sel], ytr[sel], golden["opt_W"][si, ni, ci], golden["opt_b"][si, ni, ci], c))
    print("worst max|grad(F/n)| at a stored optimum:", worst)
    assert worst <= 1e-9


def test_stored_predictions_are_the_optimums(golden, banks):
    _, (Xte, _) = banks
    for idx in np.ndindex(3, 5, 3):
        assert np.array_equal(R.predict(Xte, golden["opt_W"][idx], golden["opt_b"][idx]), golden["opt_pred"][idx])
    # the gap rule of the GPU test leaves at least 90 % of the bank to compare in every case
    assert max(R.gap_rows(Xte, golden["opt_W"][idx], golden["opt_b"][idx]).sum() for idx in np.ndindex(3, 5, 3)) <= 30


class TableFit:
    """a stand-in for the batched fit-and-score whose accuracies come from a table"""

    def __init__(self, grid, steps):
        self.grid, self.steps, self.calls = grid, steps, []

    def __call__(self, train_rows, val_rows, Cs):
        Cs = np.asarray(Cs)
        self.calls.append(Cs.copy())
        runs = Cs.shape[0]
        if Cs.shape[1] == 7:
            return np.tile(np.array(self.grid), (runs, 1)), np.zeros((runs, 7)), None
        left, right = self.steps[len(self.calls) - 2]
        step = len(self.calls) - 2
        test = np.array([[0.50 + 0.01 * step + 0.1 * r, 0.60 + 0.01 * step + 0.1 * r] for r in range(runs)])
        return np.tile(np.array([left, right]), (runs, 1)), test, None


def test_search_control_flow(banks, tmp_path):
    from ppt_amd import probe
    (Xtr, ytr), (Xte, yte) = banks
    fit = TableFit(grid=[0.2, 0.5, 0.5, 0.3, 0.5, 0.1, 0.0], steps=[(0.5, 0.5), (0.4, 0.6), (0.7, 0.6)])
    res = probe.linear_probe((Xtr, ytr), (Xte, yte), shots=(4,), num_run=2, num_step=3, fit=fit, out_dir=str(tmp_path))
    # the grid, then the first maximum (1e4, not the equal 1e2 or 1e-2) opens [1e3, 1e5]
    assert np.array_equal(fit.calls[0], np.tile(np.array(probe.SEARCH_LIST), (2, 1)))
    np.testing.assert_allclose(fit.calls[1], [[1e3, 1e5]] * 2, rtol=1e-12)
    # a tie keeps the left end: next [1e3, 1e4]; then right is strictly better: next [10^3.5, 1e4]
    np.testing.assert_allclose(fit.calls[2], [[1e3, 1e4]] * 2, rtol=1e-12)
    np.testing.assert_allclose(fit.calls[3], [[10 ** 3.5, 1e4]] * 2, rtol=1e-12)
    assert len(fit.calls) == 4
    for r in range(2):
        cs = [c for c, _ in res["steps"][4][r]]
        np.testing.assert_allclose(cs, [1e3, 1e4, 10 ** 3.5], rtol=1e-12)
        accs = [a for _, a in res["steps"][4][r]]
        np.testing.assert_allclose(accs, [50 + 10 * r, 61 + 10 * r, 52 + 10 * r], atol=1e-9)          # the kept end's test accuracy
    mean, std = res["summary"][4]
    assert abs(mean - 57.0) < 1e-9 and abs(std - 5.0) < 1e-9          # population std of (52, 62)
    # selections are select_shots', seed = run number
    for r in range(2):
        tr, va = probe.select_shots(ytr, yte, 4, r + 1)
        assert np.array_equal(res["selections"][4][r][0], tr) and np.array_equal(res["selections"][4][r][1], va)
    # the two files, in the reference's line formats (linear_probe.py:97, :116), seed by seed
    details = open(tmp_path / "mn40-run2-step3_details.txt").read().splitlines()
    assert details[0] == "modelnet40, seed 1, 4 shot, weight 1000.0, test_acc 50.00"
    assert details[3].startswith("modelnet40, seed 2, 4 shot, weight 1000.0, test_acc 60.00") and len(details) == 6
    assert open(tmp_path / "mn40-run2-step3.txt").read() == "modelnet40, 4 Shot, Test acc stat: 57.00 (5.00)\n"


def test_bank_files_round_trip(tmp_path):
    from ppt_amd import probe
    import torch
    feats = np.random.RandomState(3).randn(7, 5)
    labels = [3, 1, 4, 1, 5, 9, 2]
    # as the reference writes it (lp_feat_extractor.py:58-68): lists of Python floats -> float64, labels -> int64
    np.savez(str(tmp_path / "ref"), feature_list=[row.tolist() for row in feats], label_list=labels)
    f, l = probe.load_features(str(tmp_path / "ref.npz"))
    assert f.dtype == np.float32 and l.dtype == np.int64 and np.array_equal(f, feats.astype(np.float32)) and l.tolist() == labels
    # and back: what the reference's reader (linear_probe.py:15-19) takes out of a bank written here
    probe.save_features(str(tmp_path / "ours"), torch.from_numpy(f), torch.tensor(labels))
    with np.load(str(tmp_path / "ours.npz")) as z:
        assert sorted(z.files) == ["feature_list", "label_list"]
        assert np.array_equal(z["feature_list"], f) and np.array_equal(z["label_list"], labels)


def test_argument_checks_without_gpu():
    """host-side checks return before any launch: fake non-null pointers are never dereferenced"""
    from ppt_amd import _lib
    L = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, -3
    p = ctypes.c_void_p(0x1000)

    def fit(feat=p, labels=p, rows=p, F=2, n=10, d=16, K=5, C=(1.0, 0.5), W=p, b=p, info=p, ws=p, ws_bytes=1 << 30, ld=None, tol=1e-4):
        c = (ctypes.c_float * len(C))(*C) if C is not None else None
        return L.ppt_logreg_fit_f32(feat, d if ld is None else ld, 100, labels, rows, F, n, d, K, c, tol, 1000, W, b, info, ws, ws_bytes, None)

    for name in ("feat", "labels", "rows", "W", "b", "info", "ws", "C"):
        assert fit(**{name: None}) == EINVAL, name
    assert fit(K=1) == EUNSUPPORTED and fit(K=65, n=80) == EUNSUPPORTED and fit(d=1025) == EUNSUPPORTED
    assert fit(n=4) == EUNSUPPORTED and fit(n=1025) == EUNSUPPORTED                   # n < K, n > 1024
    assert fit(C=(1.0, 0.0)) == EINVAL and fit(C=(-1.0, 1.0)) == EINVAL
    assert fit(C=(1.0, float("inf"))) == EINVAL and fit(C=(float("nan"), 1.0)) == EINVAL
    assert fit(ld=15) == EINVAL and fit(F=0, C=()) == EINVAL and fit(tol=-1.0) == EINVAL
    assert fit(ws_bytes=1024) == EINVAL and fit(ws=ctypes.c_void_p(0x1010)) == EINVAL          # too small; not 256-byte aligned
    assert L.ppt_logreg_workspace_bytes(2, 10, 16, 5) > 0 and L.ppt_logreg_workspace_bytes(2, 10, 16, 65) == 0
    assert L.ppt_logreg_workspace_bytes(4, 640, 768, 40) == 2 * L.ppt_logreg_workspace_bytes(2, 640, 768, 40)

    def predict(feat=p, W=p, b=p, pred=p, n_eval=10, d=16, K=5, rows=p):
        return L.ppt_logreg_predict_f32(feat, d, 100, rows, n_eval, W, b, 2, d, K, pred, None)

    for name in ("feat", "W", "b", "pred"):
        assert predict(**{name: None}) == EINVAL, name
    assert predict(K=1) == EUNSUPPORTED and predict(K=65) == EUNSUPPORTED and predict(d=1025) == EUNSUPPORTED
    assert predict(n_eval=0) == EINVAL and predict(rows=None, n_eval=101) == EINVAL
