"""CPU: the restatement of tests/tsne_ref.py against itself (gradient vs finite differences of its own KL) and, where sklearn is
installed, against sklearn's joint probabilities; the stop rules, the pixel mapping and the palette of ppt_amd.tsne; the
host-side argument checks of the two t-SNE entry points; the payload round trip and the command line."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import tsne_ref as R
import viz_ref


def _case(N=60, D=8, K=4, perplexity=10.0):
    x, labels = R.blobs(N, D, K, seed=3)
    P, beta, done = R.affinities(x, perplexity)
    assert done.all()
    return x, labels, P


@pytest.mark.parametrize("scale", [1e-4, 5.0, 50.0])
def test_gradient_is_the_derivative_of_the_restatements_own_kl(scale, alpha=1.0):
    """g = d KL / d y by central differences in float64, at the three Y scales a run passes through, for alpha = 1 (with
    exaggeration sklearn's g, and the statement's, is not the derivative of KL_t: the repulsive term keeps the factor 1 where
    sum alpha P = alpha would put alpha).  KL's second derivative is O(1) (the weights w and their derivatives are bounded by
    1), so with h = 1e-6 * max(scale, 1) the truncation error is far below the 1e-6 relative tolerance asked here; the rounding
    error of the difference is ~1e-16 * KL / h."""
    _, _, P = _case()
    Y = np.random.RandomState(5).standard_normal((P.shape[0], 2)) * scale
    g = R.pair_pass(P, Y, alpha)["g"]
    h = 1e-6 * max(scale, 1.0)
    fd = np.zeros_like(g)
    for i in range(0, P.shape[0], 7):
        for k in range(2):
            Yp, Ym = Y.copy(), Y.copy()
            Yp[i, k] += h
            Ym[i, k] -= h
            fd[i, k] = (R.pair_pass(P, Yp, alpha)["kl"] - R.pair_pass(P, Ym, alpha)["kl"]) / (2 * h)
    rows = np.arange(0, P.shape[0], 7)
    err = np.abs(fd[rows] - g[rows]).max()
    ref = np.abs(g[rows]).max()
    print(f"TSNE fd scale {scale} alpha {alpha}: max |fd - g| {err:.3e} of max |g| {ref:.3e}")
    assert err <= 1e-6 * ref + 1e-9 * alpha / max(scale, 1.0)


def test_restatement_affinities_properties():
    x, _, P = _case()
    assert np.array_equal(P, P.T) and (np.diag(P) == 0).all() and abs(P.sum() - 1) < 1e-12
    d32 = R.sqdist(x, np.float32)
    assert d32.dtype == np.float32 and np.array_equal(d32, d32.T) and (np.diag(d32) == 0).all()
    xd, _ = R.blobs(96, 40, 4, seed=2, duplicates=True)
    dd = R.sqdist(xd, np.float32)
    assert (dd[np.arange(12), np.arange(84, 96)] == 0).all()            # a duplicate row is at distance exactly 0
    assert set(R.duplicate_rows(96)) == set(range(12)) | set(range(84, 96))
    xs, _ = R.blobs(50, 8, 4, seed=3, scale=50.0)
    Ps, _, done = R.affinities(xs, 10.0)
    assert done.all() and np.isfinite(Ps).all() and abs(Ps.sum() - 1) < 1e-12   # the minimum is subtracted: no underflow to 0 / 0


def test_sklearn_joint_probabilities_agree_with_the_restatement():
    """sklearn's _joint_probabilities on fp32 squared distances against the fp64 restatement.  Both searches stop anywhere
    inside |H - log(perplexity)| <= 1e-5.  dH / dbeta = -beta Var_p(e) and d log p_{j|i} / dbeta = -(e_ij - E_p e), so two
    betas inside the band differ by at most 2e-5 / (beta Var_p(e)) and the conditionals by p |e_ij - E_p e| times that; on top
    come the fp32 distances (gamma_D = (D + 2) 2^-24 on each, through beta d: beta (d_ij + m_i) gamma_D on log p, twice for the
    normalising sum), sklearn's fp32 storage (2^-24 relative, a few times) and its floor at machine epsilon."""
    pytest.importorskip("sklearn")
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne
    x, _ = R.blobs(120, 16, 4, seed=7)
    perplexity = 15.0
    d32 = R.sqdist(x, np.float32)
    got = squareform(_t_sne._joint_probabilities(d32, perplexity, 0)).astype(np.float64)
    d = R.sqdist(x)
    e, m = R.shifted(d)
    beta, done = R.search(e, perplexity)
    assert done.all()
    cond = R.conditionals(e, beta)
    mean_e = (cond * e).sum(axis=1)
    var_e = (cond * (e - mean_e[:, None]) ** 2).sum(axis=1)
    slack_beta = 2e-5 / (beta * var_e)
    gamma = (x.shape[1] + 2) * R.EPS32
    rel = np.abs(e - mean_e[:, None]) * slack_beta[:, None] + 2 * beta[:, None] * (d + m[:, None]) * gamma + 8 * R.EPS32
    bound = (cond * rel + (cond * rel).T) / (2 * x.shape[0]) + 3e-16
    err = np.abs(got - R.joint(cond))
    print(f"TSNE sklearn P: worst |dP| / bound {np.max(err / bound):.3f}, max relative slack {rel.max():.2e}")
    assert (err <= bound).all()


def test_stop_rules_on_hand_made_sequences():
    from ppt_amd.tsne import check_spans, stop_check
    inf = float("inf")
    # progress at every check: never stops
    best, it = inf, 0
    for i, kl in zip(range(49, 1000, 50), np.linspace(3.0, 1.0, 19)):
        reason, best, it = stop_check(i, kl, 1e-3, best, it, 300, 1e-7)
        assert reason is None and it == i
    # no progress after iteration 49: the check at 399 is 350 > 300 iterations past the best one (349, at 300, is not)
    best, it, out = inf, 0, []
    for i in range(49, 450, 50):
        reason, best, it = stop_check(i, 2.0 if i <= 99 else 2.5, 1e-3, best, it, 300, 1e-7)
        out.append(reason)
    assert best == 2.0 and it == 49                        # an equal error is no progress: the first one stays the best
    assert out == [None] * 7 + ["no_progress", "no_progress"]
    # the exploration stage's patience of 250 cannot fire inside 250 iterations
    best, it = inf, 0
    for i in range(49, 250, 50):
        reason, best, it = stop_check(i, 5.0, 1.0, best, it, 250, 1e-7)
        assert reason is None
    # the gradient norm stops at or below the threshold, also on an iteration that made progress
    assert stop_check(49, 1.0, 1e-7, inf, 0, 300, 1e-7)[0] == "grad_norm"
    assert stop_check(49, 1.0, 1.1e-7, inf, 0, 300, 1e-7)[0] is None
    assert stop_check(99, float("nan"), 1.0, 1.0, 49, 300, 1e-7)[0] is None          # a NaN error is no progress, not a stop by itself
    assert check_spans(0, 250, 50) == [(0, 50, True), (50, 50, True), (100, 50, True), (150, 50, True), (200, 50, True)]
    assert check_spans(250, 330, 50) == [(250, 50, True), (300, 30, False)]
    assert check_spans(120, 260, 100) == [(120, 80, True), (200, 60, False)]
    assert check_spans(0, 300, 0) == [(0, 300, False)] and check_spans(5, 5, 50) == []


def test_helpers_of_the_host_side():
    from ppt_amd import tsne as T
    assert T.auto_learning_rate(2468, 12.0) == 2468 / 12.0 / 4.0 and T.auto_learning_rate(300, 12.0) == 50.0
    y = T.random_init(37, 4)
    assert y.dtype == np.float32 and y.shape == (37, 2) and np.array_equal(y, R.random_init(37, 4)) and 0 < np.abs(y).max() < 1e-3
    assert not np.array_equal(y, T.random_init(37, 5))
    f = T.features_f32(np.arange(12, dtype=np.float64).reshape(4, 3)[:, ::-1])
    assert f.dtype == torch.float32 and f.is_contiguous() and f.shape == (4, 3) and f[0].tolist() == [2.0, 1.0, 0.0]
    assert T.features_f32(torch.ones(3, 2, dtype=torch.float16)).dtype == torch.float32
    with pytest.raises(ValueError):
        T.features_f32(np.zeros((3, 2), np.int64))
    with pytest.raises(ValueError):
        T.features_f32(np.zeros(5))


@pytest.mark.parametrize("size,n", [(96, 257), (1000, 40), (64, 1)])
def test_pixel_mapping_on_cpu_tensors_equals_numpy(size, n):
    """every coordinate equal, except where the float64 value lies within 1e-9 of an integer (either neighbour passes)"""
    from ppt_amd import tsne as T
    Y = (np.random.RandomState(size).standard_normal((n, 2)) * [30.0, 11.0]).astype(np.float32)
    want, values = R.scatter_pixels(Y, size)
    band = viz_ref.in_band(values)
    got = T.scatter_pixels(torch.from_numpy(Y), size)
    assert got.dtype == torch.int32 and got.shape == (n, 3) and not got.is_cuda
    got = got.numpy()
    assert not ((got != want) & ~band).any() and (np.abs(got - want) <= 1).all()
    assert (got[:, 2] == 0).all()
    lo, hi = int(0.05 * (size - 1)), int(np.ceil(0.95 * (size - 1)))
    assert got[:, :2].min() >= lo and got[:, :2].max() <= hi                     # inside the margin
    if n > 1:
        assert got[np.argmax(Y[:, 1]), 0] == got[:, 0].min()                     # y points upwards: the largest y is the top row
        assert got[np.argmax(Y[:, 0]), 1] == got[:, 1].max()                     # x -> column
        assert got[:, 1].max() - got[:, 1].min() > got[:, 0].max() - got[:, 0].min()    # one scale: the wider axis stays wider
    with pytest.raises(ValueError):
        T.scatter_pixels(torch.zeros(4, 3), size)


@pytest.mark.parametrize("n", [1, 15, 40, 300])
def test_class_palette_is_distinct_for_any_class_count(n):
    from ppt_amd import tsne as T
    pal = T.class_palette(n)
    assert pal.dtype == torch.float32 and pal.shape == (n, 3) and pal.min() >= 0 and pal.max() <= 255
    assert len({tuple(row) for row in pal.tolist()}) == n
    assert torch.equal(pal, T.class_palette(300)[:n])                           # a class keeps its colour when classes are added


def test_argument_validation_without_gpu():
    """NULL pointers, non-positive sizes, bad strides and short workspaces return PPT_EINVAL before any launch; shapes outside
    the limits return PPT_EUNSUPPORTED and a zero workspace"""
    from ppt_amd import _lib, ops
    L = _lib.lib()
    buf = ctypes.create_string_buffer(8192)
    p = (ctypes.addressof(buf) + 255) & ~255               # a non-NULL, aligned address that is never dereferenced
    big = 1 << 20
    #                        x  ld  N   D  perp  P  ldp beta pstats ws bytes stream
    A = L.ppt_tsne_affinities
    assert A(None, 8, 16, 8, 5.0, p, 16, p, p, p, big, None) == -1
    assert A(p, 8, 16, 8, 5.0, None, 16, p, p, p, big, None) == -1
    assert A(p, 8, 16, 8, 5.0, p, 16, None, p, p, big, None) == -1
    assert A(p, 8, 16, 8, 5.0, p, 16, p, None, p, big, None) == -1
    assert A(p, 8, 16, 8, 5.0, p, 16, p, p, None, big, None) == -1
    assert A(p, 8, 0, 8, 5.0, p, 16, p, p, p, big, None) == -1                  # N = 0
    assert A(p, 8, 16, 0, 5.0, p, 16, p, p, p, big, None) == -1                 # D = 0
    assert A(p, 7, 16, 8, 5.0, p, 16, p, p, p, big, None) == -1                 # ld < D
    assert A(p, 8, 16, 8, 5.0, p, 12, p, p, p, big, None) == -1                 # ldp < N
    assert A(p, 8, 18, 8, 5.0, p, 18, p, p, p, big, None) == -1                 # ldp % 4 != 0
    assert A(p, 8, 16, 8, 0.0, p, 16, p, p, p, big, None) == -1                 # perplexity = 0
    assert A(p, 8, 16, 8, float("nan"), p, 16, p, p, p, big, None) == -1
    assert A(p, 8, 16, 8, 5.0, p + 4, 16, p, p, p, big, None) == -1             # P misaligned
    assert A(p, 8, 16, 8, 5.0, p, 16, p, p, p, 0, None) == -1                   # short workspace
    assert A(p, 8, 1, 8, 5.0, p, 4, p, p, p, big, None) == -3                   # N < 2
    assert A(p, 8, 16385, 8, 5.0, p, 16388, p, p, p, big, None) == -3           # N > 16384
    assert A(p, 4097, 16, 4097, 5.0, p, 16, p, p, p, big, None) == -3           # D > 4096
    assert L.ppt_tsne_affinities_workspace_bytes(1, 8) == 0 and L.ppt_tsne_affinities_workspace_bytes(16385, 8) == 0
    assert L.ppt_tsne_affinities_workspace_bytes(16, 0) == 0 and L.ppt_tsne_affinities_workspace_bytes(16, 4097) == 0
    assert L.ppt_tsne_affinities_workspace_bytes(2, 1) == 256 and L.ppt_tsne_affinities_workspace_bytes(2468, 40) == 97536
    assert ops.tsne_affinities_workspace_bytes(16384, 4096) == 512 * 512 * 16
    #                   P ldp pstats N  y update gains t0 n  t_switch ee   lr    check stats rows grad ws bytes stream
    S = L.ppt_tsne_steps
    assert S(None, 16, p, 16, p, p, p, 0, 1, 250, 12.0, 50.0, 0, None, 0, None, p, big, None) == -1
    assert S(p, 16, None, 16, p, p, p, 0, 1, 250, 12.0, 50.0, 0, None, 0, None, p, big, None) == -1
    assert S(p, 16, p, 16, None, p, p, 0, 1, 250, 12.0, 50.0, 0, None, 0, None, p, big, None) == -1
    assert S(p, 16, p, 16, p, None, p, 0, 1, 250, 12.0, 50.0, 0, None, 0, None, p, big, None) == -1
    assert S(p, 16, p, 16, p, p, None, 0, 1, 250, 12.0, 50.0, 0, None, 0, None, p, big, None) == -1
    assert S(p, 16, p, 16, p, p, p, 0, 1, 250, 12.0, 50.0, 0, None, 0, None, None, big, None) == -1
    assert S(p, 16, p, 0, p, p, p, 0, 1, 250, 12.0, 50.0, 0, None, 0, None, p, big, None) == -1            # N = 0
    assert S(p, 12, p, 16, p, p, p, 0, 1, 250, 12.0, 50.0, 0, None, 0, None, p, big, None) == -1           # ldp < N
    assert S(p, 16, p, 16, p, p, p, -1, 1, 250, 12.0, 50.0, 0, None, 0, None, p, big, None) == -1          # t0 < 0
    assert S(p, 16, p, 16, p, p, p, 0, 0, 250, 12.0, 50.0, 0, None, 0, None, p, big, None) == -1           # n = 0
    assert S(p, 16, p, 16, p, p, p, 0, 1, 250, 12.0, 0.0, 0, None, 0, None, p, big, None) == -1            # lr = 0
    assert S(p, 16, p, 16, p, p, p, 0, 1, 250, 0.0, 50.0, 0, None, 0, None, p, big, None) == -1            # exaggeration = 0
    assert S(p, 16, p, 16, p, p, p, 0, 1, 250, 12.0, 50.0, -1, None, 0, None, p, big, None) == -1          # check_every < 0
    assert S(p, 16, p, 16, p, p, p, 0, 50, 250, 12.0, 50.0, 50, None, 0, None, p, big, None) == -1         # a check, no stats
    assert S(p, 16, p, 16, p, p, p, 0, 100, 250, 12.0, 50.0, 50, p, 1, None, p, big, None) == -1           # two checks, one row
    assert S(p, 16, p, 16, p, p, p, 0, 1, 250, 12.0, 50.0, 0, None, 0, None, p, 0, None) == -1             # short workspace
    assert S(p, 16, p, 16, p + 4, p, p, 0, 1, 250, 12.0, 50.0, 0, None, 0, None, p, big, None) == -1       # y misaligned
    assert S(p, 4, p, 1, p, p, p, 0, 1, 250, 12.0, 50.0, 0, None, 0, None, p, big, None) == -3             # N < 2
    assert S(p, 16388, p, 16385, p, p, p, 0, 1, 250, 12.0, 50.0, 0, None, 0, None, p, big, None) == -3     # N > 16384
    assert L.ppt_tsne_steps_workspace_bytes(1) == 0 and L.ppt_tsne_steps_workspace_bytes(16385) == 0
    assert L.ppt_tsne_steps_workspace_bytes(2) == 768 and ops.tsne_steps_workspace_bytes(2468) == 39680 + 2 * 9984


def test_tsne_has_no_cpu_path():
    from ppt_amd import ops, tsne as T
    y = torch.zeros(8, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.tsne_affinities(torch.zeros(8, 4), 3.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.tsne_steps(torch.zeros(8, 8), torch.zeros(2, dtype=torch.float64), y, y.clone(), y.clone(), 0, 1, lr=50.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        T.feature_scatter(torch.zeros(8, 2), torch.zeros(8, dtype=torch.int64), size=32, radius=2)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            T.tsne(np.zeros((8, 4), np.float32), perplexity=3.0)
    with pytest.raises(ValueError):
        T.feature_scatter(torch.zeros(8, 2), torch.zeros(7, dtype=torch.int64))
    with pytest.raises(ValueError):
        T.feature_scatter(torch.zeros(2, 2), torch.tensor([0, 3]), palette=[(1, 2, 3)] * 3)


def test_command_line_flags_parse():
    from ppt_amd import analysis
    ap = argparse.ArgumentParser()
    analysis.tsne_parser(ap.add_subparsers(dest="command", required=True))
    a = ap.parse_args(["tsne", "--feats", "feats.pt", "--out", "mn40_feats.png"])
    assert (a.command, a.feats, a.out, a.coords, a.perplexity, a.n_iter, a.seed, a.size, a.radius) == \
        ("tsne", "feats.pt", "mn40_feats.png", None, 30.0, 1000, 0, 1000, 6)
    a = ap.parse_args(["tsne", "--feats", "f.pt", "--out", "o.png", "--coords", "y.npz", "--perplexity", "12.5", "--n_iter", "500",
                       "--seed", "3", "--size", "640", "--radius", "4"])
    assert (a.coords, a.perplexity, a.n_iter, a.seed, a.size, a.radius) == ("y.npz", 12.5, 500, 3, 640, 4)
    with pytest.raises(SystemExit):
        ap.parse_args(["tsne", "--out", "o.png"])


def test_payload_round_trip_into_the_input_conversion(tmp_path):
    """save_recog_feats -> load_recog_feats -> features_f32: the float64 payload holds the fp32 logits exactly"""
    from ppt_amd import analysis, tsne as T
    logits = torch.from_numpy(np.random.RandomState(1).standard_normal((33, 15)).astype(np.float32) * 40)
    labels = torch.arange(33) % 15
    path = str(tmp_path / "feats.pt")
    analysis.save_recog_feats(path, logits, labels, [f"c{int(i)}" for i in labels])
    feats, lab, names = analysis.load_recog_feats(path)
    assert feats.dtype == np.float64 and feats.shape == (33, 15) and lab.dtype == np.int64 and np.array_equal(lab, labels.numpy())
    assert names.shape == (33,) and names[4] == "c4"
    x = T.features_f32(feats)
    assert x.dtype == torch.float32 and torch.equal(x, logits)
    torch.save({"test_feats": feats, "test_labels": lab[:-1]}, path)
    with pytest.raises(ValueError):
        analysis.load_recog_feats(path)
