"""GPU: csrc/tsne.hip and ppt_amd/tsne.py against the float64 restatement of tests/tsne_ref.py -- the affinities, the pair pass,
the update step bit for bit, a short trajectory, determinism, the whole run against sklearn's recorded embeddings
(tests/golden/g_tsne.npz, written by tests/golden/make_golden_tsne.py) and the scatter picture.  Figures measured on an MI355X
are in profiles/r20_tsne.md."""
import functools
import os

import numpy as np
import pytest
import torch

import tsne_ref as R
import viz_ref

pytestmark = pytest.mark.gpu

EPS = R.EPS32
SENTINEL = 7.5                                             # what the padding columns of P hold before the call

# (N, D, perplexity, K, variant)
AFFINITY_CASES = {
    "tiny": (5, 3, 2.0, 2, "plain"),
    "odd": (67, 40, 5.0, 5, "plain"),
    "two_tiles": (257, 40, 30.0, 5, "plain"),
    "wide_rows": (130, 513, 30.0, 5, "wide"),             # D = 513 in rows of 516 (NaN padding): the vector path and its scalar tail
    "many_rows": (1030, 15, 30.0, 15, "plain"),           # more than 256 rows per thread stride, 33 tiles
    "logit_scale": (257, 40, 30.0, 5, "scaled"),
    "duplicates": (96, 40, 10.0, 4, "duplicates"),
    "padded_rows": (67, 40, 5.0, 5, "padded"),             # ld > D, the padding NaN: the scalar path (ld % 4 != 0)
}
TAU_MARGIN = 4.0


def _input(name):
    N, D, perplexity, K, variant = AFFINITY_CASES[name]
    x, _ = R.blobs(N, D, K, seed=11, scale=50.0 if variant == "scaled" else 1.0, duplicates=variant == "duplicates")
    return x, perplexity, variant


@functools.lru_cache(maxsize=None)
def _ref64(name):
    """the float64 side of a case, computed once: distances, their shift, and which rows the fp64 search converges on"""
    x, perplexity, _ = _input(name)
    d = R.sqdist(x)
    e, m = R.shifted(d)
    _, done = R.search(e, perplexity)
    return d, e, m, done


@functools.lru_cache(maxsize=None)
def _tau():
    """The allowance for evaluating H in fp32: the restatement run in float32 on every case, its entropy (fp32 distances, fp32
    sums) against the float64 entropy at the SAME beta; the worst converged row of all cases, times TAU_MARGIN.  Nothing of the
    kernel's output enters."""
    worst = 0.0
    for name in AFFINITY_CASES:
        x, perplexity, _ = _input(name)
        e32, _ = R.shifted(R.sqdist(x, np.float32))
        beta32, done32 = R.search(e32, perplexity, np.float32)
        H32, _, _ = R.entropy_rows(e32, beta32, np.float32)
        H64, _, _ = R.entropy_rows(_ref64(name)[1], beta32.astype(np.float64))
        rows = done32 & _ref64(name)[3]
        worst = max(worst, float(np.abs(H32.astype(np.float64) - H64)[rows].max()))
    return TAU_MARGIN * worst, worst


def _device_affinities(x, perplexity, ld=None):
    from ppt_amd import ops
    N, D = x.shape
    if ld is None:
        xd = torch.from_numpy(x).cuda()
    else:
        bank = torch.full((N, ld), float("nan"), dtype=torch.float32, device="cuda")
        bank[:, :D] = torch.from_numpy(x).cuda()
        xd = bank[:, :D]
    ldp = ((N + 3) & ~3) + 4
    buf = torch.full((N, ldp), SENTINEL, dtype=torch.float32, device="cuda")
    P, beta, pstats = ops.tsne_affinities(xd, perplexity, P=buf[:, :N])
    torch.cuda.synchronize()
    return buf.cpu().numpy(), beta.cpu().numpy(), pstats.cpu().numpy()


@pytest.mark.parametrize("name", list(AFFINITY_CASES))
def test_affinities(name):
    """P, beta and the sums of ppt_tsne_affinities against float64.

    Structure: P == P^T bit for bit, a zero diagonal, padding columns untouched.
    Sum: sum_j p_{j|i} = (sum_j q_ij) / (float)S_i; S_i carries the fp32 partial sums of ceil(N / 256) terms per thread and its
    rounding to fp32, every quotient one rounding, the symmetrisation an addition and a division: |sum P - 1| <= (ceil(N / 256) +
    5) 2^-24 (summed here in float64).
    Entropy: the float64 entropy of the float64 conditional row at the kernel's beta_i lies within 1e-5 + tau of log(perplexity);
    tau: _tau().  Rows are exempt only where the float64 restatement itself runs out of its 100 steps, and these are rows of
    the designed duplicates.
    P: against the float64 joint built from the kernel's beta.  With eps = 2^-24 and gamma_D = (D + 2) eps the bound of a fp32
    distance (subtraction, square: 3 eps per term; D - 1 additions), e_ij = d_ij - m_i carries gamma_D (d_ij + m_i) + eps e_ij,
    the product beta e one more eps: the exponent is off by Delta_ij = beta_i (gamma_D (d_ij + m_i) + 2 eps e_ij), q_ij by the
    factor exp(+-Delta_ij) (1 +- 2 eps) (expf: 1 ulp).  The normalising sum inherits the q-weighted mean of that plus its own
    summation, E_i = sum_j q_ij (Delta_ij + 2 eps) / S_i + (ceil(N / 256) + 1) eps, the quotient one eps:
    p_{j|i} is off by the relative r_ij = Delta_ij + E_i + 3 eps, and
        |P32_ij - P64_ij| <= 1.01 (p_{j|i} r_ij + p_{i|j} r_ji) / 2N + 2 eps P64_ij + 2^-126
    (1.01: the second-order terms, Delta <= 1e-2 here; 2 eps: the addition and the division; 2^-126: fp32 underflow)."""
    x, perplexity, variant = _input(name)
    N, D = x.shape
    buf, beta, pstats = _device_affinities(x, perplexity, ld={"padded": D + 3, "wide": (D + 3) & ~3}.get(variant))
    P = buf[:, :N]
    assert (buf[:, N:] == SENTINEL).all(), "padding columns of P were written"
    assert np.isfinite(P).all() and (P >= 0).all()
    assert np.array_equal(P, P.T), "P is not symmetric bit for bit"
    assert (np.diag(P) == 0).all()
    total = P.astype(np.float64).sum()
    sum_bound = (-(-N // 256) + 5) * EPS
    print(f"TSNE affinities {name}: |sum P - 1| = {abs(total - 1):.2e} (bound {sum_bound:.2e})")
    assert abs(total - 1) <= sum_bound
    assert abs(pstats[0] - total) <= 1e-12
    pos = P > 0
    plogp = (P[pos].astype(np.float64) * np.log(P[pos].astype(np.float64)))
    assert abs(pstats[1] - plogp.sum()) <= 4 * EPS * np.abs(plogp).sum() + 1e-12           # logf (1 ulp) and the fp32 product

    d, e, m, done = _ref64(name)
    exempt = ~done
    if variant == "duplicates":
        assert set(np.flatnonzero(exempt)) <= set(R.duplicate_rows(N))
    else:
        assert not exempt.any()
    beta64 = beta.astype(np.float64)
    assert (beta > 0).all() and np.isfinite(beta).all()
    H, S, q = R.entropy_rows(e, beta64)
    tau, tau_raw = _tau()
    dev = np.abs(H - np.log(perplexity))
    worst = int(np.argmax(np.where(exempt, 0, dev)))
    print(f"TSNE affinities {name}: worst |H - log perplexity| = {dev[worst]:.3e} at row {worst} (1e-5 + tau, tau = {tau:.3e} = "
          f"{TAU_MARGIN} x {tau_raw:.3e}); exempt rows {int(exempt.sum())}")
    assert (dev[~exempt] <= 1e-5 + tau).all()

    gamma = (D + 2) * EPS
    delta = beta64[:, None] * (gamma * (d + m[:, None]) + 2 * EPS * e)
    np.fill_diagonal(delta, 0)
    E = (q * (delta + 2 * EPS)).sum(axis=1) / S + (-(-N // 256) + 1) * EPS
    cond = q / S[:, None]
    rel = delta + E[:, None] + 3 * EPS
    P64 = R.joint(cond)
    bound = 1.01 * (cond * rel + (cond * rel).T) / (2 * N) + 2 * EPS * P64 + 2.0 ** -126
    err = np.abs(P.astype(np.float64) - P64)
    ratio = err / bound
    i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"TSNE affinities {name}: worst |P32 - P64| / bound = {ratio[i, j]:.3f} at ({i}, {j}); max Delta {delta.max():.2e}, "
          f"max relative error {np.max(err[P64 > 1e-30] / P64[P64 > 1e-30]):.2e}")
    assert delta.max() <= 1e-2
    assert (err <= bound).all()


# ---- the pair pass --------------------------------------------------------------------------------------------------------------
ROUNDINGS = 48


@functools.lru_cache(maxsize=None)
def _pair_P(N):
    """the float64 restatement's P, rounded to fp32 once: the kernel and the judge read the same numbers"""
    if N == 2:
        return np.array([[0.0, 0.5], [0.5, 0.0]], np.float32)
    x, _ = R.blobs(N, 40, 5, seed=N)
    P, _, _ = R.affinities(x, min(30.0, (N - 1) / 3.0))
    return P.astype(np.float32)


def _pair_Y(N, kind):
    rng = np.random.RandomState(N + 1)
    Y = rng.standard_normal((N, 2))
    if kind == "coincident":
        Y = Y * 5.0
        Y[N - 1] = Y[0]
        return Y.astype(np.float32)
    return (Y * {"init": 1e-4, "mid": 5.0, "late": 50.0}[kind]).astype(np.float32)


def _device_P(P32):
    """a host P on the device as ppt_tsne_steps takes it: rows padded to a multiple of four, sum P and sum P log P in double"""
    N = P32.shape[0]
    Pd = torch.zeros((N, (N + 3) & ~3), dtype=torch.float32, device="cuda")
    Pd[:, :N] = torch.from_numpy(P32).cuda()
    P64 = P32.astype(np.float64)
    pos = P64 > 0
    return Pd[:, :N], torch.tensor([P64.sum(), (P64[pos] * np.log(P64[pos])).sum()], dtype=torch.float64, device="cuda")


def _one_step(P32, Y32, alpha, t0=0, t_switch=250, lr=50.0, update=None, gains=None):
    """one iteration on the device with a check -> dict(grad, Z, kl, norm, y, update, gains)"""
    from ppt_amd import ops
    N = P32.shape[0]
    Pd, pstats = _device_P(P32)
    y = torch.from_numpy(Y32).cuda().clone()
    upd = torch.zeros_like(y) if update is None else torch.from_numpy(update).cuda()
    gn = torch.ones_like(y) if gains is None else torch.from_numpy(gains).cuda()
    grad, stats = torch.zeros_like(y), torch.zeros((1, 2), dtype=torch.float32, device="cuda")
    ws = torch.zeros(ops.tsne_steps_workspace_bytes(N), dtype=torch.uint8, device="cuda")
    ops.tsne_steps(Pd, pstats, y, upd, gn, t0, 1, t_switch=t_switch, early_exaggeration=alpha if t0 < t_switch else 12.0, lr=lr,
                   check_every=1, stats=stats, grad=grad, workspace=ws)
    torch.cuda.synchronize()
    z_off = (N * 16 + 255) & ~255
    zrow = ws[z_off:z_off + 4 * N].cpu().numpy().view(np.float32)
    return dict(grad=grad.cpu().numpy(), Z=zrow.astype(np.float64).sum(), kl=float(stats[0, 0]), norm=float(stats[0, 1]),
                y=y.cpu().numpy(), update=upd.cpu().numpy(), gains=gn.cpu().numpy())


@pytest.mark.parametrize("kind", ["init", "mid", "late", "coincident"])
@pytest.mark.parametrize("alpha", [1.0, 12.0])
@pytest.mark.parametrize("N", [2, 67, 257, 1030])
def test_pair_pass(N, alpha, kind):
    """grad, Z, KL_t and ||g|| of one iteration against float64, P and Y being the same fp32 numbers on both sides.

    Per row and component |g32_i - g64_i| <= 4 gamma_N (alpha sum_j P_ij w_ij |y_i - y_j| + sum_j w_ij^2 |y_i - y_j| / Z),
    gamma_N = (N + c) 2^-24 with c = 48.  Per term: 1 + d^2 carries 5 roundings (dx or dy 1, its square 2 + 1, the sum 1, the
    + 1 one more; all terms positive), w = v_rcp_f32 of it (1 ulp = 2) 7; an attractive term (P w) dx 7 + 1 + 2 = 10; a
    repulsive term (w w) dx 14 + 1 + 2 = 17; Z, the same for every row, the 7 of w; 1 / Z rounded to fp32, the product with
    it, alpha a and the subtraction 4 more: at most 17 + 7 + 4 = 28.  Summation: a lane adds at most N / 64 + 3 terms in
    sequence, then six butterfly steps, N / 64 + 9 per row sum, and the repulsive side carries two of them (r_i and Z):
    28 + 18 + N / 32 <= N + 48 for every N.  Z is a sum of positive terms: gamma_N Z.  KL_t = alpha (sum P log P
    + sum P (log alpha + log Z) + sum P log(1 + d^2)): the last sum carries per term the 5 roundings of 1 + d^2 (absolute, on the
    logarithm), logf (1 ulp) and a product, and its summation; log Z the error of Z:
        |KL32 - KL64| <= alpha gamma_N (sum P (|log(1 + d^2)| + 2) + sum |P log P|) + 2 eps |KL|   (the last: stored as fp32).
    | ||g32|| - ||g64|| | <= || bound || + 2 eps ||g||."""
    P32 = _pair_P(N)
    Y32 = _pair_Y(N, kind)
    out = _one_step(P32, Y32, alpha)
    ref = R.pair_pass(P32, Y32, alpha)
    gamma = (N + ROUNDINGS) * EPS
    bound = 4 * gamma * (ref["attr_abs"] + ref["rep_abs"])
    err = np.abs(out["grad"].astype(np.float64) - ref["g"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    i, k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    P64 = P32.astype(np.float64)
    diff = Y32.astype(np.float64)[:, None, :] - Y32.astype(np.float64)[None, :, :]
    logdd = np.log((diff ** 2).sum(-1) + 1)
    pos = P64 > 0
    kl_bound = alpha * gamma * ((P64 * (np.abs(logdd) + 2)).sum() + np.abs(P64[pos] * np.log(P64[pos])).sum()) + 2 * EPS * abs(ref["kl"])
    norm_bound = np.sqrt((bound ** 2).sum()) + 2 * EPS * ref["norm"]
    print(f"TSNE pair N={N} alpha={alpha} {kind}: worst |dg| / bound = {ratio[i, k]:.4f} at ({i}, {k}) [c = {ROUNDINGS}]; "
          f"|dZ| / bound = {abs(out['Z'] - ref['Z']) / (gamma * ref['Z']):.4f}; |dKL| / bound = {abs(out['kl'] - ref['kl']) / kl_bound:.4f} "
          f"(KL {ref['kl']:.5f}); |dnorm| / bound = {abs(out['norm'] - ref['norm']) / max(norm_bound, 1e-300):.4f}")
    assert np.isfinite(out["grad"]).all()
    assert (err <= bound).all()
    assert abs(out["Z"] - ref["Z"]) <= gamma * ref["Z"]
    assert abs(out["kl"] - ref["kl"]) <= kl_bound
    assert abs(out["norm"] - ref["norm"]) <= norm_bound


@pytest.mark.parametrize("t0,mu", [(0, 0.5), (300, 0.8)])
def test_update_is_the_numpy_step_bit_for_bit(t0, mu):
    """given the kernel's own grad, one step's gains, update and y equal the fp32 numpy restatement bit for bit, in both
    momentum stages, from a state where some gains sit at the 0.01 floor and others fall onto it"""
    N, lr = 257, 53.25
    P32 = _pair_P(N)
    rng = np.random.RandomState(9)
    Y32 = (rng.standard_normal((N, 2)) * 5).astype(np.float32)
    update = (rng.standard_normal((N, 2)) * 0.3).astype(np.float32)
    gains = rng.choice(np.asarray([0.01, 0.0125, 0.012, 1.0, 2.6, 0.8], np.float32), size=(N, 2)).astype(np.float32)
    update[::17] = 0                                       # update * g == 0: not an increase
    out = _one_step(P32, Y32, 12.0, t0=t0, lr=lr, update=update.copy(), gains=gains.copy())
    y, upd, gn = R.descent_step(out["grad"], Y32, update, gains, mu, lr, np.float32)
    assert np.array_equal(out["gains"].view(np.uint32), gn.view(np.uint32))
    assert np.array_equal(out["update"].view(np.uint32), upd.view(np.uint32))
    assert np.array_equal(out["y"].view(np.uint32), y.view(np.uint32))
    assert (gn == np.float32(0.01)).sum() >= 20 and (gn > 1).any()          # the floor was exercised, and so was the + 0.2 branch


# ---- a short trajectory ---------------------------------------------------------------------------------------------------------
E2E_CASES = {"a": dict(N=300, D=40, K=6, perplexity=30.0, seed=0), "b": dict(N=257, D=40, K=5, perplexity=10.0, seed=1)}
TRAJECTORY_MARGIN = 4.0


@functools.lru_cache(maxsize=None)
def _e2e(name):
    c = E2E_CASES[name]
    x, labels = R.blobs(c["N"], c["D"], c["K"], c["seed"])
    P64, _, done = R.affinities(x, c["perplexity"])
    assert done.all()
    return x, labels, P64


@pytest.mark.parametrize("name", list(E2E_CASES))
def test_short_trajectory(name):
    """10 iterations from the same Y0 and the same fp32 P: max |Y_dev - Y_64| / max |Y_64| against the same figure of the fp32
    numpy restatement, times a margin for the different summation order (TRAJECTORY_MARGIN; the measured ratios are in
    profiles/r20_tsne.md).  No longer horizon: the fp32 and fp64 runs part company before iteration 50."""
    from ppt_amd import ops
    x, _, P64 = _e2e(name)
    N = x.shape[0]
    P32 = P64.astype(np.float32)
    Y0, lr = R.random_init(N, 0), R.auto_learning_rate(N)
    Y64 = R.run(P32, Y0, 10, lr)
    Ynp = R.run(P32, Y0, 10, lr, dtype=np.float32)
    Pd, pstats = _device_P(P32)
    y = torch.from_numpy(Y0).cuda().clone()
    ops.tsne_steps(Pd, pstats, y, torch.zeros_like(y), torch.ones_like(y), 0, 10, lr=lr)
    fig_dev = np.abs(y.cpu().numpy().astype(np.float64) - Y64).max() / np.abs(Y64).max()
    fig_np = np.abs(Ynp.astype(np.float64) - Y64).max() / np.abs(Y64).max()
    print(f"TSNE trajectory {name}: device {fig_dev:.3e}, numpy fp32 {fig_np:.3e}, ratio {fig_dev / fig_np:.3f} (margin {TRAJECTORY_MARGIN})")
    assert fig_dev <= TRAJECTORY_MARGIN * fig_np


# ---- determinism ----------------------------------------------------------------------------------------------------------------
def test_runs_are_deterministic_and_spans_compose():
    from ppt_amd import ops, tsne as T
    x, _, _ = _e2e("a")
    runs = [T.tsne(x, perplexity=30.0, n_iter=300, seed=4) for _ in range(2)]
    (Y1, info1), (Y2, info2) = runs
    assert Y1.dtype == torch.float32 and Y1.shape == (300, 2) and Y1.is_cuda and torch.isfinite(Y1).all()
    assert torch.equal(Y1.view(torch.int32), Y2.view(torch.int32))
    assert torch.equal(info1["betas"].view(torch.int32), info2["betas"].view(torch.int32))
    assert info1["stats"] == info2["stats"] and [s[0] for s in info1["stats"]] == [49, 99, 149, 199, 249, 299]
    assert info1["n_iter"] == 300 and info1["kl_divergence"] == info1["stats"][-1][1] and info1["learning_rate"] == 50.0
    # no reads at all, and checks whose stop rules never fire: the same Y
    Y3, info3 = T.tsne(x, perplexity=30.0, n_iter=300, seed=4, check_every=None)
    Y4, info4 = T.tsne(x, perplexity=30.0, n_iter=300, seed=4, check_every=50, min_grad_norm=0.0, n_iter_without_progress=10 ** 9)
    assert info4["stopped"] is None and info4["n_iter"] == 300 and info3["stats"] == []
    assert torch.equal(Y3.view(torch.int32), Y4.view(torch.int32)) and torch.equal(Y3.view(torch.int32), Y1.view(torch.int32))
    assert torch.is_tensor(info3["kl_divergence"]) and float(info3["kl_divergence"]) == info4["kl_divergence"]
    # 100 iterations as 50 + 50 (across nothing special) and 200 .. 300 as 50 + 50 across the switch at 250
    P, _, pstats = ops.tsne_affinities(torch.from_numpy(x).cuda(), 30.0)
    for t0 in (0, 200):
        states = []
        for spans in ((100,), (50, 50)):
            y = torch.from_numpy(R.random_init(300, 1)).cuda() * (1.0 if t0 == 0 else 3e4)
            upd, gn = torch.zeros_like(y), torch.ones_like(y)
            stats = torch.zeros((2, 2), dtype=torch.float32, device="cuda")
            t, row = t0, 0
            for n in spans:
                ops.tsne_steps(P, pstats, y, upd, gn, t, n, lr=50.0, check_every=50, stats=stats[row:])
                t, row = t + n, row + n // 50
            states.append((y, upd, gn, stats))
        for a, b in zip(*states):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert (states[0][3] != 0).all()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden(name):
    """(dense float64 KL of sklearn's default embeddings, their 1-NN purities)"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g_tsne.npz"))
    _, labels, P64 = _e2e(name)
    ys = g[f"{name}_default"]
    return [R.kl_dense(P64, y) for y in ys], [R.nn_purity(y, labels) for y in ys], [R.kl_dense(P64, y) for y in g[f"{name}_exact"]]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("name", list(E2E_CASES))
def test_end_to_end_against_the_references_call(name, seed):
    """tsne() with the defaults against what sklearn's TSNE(n_components=2, learning_rate='auto', init='random') returned for
    five seeds (the golden file).  The float64 restatement evaluates the dense KL(P || Q(Y)) of every embedding; a device KL
    must be <= max_s KL(sklearn default, s) + (max_s - min_s) -- sklearn's own seed-to-seed range is the margin, nothing tighter
    separates two good embeddings -- and the 1-NN label purity at least the minimum of the golden ones.  On the CPU the fp32
    numpy restatement gave 0.2874 / 0.2862 / 0.2885 (case a, bound 0.3001) and 0.7756 / 0.7749 / 0.7694 (case b, bound 0.7960)
    for these three seeds."""
    from ppt_amd import tsne as T
    x, labels, P64 = _e2e(name)
    kls, purities, kls_exact = _golden(name)
    bound = max(kls) + (max(kls) - min(kls))
    Y, info = T.tsne(x, perplexity=E2E_CASES[name]["perplexity"], seed=seed)
    Yh = Y.cpu().numpy()
    kl, purity = R.kl_dense(P64, Yh), R.nn_purity(Yh, labels)
    print(f"TSNE end to end {name} seed {seed}: dense KL {kl:.4f} (device's own {info['kl_divergence']:.4f}, {info['n_iter']} iterations), "
          f"bound {bound:.4f}; sklearn default {min(kls):.4f}-{max(kls):.4f}, exact {min(kls_exact):.4f}-{max(kls_exact):.4f}; "
          f"purity {purity:.3f} (golden minimum {min(purities):.3f})")
    assert np.isfinite(Yh).all()
    assert kl <= bound
    assert purity >= min(purities)
    assert abs(info["kl_divergence"] - kl) <= 1e-3 * kl     # the device's own figure (fp32 P, fp32 sums) tells the same story


# ---- the picture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 5])
def test_feature_scatter_is_the_sequential_renderer_on_the_numpy_pixels(radius):
    from ppt_amd import tsne as T
    n, size, classes = 257, 96, 40
    Y = (np.random.RandomState(21).standard_normal((n, 2)) * [22.0, 9.0]).astype(np.float32)
    labels = np.arange(n) % classes
    ixyz, values = R.scatter_pixels(Y, size)
    assert not viz_ref.in_band(values[:, :2]).any()
    pal = T.class_palette(classes)
    assert len({tuple(c) for c in pal.tolist()}) == classes                     # one distinct colour per class
    colors = pal.numpy()[labels][None]
    want, win = viz_ref.render_sequential(ixyz, colors, size, size, radius, (255, 255, 255))
    got = T.feature_scatter(torch.from_numpy(Y).cuda(), torch.from_numpy(labels), size=size, radius=radius)
    assert got.dtype == torch.uint8 and got.shape == (size, size, 3) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want[0])
    assert 0.02 < (win >= 0).mean() < 0.98
    if radius == 1:                                                             # r = 1: shade 1, depth 0 -> intensity 0.65: flat colours
        seen = {tuple(c) for c in got.cpu().numpy()[win >= 0].tolist()}
        assert len(seen) == len(np.unique(labels[np.unique(win[win >= 0])]))
