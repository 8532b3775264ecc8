"""A numpy restatement of the t-SNE statement in include/ppt_hip.h (ppt_tsne_affinities, ppt_tsne_steps), parametrised by dtype:
float64 is the judge of the device tests, float32 a yardstick for what rounding alone does.  It also makes the inputs.

Nothing here is taken from sklearn's source; tests/golden/make_golden_tsne.py records what sklearn's own call returns."""
import numpy as np

SEARCH_STEPS, SEARCH_TOL = 100, 1e-5
EXPLORATION_ITERS = 250
EPS32 = 2.0 ** -24                                         # unit round-off of fp32


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def blobs(N, D, K, seed=0, scale=1.0, duplicates=False):
    """K centres N(0, 4^2) in D dimensions, unit noise, labels i % K, float32.  scale=50: the "logit-scale" variant;
    duplicates: the last eighth of the rows repeats the first rows exactly.  -> (x [N, D] f32, labels [N] int64)"""
    rng = np.random.RandomState(seed)
    centres = rng.normal(0.0, 4.0, (K, D))
    labels = np.arange(N) % K
    x = ((centres[labels] + rng.normal(0.0, 1.0, (N, D))) * scale).astype(np.float32)
    if duplicates:
        n8 = N // 8
        x[N - n8:] = x[:n8]
    return x, labels.astype(np.int64)


def duplicate_rows(N):
    """the rows that have an exact copy in blobs(..., duplicates=True)"""
    n8 = N // 8
    return np.concatenate([np.arange(n8), np.arange(N - n8, N)])


# ---- affinities -----------------------------------------------------------------------------------------------------------------
def sqdist(x, dtype=np.float64):
    """d_ij = sum_c (x_ic - x_jc)^2, the columns accumulated in ascending order, every step in `dtype`"""
    x = np.asarray(x).astype(dtype)
    d = np.zeros((x.shape[0], x.shape[0]), dtype)
    for c in range(x.shape[1]):
        t = x[:, None, c] - x[None, :, c]
        d += t * t
    return d


def shifted(d):
    """e_ij = d_ij - m_i with m_i = min_{j != i} d_ij; the diagonal is set to 0 (it is masked everywhere)"""
    n = d.shape[0]
    off = ~np.eye(n, dtype=bool)
    m = np.where(off, d, np.inf).min(axis=1)
    e = d - m[:, None]
    e[~off] = 0
    return e, m


def entropy_rows(e, beta, dtype=np.float64):
    """(H, S, q) of every row at its beta: q_ij = exp(-(beta_i e_ij)) off the diagonal, S = sum q, H = log S + beta A / S"""
    e = e.astype(dtype)
    beta = np.asarray(beta).astype(dtype)
    off = ~np.eye(e.shape[0], dtype=bool)
    q = np.where(off, np.exp(-(beta[:, None] * e)), dtype(0))
    S = q.sum(axis=1)
    A = (e * q).sum(axis=1)
    return np.log(S) + beta * A / S, S, q


def search(e, perplexity, dtype=np.float64):
    """The perplexity search of the statement for all rows at once -> (beta [N], converged [N] bool)"""
    n = e.shape[0]
    target = dtype(np.log(perplexity))
    beta, lo, hi = np.ones(n, dtype), np.full(n, -np.inf, dtype), np.full(n, np.inf, dtype)
    done = np.zeros(n, bool)
    for step in range(SEARCH_STEPS):
        H, _, _ = entropy_rows(e, beta, dtype)
        diff = H - target
        done |= np.abs(diff) <= SEARCH_TOL
        if done.all() or step == SEARCH_STEPS - 1:
            break
        up, down = ~done & (diff > 0), ~done & ~(diff > 0)
        lo = np.where(up, beta, lo)
        hi = np.where(down, beta, hi)
        with np.errstate(invalid="ignore"):
            nb_up = np.where(np.isinf(hi), beta * dtype(2), (beta + hi) * dtype(0.5))
            nb_down = np.where(np.isinf(lo), beta * dtype(0.5), (beta + lo) * dtype(0.5))
        beta = np.where(up, nb_up, np.where(down, nb_down, beta))
    return beta, done


def conditionals(e, beta, dtype=np.float64):
    """p_{j|i} = q_ij(beta_i) / S_i"""
    _, S, q = entropy_rows(e, beta, dtype)
    return q / S[:, None]


def joint(cond):
    """P_ij = (p_{j|i} + p_{i|j}) / (2 N), P_ii = 0"""
    return (cond + cond.T) / cond.dtype.type(2 * cond.shape[0])


def affinities(x, perplexity, dtype=np.float64):
    """-> (P [N, N], beta [N], converged [N]) of the statement in `dtype`"""
    e, _ = shifted(sqdist(x, dtype))
    beta, done = search(e, perplexity, dtype)
    return joint(conditionals(e, beta, dtype)), beta, done


# ---- the descent ----------------------------------------------------------------------------------------------------------------
def pair_pass(P, Y, alpha, dtype=np.float64):
    """-> dict(g [N, 2], Z, kl, norm, attr_abs [N, 2], rep_abs [N, 2]): the gradient, KL_t and ||g|| of the statement in `dtype`;
    attr_abs / rep_abs: alpha sum_j P w |y_i - y_j| and sum_j w^2 |y_i - y_j| / Z, the magnitudes an error bound scales with"""
    P, Y = np.asarray(P).astype(dtype), np.asarray(Y).astype(dtype)
    alpha = dtype(alpha)
    diff = Y[:, None, :] - Y[None, :, :]
    dd = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + dtype(1)
    w = dtype(1) / dd
    np.fill_diagonal(w, 0)
    Z = w.sum(dtype=np.float64).astype(dtype) if dtype == np.float32 else w.sum()
    pw, ww = P * w, w * w
    a = (pw[..., None] * diff).sum(axis=1)
    r = (ww[..., None] * diff).sum(axis=1)
    g = dtype(4) * (alpha * a - r / Z)
    pos = P > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(pos, alpha * P * (np.log(np.where(pos, alpha * P, 1)) + np.log(Z) + np.log(dd)), 0)
    return dict(g=g, Z=Z, kl=terms.sum(), norm=np.sqrt((g.astype(np.float64) ** 2).sum()),
                attr_abs=alpha * (pw[..., None] * np.abs(diff)).sum(axis=1), rep_abs=(ww[..., None] * np.abs(diff)).sum(axis=1) / Z)


def kl_dense(P, Y):
    """KL(P || Q(Y)) of an embedding, in float64 (alpha = 1): what the end-to-end test ranks embeddings by"""
    return float(pair_pass(P, Y, 1.0, np.float64)["kl"])


def descent_step(g, y, update, gains, mu, lr, dtype=np.float32):
    """sklearn's _gradient_descent update, elementwise and in the statement's order -> (y, update, gains), new arrays"""
    g, y, update, gains = (np.asarray(v).astype(dtype) for v in (g, y, update, gains))
    inc = update * g < 0
    gains = np.where(inc, gains + dtype(0.2), gains * dtype(0.8))
    gains = np.maximum(gains, dtype(0.01))
    update = dtype(mu) * update - dtype(lr) * (g * gains)
    return y + update, update, gains


def run(P, Y0, n_iter, lr, early_exaggeration=12.0, t_switch=EXPLORATION_ITERS, dtype=np.float64, t0=0):
    """n_iter iterations from Y0 (update 0, gains 1) -> Y"""
    P = np.asarray(P).astype(dtype)
    y = np.asarray(Y0).astype(dtype)
    update, gains = np.zeros_like(y), np.ones_like(y)
    for t in range(t0, t0 + n_iter):
        alpha, mu = (early_exaggeration, 0.5) if t < t_switch else (1.0, 0.8)
        g = pair_pass(P, y, alpha, dtype)["g"]
        y, update, gains = descent_step(g, y, update, gains, mu, lr, dtype)
    return y


def auto_learning_rate(n, early_exaggeration=12.0):
    return max(n / early_exaggeration / 4.0, 50.0)


def random_init(n, seed):
    return (1e-4 * np.random.RandomState(seed).standard_normal((n, 2))).astype(np.float32)


def nn_purity(Y, labels):
    """share of points whose nearest neighbour in the embedding carries their label"""
    Y = np.asarray(Y, np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    return float((labels[d.argmin(axis=1)] == labels).mean())


# ---- the picture ----------------------------------------------------------------------------------------------------------------
def scatter_pixels(Y, size, margin=0.05):
    """ppt_amd.tsne.scatter_pixels in float64 numpy -> (ixyz [n, 3] int32, the float64 (row, col) before truncation)"""
    p = np.asarray(Y).astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    extent = hi - lo
    span = extent.max()
    span = span if span > 0 else 1.0
    u = ((p - lo) + (span - extent) / 2.0) / span
    edge, inner = margin * (size - 1), (1.0 - 2.0 * margin) * (size - 1)
    col = edge + u[:, 0] * inner
    row = edge + (1.0 - u[:, 1]) * inner
    values = np.stack([row, col, np.zeros_like(row)], axis=1)
    return values.astype(np.int32), values
