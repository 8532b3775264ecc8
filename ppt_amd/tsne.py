"""The feature-distribution figure on the device: the "mn40 and sonn Feature Distribution" cells of notebook/visualize.ipynb.

The notebook loads the payload of save_recog_feats (test_feats [n, C], test_labels), calls
sklearn.manifold.TSNE(n_components=2, learning_rate='auto', init='random').fit_transform(test_feats) on the CPU and scatters the
result coloured by label.  Here the logits never leave the device: csrc/tsne.hip runs the exact O(N^2) algorithm (two launches
per iteration, P read once per iteration) and the ball renderer of ppt_amd.viz draws the scatter.

    Y, info = tsne(logits, perplexity=30.0, seed=0)                  # [n, 2] f32 on the device; info['kl_divergence'], ...
    img = feature_scatter(Y, labels, size=1000, radius=6)            # uint8 [1000, 1000, 3] on the device
    viz.save_png("mn40_feats.png", img)
    python -m ppt_amd.analysis tsne --feats modelnet40_test_feats_labels.pt --out mn40_feats.png

The algorithm is this project's own statement (include/ppt_hip.h: ppt_tsne_affinities, ppt_tsne_steps), held to an fp64
restatement by the tests.  Not in scope: Barnes-Hut (the exact method is the fast one here), PCA initialisation,
n_components != 2, metrics other than squared Euclidean, the seaborn look of the notebook's figure -- and any promise of
sklearn's coordinates: the optimisation is chaotic (an fp32 and an fp64 run of the same statement from the same start differ by
O(1) of the embedding's extent by iteration 50), so embeddings are compared by their KL divergence, not point by point.
"""
import colorsys

import numpy as np
import torch

from . import ops

EXPLORATION_ITERS = 250            # sklearn's _EXPLORATION_MAX_ITER: the early-exaggeration stage, momentum 0.5
SCATTER_MARGIN = 0.05              # share of the picture left free on every side of the embedding's bounding box


def auto_learning_rate(n, early_exaggeration):
    """sklearn's learning_rate='auto': max(N / early_exaggeration / 4, 50)"""
    return max(n / early_exaggeration / 4.0, 50.0)


def random_init(n, seed):
    """init='random': 1e-4 * standard normal from numpy's RandomState(seed), as float32 [n, 2] (host)"""
    return (1e-4 * np.random.RandomState(seed).standard_normal((n, 2))).astype(np.float32)


def features_f32(feats):
    """a device tensor, a CPU tensor or a numpy array of any float dtype -> a contiguous f32 tensor [n, C] on the same device
    (the payload's float64 test_feats hold fp32 logits exactly: nothing is lost)"""
    t = feats if torch.is_tensor(feats) else torch.from_numpy(np.ascontiguousarray(feats))
    if t.dim() != 2 or not t.is_floating_point():
        raise ValueError(f"tsne: features must be a float matrix [n, C], got {t.dtype} {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


def stop_check(i, error, grad_norm, best_error, best_iter, n_iter_without_progress, min_grad_norm):
    """The stop rules of sklearn's _gradient_descent at a check iteration i, as a pure function:
    -> (reason | None, best_error, best_iter).  A smaller error resets the progress clock; otherwise more than
    n_iter_without_progress iterations since the best one stop the stage ('no_progress'); a gradient norm at or below
    min_grad_norm stops it too ('grad_norm')."""
    if error < best_error:
        best_error, best_iter = error, i
    elif i - best_iter > n_iter_without_progress:
        return "no_progress", best_error, best_iter
    if grad_norm <= min_grad_norm:
        return "grad_norm", best_error, best_iter
    return None, best_error, best_iter


def check_spans(t_begin, t_end, check_every):
    """[t_begin, t_end) cut after every iteration t with (t + 1) % check_every == 0: [(t0, n, ends_on_check)]"""
    spans, t = [], t_begin
    while t < t_end:
        nxt = t_end if not check_every else min((t // check_every + 1) * check_every, t_end)
        spans.append((t, nxt - t, bool(check_every) and nxt % check_every == 0))
        t = nxt
    return spans


def tsne(feats, perplexity=30.0, n_iter=1000, early_exaggeration=12.0, learning_rate='auto', init='random', seed=0,
         n_iter_without_progress=300, min_grad_norm=1e-7, check_every=50):
    """Exact t-SNE of feats [n, C] in two dimensions -> (Y [n, 2] f32 on the device, info).

    The defaults are those of the notebook's call.  learning_rate='auto': max(n / early_exaggeration / 4, 50); init='random':
    random_init(n, seed), or a caller's [n, 2] tensor / array.  The first min(250, n_iter) iterations run exaggerated with
    momentum 0.5, the rest with momentum 0.8.  Every check_every iterations the device writes (KL, ||g||) and the host reads
    these two floats and applies stop_check (no progress counts as 250 iterations in the first stage, n_iter_without_progress
    in the second); check_every=None enqueues every iteration without a read.  info: 'kl_divergence' (of the last iteration;
    a 0-dim device tensor when check_every is None), 'n_iter' (iterations run), 'betas' [n] f32 on the device, 'stats'
    [(iteration, KL, ||g||)], 'learning_rate', 'stopped' (the reason the second stage ended early, or None)."""
    if not torch.cuda.is_available():
        raise RuntimeError("tsne: needs a CUDA/HIP device (ppt_amd has no CPU path)")
    x = features_f32(feats)
    n = x.shape[0]
    if perplexity >= n:
        raise ValueError("perplexity must be less than n_samples")
    if n_iter < 1 or (check_every is not None and check_every < 1):
        raise ValueError("tsne: n_iter and check_every must be positive")
    dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
    x = x.to(dev)
    lr = auto_learning_rate(n, early_exaggeration) if learning_rate == 'auto' else float(learning_rate)
    if isinstance(init, str):
        if init != 'random':
            raise ValueError(f"tsne: init must be 'random' or an [n, 2] array, got {init!r} (PCA initialisation is not in scope)")
        y = torch.from_numpy(random_init(n, seed)).to(dev)
    else:
        y = features_f32(init).to(dev).clone()
        if y.shape != (n, 2):
            raise ValueError(f"tsne: init must be [n, 2], got {tuple(y.shape)}")
    P, betas, pstats = ops.tsne_affinities(x, perplexity)
    update, gains = torch.zeros_like(y), torch.ones_like(y)
    workspace = torch.empty(ops.tsne_steps_workspace_bytes(n), dtype=torch.uint8, device=dev)
    ce = int(check_every or 0)
    rows = torch.zeros(((n_iter // ce if ce else 0) + 1, 2), dtype=torch.float32, device=dev)
    last = rows[-1:]                                        # the last iteration's figures, if it is not a check iteration anyway
    history, used, stopped = [], 0, None

    def steps(t0, count, t_switch, every, out):
        ops.tsne_steps(P, pstats, y, update, gains, t0, count, t_switch=t_switch, early_exaggeration=early_exaggeration, lr=lr,
                       check_every=every, stats=out, workspace=workspace)

    t, kl = 0, None
    explore_end = min(EXPLORATION_ITERS, n_iter)
    for t_end, t_switch, patience in ((explore_end, explore_end, EXPLORATION_ITERS), (n_iter, None, n_iter_without_progress)):
        t_switch = t if t_switch is None else t_switch      # the second stage begins where the first one ended
        best_error, best_iter, stopped = float("inf"), t, None
        for t0, count, on_check in check_spans(t, t_end, ce):
            final = t0 + count == n_iter
            if on_check:
                out = rows[used:used + 1]
                used += 1
                steps(t0, count, t_switch, ce, out)
                kl, norm = out[0].tolist()                  # the one two-float read of this check
                history.append((t0 + count - 1, kl, norm))
                stopped, best_error, best_iter = stop_check(t0 + count - 1, kl, norm, best_error, best_iter, patience, min_grad_norm)
            elif final:                                     # the last iteration reports its KL as sklearn's does: a span of its own
                if count > 1:
                    steps(t0, count - 1, t_switch, 0, None)
                steps(t0 + count - 1, 1, t_switch, 1, last)
                kl = last[0, 0]
            else:
                steps(t0, count, t_switch, 0, None)
            t = t0 + count
            if stopped:
                break
    if torch.is_tensor(kl) and check_every is not None:
        kl = float(kl)
    return y, {"kl_divergence": kl, "n_iter": t, "betas": betas, "stats": history, "learning_rate": lr, "stopped": stopped}


def class_palette(n):
    """n distinct RGB colours (0-255) for n classes, for any n: hues step by the golden ratio, saturation and value cycle over
    three levels; a colour that repeats an earlier one as bytes is skipped.  (The notebook's sns.color_palette(None, 40) cycles
    ten colours over forty classes; that is not reproduced.)  -> [n, 3] f32 tensor"""
    out, seen, k = [], set(), 0
    while len(out) < n:
        h = (k * 0.6180339887498949) % 1.0
        s, v = (0.85, 0.55, 1.0)[k % 3], (0.90, 0.70, 0.55)[(k // 3) % 3]
        rgb = tuple(int(round(255 * c)) for c in colorsys.hsv_to_rgb(h, s, v))
        k += 1
        if rgb not in seen and rgb != (255, 255, 255):
            seen.add(rgb)
            out.append(rgb)
    return torch.tensor(out, dtype=torch.float32).reshape(-1, 3)


def scatter_pixels(Y, size, margin=SCATTER_MARGIN):
    """Y [n, 2] (any float dtype, any device) -> ixyz [n, 3] int32 on the same device: row, column, depth 0 in a size x size
    picture.  In float64, in this order: lo, hi = the per-axis minimum and maximum; span = the larger of the two extents (1 if
    both are 0): one scale for both axes; u = ((Y - lo) + (span - (hi - lo)) / 2) / span in [0, 1], each axis centred;
    column = margin (size - 1) + u_x ((1 - 2 margin) (size - 1)), row = margin (size - 1) + (1 - u_y) ((1 - 2 margin)
    (size - 1)) -- y points upwards --; truncated toward zero."""
    if Y.dim() != 2 or Y.shape[1] != 2:
        raise ValueError(f"scatter_pixels: Y must be [n, 2], got {tuple(Y.shape)}")
    p = Y.detach().double()
    lo, hi = p.amin(dim=0), p.amax(dim=0)
    extent = hi - lo
    span = extent.amax()
    span = torch.where(span > 0, span, torch.ones_like(span))
    u = ((p - lo) + (span - extent) / 2.0) / span
    edge, inner = margin * (size - 1), (1.0 - 2.0 * margin) * (size - 1)
    col = edge + u[:, 0] * inner
    row = edge + (1.0 - u[:, 1]) * inner
    return torch.stack([row, col, torch.zeros_like(row)], dim=1).to(torch.int32)


def feature_scatter(Y, labels, size=1000, radius=6, palette=None, background=(255, 255, 255)):
    """The scatter of an embedding Y [n, 2] coloured by label -> uint8 [size, size, 3] on the device (viz.render_balls: every
    point a shaded ball; all depths are 0, so where two balls overlap the lower point index wins).  palette: [>= classes, 3]
    colours in [0, 255] (default: class_palette(max label + 1), one distinct colour per class)."""
    from . import viz
    labels = torch.as_tensor(labels).to(Y.device).long().reshape(-1)
    if labels.shape[0] != Y.shape[0]:
        raise ValueError("feature_scatter: Y and labels differ in length")
    classes = int(labels.max()) + 1 if labels.numel() else 0
    pal = class_palette(classes) if palette is None else torch.as_tensor(palette, dtype=torch.float32).reshape(-1, 3)
    if labels.numel() and (int(labels.min()) < 0 or pal.shape[0] < classes):
        raise ValueError(f"feature_scatter: labels in [0, {classes}) need {classes} colours, the palette has {pal.shape[0]}")
    colors = pal.to(Y.device)[labels]
    return viz.render_balls(scatter_pixels(Y, size), colors, int(size), radius, background)
