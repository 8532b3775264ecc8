"""The two readers of a checkpoint_best.pt, on the device: the nearest words of the learned prompt tokens (interpret_prompt.py)
and the test set's logits for the notebook (save_recog_feats.py).

    ids, dist = nearest_tokens(ctx, model.token_embedding.weight, topk=10)        # interpret_prompt.py:34-37
    rows = interpret_prompt(torch.load("checkpoint_best.pt"), model, topk=10)     # prints the reference's lines
    logits, labels = recognition_logits(model, loader)                            # save_recog_feats.py:53-73
    save_recog_feats("modelnet40_test_feats_labels.pt", logits, labels, names)    # save_recog_feats.py:75-78 (same payload)
    python -m ppt_amd.analysis interpret --fpath checkpoint_best.pt --topk 10 [--dataset_name modelnet40 --bpe_path FILE]
    python -m ppt_amd.analysis logits --fpath checkpoint_best.pt --data test.npz --out feats.pt [--dataset_name ... --head_type 2]
    feats, labels, names = load_recog_feats("modelnet40_test_feats_labels.pt")     # the payload back (visualize.ipynb's torch.load)
    python -m ppt_amd.analysis tsne --feats feats.pt --out mn40_feats.png [--coords y.npz --perplexity 30 --n_iter 1000 --seed 0]

The reference forms torch.cdist(ctx, token_embedding), a [M, 49408] matrix, and argsorts all of its columns for the first
topk; here csrc/nearest.hip reads the table once and keeps the k best per token (ops.nearest_rows).  The distances are the
direct form sqrt(sum (q - t)^2): a token initialised from a word (template_init, ULIP_models.py:80-83) is at distance exactly 0
from that word's row, where cdist's expanded form gives a few 1e-6.
"""
import argparse

import numpy as np
import torch

from . import ops


def nearest_tokens(ctx, token_embedding, topk):
    """ctx [M, D] (any float dtype; `.float()` as interpret_prompt.py:29), token_embedding [V, D] f32 on the device
    -> (ids [M, topk] int64, dist [M, topk] f32) on the device, ascending distance, equal distances by ascending id.
    Only the generic 2-D context, as in the reference: a class-specific [C, M, D] context raises ValueError."""
    if ctx.dim() != 2:
        raise ValueError(f"nearest_tokens: a generic context [M, D] is expected, got {tuple(ctx.shape)} "
                         "(the reference handles ctx.dim() == 2 only)")
    table = token_embedding.detach()
    q = ctx.detach().float().to(table.device).contiguous()
    idx, dist = ops.nearest_rows(q, table, int(topk))
    return idx.long(), dist


def _learnable_tokens(state):
    for key in ("state_dict", "state_dict_prompt"):               # main_cls.py:132 / main_partseg.py:135
        if key in state:
            state = state[key]
            break
    return state["learnable_tokens"]


def interpret_prompt(state, model, topk, bpe_path=None):
    """interpret_prompt.py:25-42 on a loaded checkpoint_best.pt payload (or a bare {'learnable_tokens': ...}) and a model that
    holds the token embedding: prints, per prompt token, the reference's line f"{m+1}: {words} {dist}" (distances ':.4f') and
    returns [(words | None, ids, dists)] per token.  Words come from ppt_amd.tokenizer's decoder when the CLIP merge table is
    found (bpe_path, PPT_BPE_VOCAB, ./utils/...); without it the ids are printed in their place and one line says so."""
    from .models.ULIP_models import _bpe
    token_embedding = model.token_embedding.weight
    print(f"Return the top-{topk} matched words")
    print(f"Size of token embedding: {token_embedding.shape}")
    ctx = _learnable_tokens(state)
    print(f"Size of context: {ctx.shape}")
    ids, dist = nearest_tokens(ctx, token_embedding, topk)
    ids, dist = ids.cpu().tolist(), dist.cpu().tolist()           # the one transfer
    tok = _bpe(bpe_path)
    if tok is None:
        print("(the CLIP merge table was not found: token ids are printed instead of words)")
    out = []
    for m, (row_ids, row_dist) in enumerate(zip(ids, dist)):
        words = None if tok is None else [tok.decoder[i] for i in row_ids]
        shown = [f"{d:.4f}" for d in row_dist]
        print(f"{m+1}: {row_ids if words is None else words} {shown}")
        out.append((words, row_ids, row_dist))
    return out


def recognition_logits(model, batches):
    """model(pc) over every batch (the short last one too), in eval mode under no_grad, as save_recog_feats.py:53-73.  `batches`:
    any iterable of (pc, label, ...) -- a DataLoader, DevicePrefetcher, DeviceBatchLoader or a list.  The precision mode is the
    model's current one; the training flag is restored.  No host read per batch.
    -> (logits [n, C] f32 on the device, labels [n] i64 on the device)"""
    was_training = model.training
    model.eval()
    logits, labels = [], []
    try:
        with torch.no_grad():
            for item in batches:
                pc, label = item[0], item[1]
                pred = model(pc.cuda(non_blocking=True))                                  # save_recog_feats.py:68-72
                logits.append(pred.float())
                labels.append(torch.as_tensor(label).to(pred.device, torch.int64).reshape(-1))
    finally:
        model.train(was_training)
    if not logits:
        raise ValueError("recognition_logits: no batches")
    return torch.cat(logits).contiguous(), torch.cat(labels)


def save_recog_feats(path, logits, labels, names):
    """The reference's payload (save_recog_feats.py:75-78) with torch.save: 'test_feats' float64 [n, C] (np.array of Python
    floats: exactly the fp32 logits), 'test_labels' int64 [n], 'test_names' a str array [n]."""
    feats = torch.as_tensor(logits).detach().float().cpu().numpy().astype(np.float64)
    payload = {'test_feats': feats,
               'test_labels': torch.as_tensor(labels).detach().cpu().numpy().astype(np.int64),
               'test_names': np.array([str(n) for n in names])}
    if payload['test_labels'].shape[0] != feats.shape[0] or payload['test_names'].shape[0] != feats.shape[0]:
        raise ValueError("save_recog_feats: logits, labels and names differ in length")
    torch.save(payload, path)
    return payload


def load_recog_feats(path):
    """The payload of save_recog_feats (or of the reference's save_recog_feats.py) back from disk, as the notebook's
    "Feature Distribution" cells read it: -> (test_feats float64 [n, C], test_labels int64 [n], test_names str [n] or None)"""
    payload = torch.load(path, map_location="cpu", weights_only=False)
    feats = np.asarray(payload['test_feats'], dtype=np.float64)
    labels = np.asarray(payload['test_labels']).astype(np.int64).reshape(-1)
    if feats.ndim != 2 or labels.shape[0] != feats.shape[0]:
        raise ValueError(f"load_recog_feats: test_feats {feats.shape} and test_labels {labels.shape} do not belong together")
    names = payload.get('test_names')
    return feats, labels, None if names is None else np.asarray(names)


def tsne_parser(sub):
    p = sub.add_parser("tsne", help="the notebook's feature-distribution figure from a save_recog_feats file (ppt_amd.tsne)")
    p.add_argument("--feats", required=True, help="the file `logits --out` (save_recog_feats) wrote")
    p.add_argument("--out", required=True, help="the PNG to write")
    p.add_argument("--coords", default=None, help="also write the embedding: .npz with Y [n, 2] f32, labels, kl_divergence")
    p.add_argument("--perplexity", type=float, default=30.0)
    p.add_argument("--n_iter", type=int, default=1000)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--size", type=int, default=1000)
    p.add_argument("--radius", type=int, default=6)
    return p


def tsne_figure(a):
    """`python -m ppt_amd.analysis tsne`: payload -> embedding on the device -> PNG (+ the coordinates)"""
    from . import tsne as T, viz
    feats, labels, _ = load_recog_feats(a.feats)
    Y, info = T.tsne(feats, perplexity=a.perplexity, n_iter=a.n_iter, seed=a.seed)
    viz.save_png(a.out, T.feature_scatter(Y, labels, size=a.size, radius=a.radius))
    if a.coords:
        np.savez(a.coords, Y=Y.cpu().numpy(), labels=labels, kl_divergence=np.float64(info["kl_divergence"]))
    print(f"=> {feats.shape[0]} points, KL divergence {info['kl_divergence']:.4f} after {info['n_iter']} iterations: {a.out}")
    return Y, info


def _build_model(a):
    from types import SimpleNamespace
    from .models import ULIP_models as M
    args = SimpleNamespace(classnames=M.dataset_classnames(a.dataset_name), template_init=a.template_init,
                           class_name_position=a.class_name_position, num_learnable_prompt_tokens=a.num_learnable_prompt_tokens,
                           gpu=0, task='cls', head_type=a.head_type, evaluate_3d=False, ulip2=a.ulip2, dataset_name=a.dataset_name)
    return M.ULIP_PointBERT(args).cuda(), args


def main(argv=None):
    ap = argparse.ArgumentParser(description="readers of a checkpoint_best.pt: nearest words of the prompt, logits of a test set")
    sub = ap.add_subparsers(dest="command", required=True)
    for name in ("interpret", "logits"):
        p = sub.add_parser(name)
        p.add_argument("--fpath", required=True, help="checkpoint_best.pt")
        p.add_argument("--dataset_name", default="modelnet40")
        p.add_argument("--template_init", default="")
        p.add_argument("--class_name_position", default="middle")
        p.add_argument("--num_learnable_prompt_tokens", type=int, default=32)
        p.add_argument("--head_type", type=int, default=0)
        p.add_argument("--ulip2", action="store_true")
        if name == "interpret":
            p.add_argument("--topk", type=int, default=10)
            p.add_argument("--bpe_path", default=None)
        else:
            p.add_argument("--data", required=True, help=".npz with points [M, N, 3] f32 and labels [M]")
            p.add_argument("--recipe", default="modelnet", choices=("modelnet", "scanobjectnn"))
            p.add_argument("--npoints", type=int, default=1024)
            p.add_argument("--batch_size", type=int, default=32)
            p.add_argument("--out", required=True)
    tsne_parser(sub)
    a = ap.parse_args(argv)
    if a.command == "tsne":
        return tsne_figure(a)
    state = torch.load(a.fpath, map_location="cpu", weights_only=False)
    model, args = _build_model(a)
    if a.command == "interpret":
        return interpret_prompt(state, model, a.topk, a.bpe_path)
    from .data import DeviceBatchLoader, DeviceCloudSet
    from .train import load_prompt_checkpoint
    load_prompt_checkpoint(model, state)                                                  # save_recog_feats.py:29-35
    with np.load(a.data) as f:
        cloud_set = DeviceCloudSet(np.ascontiguousarray(f["points"], dtype=np.float32), f["labels"])
    loader = DeviceBatchLoader(cloud_set, a.batch_size, a.npoints, a.recipe, train=False, shuffle=False)
    logits, labels = recognition_logits(model, loader)
    names = [args.classnames[i] for i in labels.cpu().tolist()]
    save_recog_feats(a.out, logits, labels, names)
    print('=> saved test feats!')
    return logits, labels


if __name__ == "__main__":
    main()
