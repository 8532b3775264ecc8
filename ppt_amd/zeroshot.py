"""Zero-shot classification on the device: the frozen ULIP model scored with hand-written prompt templates -- the baseline every
PPT result table starts from (parser.py:24,60: --evaluate_3d, --test_ckpt_addr "the ckpt to test 3d zero shot"; the templates of
the reference's data/templates.json: `modelnet40_64`, `shapenet_64`).

    sentences, group_sizes = build_sentences(classnames, templates)          # class-major: template.format(name)
    token_ids = SimpleTokenizer(bpe)(sentences)                              # host [S, 77]; or ready ids from anywhere
    W = classifier(model, token_ids, group_sizes)                            # [C, E]: normalise, mean over templates, normalise
    logits = ZeroShot(model, W, classnames)(pc)                              # exp(logit_scale) * cos(encode_pc(pc), W[c])
    figures = zeroshot_validate(loader, model, token_ids, group_sizes, args) # evaluate.validate's acc / acc5 / per_class_acc / loss
    python -m ppt_amd.zeroshot --test test.npz --dataset_name modelnet40 --templates templates.json --key modelnet40_64 [--bpe ...]
                               [--token_ids ids.npz] [--ulip2] [--ckpt checkpoint_best.pt --head_type H]

The command builds the model as ppt_amd.fewshot / ppt_amd.analysis do: the pretrained files under ./data are loaded and a missing
one raises (PPT_SYNTHETIC_WEIGHTS=1 is the explicit opt-out).

The sentences go through the CLIP text tower in the RAGGED row layout (ULIP_WITH_IMAGE.encode_sentences ->
engine.text_tower_forward_ragged): sentence s owns len_s = argmax(ids[s]) + 1 rows, nothing behind its EOT token is stored or
computed -- 23 064 rows instead of 33 280 for ModelNet40 x 64 templates.  Any text works: another class set than the one the
model was built with, free captions for text-to-shape retrieval.  Tokenisation needs the CLIP merge table, which is not shipped
(ppt_amd.tokenizer.find_vocab); every function here therefore takes ready token ids.
"""
import argparse
import json

import numpy as np
import torch
from torch import nn

from . import engine, ops

# Rows of the text tower per chunk of encode_sentences when the caller names none: None = all sentences in one pass (a sentence
# is never split).  profiles/zeroshot.md has the measurement behind the choice.
DEFAULT_MAX_ROWS = None


def build_sentences(classnames, templates):
    """-> (sentences, group_sizes): template.format(name) for every class and template, CLASS-major (all templates of class 0, then
    class 1, ...), `_` in a name replaced by a space as PromptLearner does (ULIP_models.py:95); group_sizes[c] = sentences of class c."""
    classnames, templates = list(classnames), list(templates)
    if not classnames or not templates:
        raise ValueError("build_sentences: no class names or no templates")
    sentences = [t.format(name.replace("_", " ")) for name in classnames for t in templates]
    return sentences, [len(templates)] * len(classnames)


def _host_ids(token_ids):
    ids = token_ids.detach().cpu().numpy() if isinstance(token_ids, torch.Tensor) else np.asarray(token_ids)
    if ids.ndim != 2 or ids.shape[0] == 0 or ids.shape[1] == 0:
        raise ValueError("token ids: expected a non-empty [S, ctx] integer array")
    if ids.dtype.kind not in "iu":
        raise ValueError(f"token ids: expected integers, got {ids.dtype}")
    return ids.astype(np.int64)


def ragged_layout(token_ids):
    """HOST: token ids [S, ctx] -> (lens [S], offsets [S + 1]) int64 numpy.  len_s = argmax(ids[s]) + 1 -- the reference's EOT rule
    (ULIP_models.py:219: the EOT token has the highest id; FIRST maximum, so a sentence the tokenizer cut at ctx without an EOT
    ends at the first occurrence of its largest id); offsets = cumsum: sentence s owns rows [offsets[s], offsets[s + 1])."""
    ids = _host_ids(token_ids)
    lens = ids.argmax(axis=1).astype(np.int64) + 1
    return lens, np.concatenate([np.zeros(1, np.int64), np.cumsum(lens)])


def encode_sentences(model, token_ids, max_rows=None):
    """ULIP_WITH_IMAGE.encode_sentences (see there)."""
    ids = _host_ids(token_ids)
    vocab, ctx = model.token_embedding.weight.shape[0], model.positional_embedding.shape[0]
    if ids.shape[1] > ctx:
        raise ValueError(f"encode_sentences: {ids.shape[1]} positions, the model's context length is {ctx}")
    if int(ids.min()) < 0 or int(ids.max()) >= vocab:
        raise ValueError(f"encode_sentences: token id outside [0, {vocab})")
    if max_rows is None:
        max_rows = DEFAULT_MAX_ROWS
    lens, _ = ragged_layout(ids)
    if max_rows is not None and int(lens.max()) > int(max_rows):
        raise ValueError(f"encode_sentences: max_rows = {max_rows} is below the longest sentence ({int(lens.max())} positions)")
    dev = model.positional_embedding.device
    if dev.type != "cuda":
        raise RuntimeError("encode_sentences: the model is not on a CUDA/HIP device (ppt_amd has no CPU path)")
    # chunks of whole sentences, at most max_rows rows each
    bounds, rows = [0], 0
    for s, n in enumerate(lens.tolist()):
        if max_rows is not None and rows + n > int(max_rows):
            bounds.append(s)
            rows = 0
        rows += n
    bounds.append(len(lens))
    heads, layers = model.transformer.heads, model.transformer.layers
    out = []
    with torch.no_grad():
        if not model._text_calibrated:
            model.calibrate_text_precision()                # the half-vs-fp32 check of the text tower on THESE weights (mixed16)
        sd, cache = model._live_state(), model._cache()
        table, pos = sd["token_embedding.weight"].detach(), sd["positional_embedding"].detach()
        for a, b in zip(bounds[:-1], bounds[1:]):
            ln = lens[a:b]
            off = np.concatenate([np.zeros(1, np.int64), np.cumsum(ln)])
            ids_d = torch.from_numpy(ids[a:b].astype(np.int32)).to(dev)
            off_d = torch.from_numpy(off.astype(np.int32)).to(dev)
            plan = torch.from_numpy(ops.ragged_attention_plan(ln)).to(dev)
            x0 = ops.sentence_rows(table, pos, ids_d, off_d, int(off[-1]))
            out.append(engine.text_tower_forward_ragged(sd, cache, x0, off_d, int(ln.max()), heads, layers, plan=plan))
    return out[0] if len(out) == 1 else torch.cat(out, dim=0)


def _group_offsets(group_sizes, S):
    sizes = np.asarray(list(group_sizes), dtype=np.int64).reshape(-1)
    if sizes.size == 0 or int(sizes.min()) < 1:
        raise ValueError("group sizes: every class needs at least one sentence")
    if int(sizes.sum()) != S:
        raise ValueError(f"group sizes add up to {int(sizes.sum())}, there are {S} sentences")
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(sizes)]).astype(np.int32)


def classifier(model, token_ids, group_sizes, max_rows=None):
    """-> W [C, E] fp32 unit rows: class c's sentences are the contiguous range of group_sizes[c] rows of token_ids (class-major,
    build_sentences); W[c] = normalize(mean_t normalize(encode_sentences(t))) -- ULIP's zero-shot rule (ops.template_ensemble)."""
    ids = _host_ids(token_ids)
    goff = _group_offsets(group_sizes, ids.shape[0])            # (checked before anything is launched)
    feat = encode_sentences(model, ids, max_rows)
    return ops.template_ensemble(feat.contiguous(), torch.from_numpy(goff).to(feat.device))


class ZeroShot(nn.Module):
    """The frozen model as a zero-shot classifier over the classes of W [C, E] (classifier()): forward(pc) -> logits [B, C] =
    exp(logit_scale) * <f / |f|, W[c]> with f = model.encode_pc(pc) -- the CLIP / ULIP rule (ops.cosine_head).  This is NOT PPT's
    own forward (ULIP_models.py:279-281), which leaves the point feature un-normalised.  No gradient.  Usable as the `model` of
    evaluate.validate: acc, acc5, per_class_acc and loss then come from the metric kernel; classnames (optional) name the rows
    of W for the caller."""

    def __init__(self, model, W, classnames=None):
        super().__init__()
        if W.dim() != 2:
            raise ValueError("ZeroShot: W must be [C, E]")
        if classnames is not None and len(classnames) != W.shape[0]:
            raise ValueError(f"ZeroShot: {len(classnames)} class names for {W.shape[0]} rows of W")
        self.model = model
        self.register_buffer("W", W.detach().float().contiguous(), persistent=False)
        self.classnames = None if classnames is None else list(classnames)

    def forward(self, pc):
        if not pc.is_cuda:
            raise RuntimeError("ZeroShot: expected a CUDA/HIP tensor (ppt_amd has no CPU path)")
        with torch.no_grad():
            f = self.model.encode_pc(pc)
            return ops.cosine_head(f.float().contiguous(), self.W, self.model.logit_scale.detach())


def zeroshot_validate(loader, model, token_ids, group_sizes, args):
    """evaluate.validate of ZeroShot(model, classifier(model, token_ids, group_sizes)) over `loader`; args as validate takes them
    (gpu, classnames; label_smoothing for the reported loss, default 0) plus max_rows (optional)."""
    from .evaluate import validate
    W = classifier(model, token_ids, group_sizes, getattr(args, "max_rows", None))
    zs = ZeroShot(model, W, getattr(args, "classnames", None))
    criterion = torch.nn.CrossEntropyLoss(label_smoothing=float(getattr(args, "label_smoothing", 0.0)))
    return validate(loader, zs, criterion, args)


def main(argv=None):
    ap = argparse.ArgumentParser(description="zero-shot 3D classification with prompt templates on a cloud file (.npz: points "
                                             "[M, N, 3] f32, labels [M])")
    ap.add_argument("--test", required=True)
    ap.add_argument("--dataset_name", default="modelnet40")
    ap.add_argument("--templates", help="JSON file: {key: [template strings with one {}]} (the reference's data/templates.json)")
    ap.add_argument("--key", default="modelnet40_64")
    ap.add_argument("--bpe", default=None, help="the CLIP merge table (bpe_simple_vocab_16e6.txt.gz)")
    ap.add_argument("--token_ids", default=None, help=".npz with token_ids [S, 77] and group_sizes [C] instead of --templates")
    ap.add_argument("--ulip2", action="store_true", help="the ULIP-2 point checkpoint (pointbert_ulip2.pt) instead of pointbert.pt")
    ap.add_argument("--ckpt", default=None, help="a checkpoint_best.pt of a tuned model (its un-frozen last-block tensors are loaded)")
    ap.add_argument("--head_type", type=int, default=0, help="the head_type the --ckpt model was tuned with")
    ap.add_argument("--npoints", type=int, default=8192)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--precision", default="mixed16", choices=("mixed16", "split16", "fp32"))
    ap.add_argument("--max_rows", type=int, default=None)
    ap.add_argument("--label_smoothing", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--gpu", type=int, default=0)
    args = ap.parse_args(argv)
    from .data import DeviceBatchLoader, DeviceCloudSet
    from .models import ULIP_models as M
    args.classnames = M.dataset_classnames(args.dataset_name)
    # evaluate_3d = False: the factory reads ./data/pretrained_models/pointbert[_ulip2].pt and ./data/initialize_models/
    # slip_base_100ep.pt as every other program here does, and a missing file raises (PPT_SYNTHETIC_WEIGHTS=1 is the explicit
    # opt-out).  With evaluate_3d set the factory loads nothing -- the reference pairs that flag with --test_ckpt_addr.
    args.task, args.evaluate_3d = "cls", False
    args.template_init, args.class_name_position, args.num_learnable_prompt_tokens = "", "middle", 32
    if args.token_ids:
        with np.load(args.token_ids) as f:
            token_ids, group_sizes = f["token_ids"], f["group_sizes"].tolist()
    elif args.templates:
        from .tokenizer import SimpleTokenizer
        with open(args.templates) as fh:
            templates = json.load(fh)[args.key]
        sentences, group_sizes = build_sentences(args.classnames, templates)
        token_ids = SimpleTokenizer(args.bpe)(sentences)
        if token_ids.dim() == 1:
            token_ids = token_ids[None]
    else:
        ap.error("one of --templates and --token_ids is required")
    model = M.ULIP_PointBERT(args)                     # (on the host: a missing checkpoint raises before the device is touched)
    if args.ckpt:
        from .train import load_prompt_checkpoint
        load_prompt_checkpoint(model, torch.load(args.ckpt, map_location="cpu", weights_only=False))
    torch.cuda.set_device(args.gpu)
    model = model.cuda().set_precision(args.precision)
    with np.load(args.test) as f:
        test_set = DeviceCloudSet(np.ascontiguousarray(f["points"], dtype=np.float32), f["labels"])
    print('------ len(val_dataset)', len(test_set))
    recipe = "scanobjectnn" if args.dataset_name.startswith("scanobjectnn") else "modelnet"
    loader = DeviceBatchLoader(test_set, args.batch_size, args.npoints, recipe, train=False, shuffle=False, drop_last=False, seed=args.seed)
    out = zeroshot_validate(loader, model, token_ids, group_sizes, args)
    print(out)
    return out


if __name__ == "__main__":
    main()
