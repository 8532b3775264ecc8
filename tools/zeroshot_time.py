"""Times the zero-shot classifier of ppt_amd/zeroshot.py on a ModelNet40 x 64-template sentence set, per precision mode:

    classifier / encode_sentences   max_rows = 4096 (chunks of whole sentences) against one pass over all rows
    padded                          what encode_text could do: model.tokenized_prompts pointed at the sentence ids, then
                                    encode_text(token_embedding(ids)) under no_grad (truncated to the longest sentence)

    python tools/zeroshot_time.py [--token_ids ids.npz | --templates templates.json --key modelnet40_64 --bpe merges.txt.gz]
                                  [--reps 5] [--out FILE.json]

Without token ids (an .npz with token_ids [S, 77] and group_sizes [C], or a template file and the CLIP merge table) a seeded
stand-in is used: 40 x 64 sentences of 6-13 tokens (SOT, random ids, EOT), the length range of the real set.  Synthetic weights,
eager launches on both sides, host clock around work that ends in a device synchronise; two warm-up calls of every candidate,
then `reps` repetitions in which the candidates ALTERNATE; median, min and max in milliseconds.  Also the relative L2 distance of
the ragged features from the padded ones.  Prints one JSON line (profiles/zeroshot.md).
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SOT, EOT = 49406, 49407


def stand_in_ids(classes=40, templates=64, seed=0):
    rng = np.random.default_rng(seed)
    lens = rng.integers(6, 14, size=classes * templates)
    ids = np.zeros((lens.size, 77), np.int64)
    for s, n in enumerate(lens):
        ids[s, 0], ids[s, n - 1] = SOT, EOT
        ids[s, 1:n - 1] = rng.integers(1, SOT, size=n - 2)
    return ids, [templates] * classes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--token_ids", default=None)
    ap.add_argument("--templates", default=None)
    ap.add_argument("--key", default="modelnet40_64")
    ap.add_argument("--bpe", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ppt_amd import weights as W, zeroshot as Z
    from ppt_amd.models import ULIP_models as M
    assert torch.cuda.is_available(), "zeroshot_time.py measures on the GPU"
    names = M.dataset_classnames("modelnet40")
    if a.token_ids:
        with np.load(a.token_ids) as f:
            ids, sizes = f["token_ids"].astype(np.int64), f["group_sizes"].tolist()
    elif a.templates:
        from ppt_amd.tokenizer import SimpleTokenizer
        sentences, sizes = Z.build_sentences(names, json.load(open(a.templates))[a.key])
        ids = SimpleTokenizer(a.bpe)(sentences).numpy()
    else:
        ids, sizes = stand_in_ids()
    lens, off = Z.ragged_layout(ids)
    args = SimpleNamespace(classnames=names, template_init='', class_name_position='middle', num_learnable_prompt_tokens=32, gpu=0,
                           task='cls', head_type=0, evaluate_3d=False, ulip2=False, synthetic_weights=True)
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.ULIP_PointBERT(args)
    m.load_state_dict(W.ulip_pointbert_state_dict(seed=0, with_token_embedding=True), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding(len(names), seed=0)
    m.cuda().eval()
    m.use_hip_graphs = False
    ids_t = torch.from_numpy(ids)
    ids_d = ids_t.cuda()
    own = m.tokenized_prompts

    def point_at(tok):
        m.tokenized_prompts, m._eot_pos, m._text_len_cache = tok, None, None

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    def padded():
        with torch.no_grad():
            return m.encode_text(m.token_embedding(ids_d), ids_d)

    res = {"sentences": int(ids.shape[0]), "ragged_rows": int(off[-1]), "padded_rows": int(ids.shape[0] * lens.max()),
           "len_min_mean_max": [int(lens.min()), float(lens.mean()), int(lens.max())], "reps": a.reps, "modes": {}}
    for mode in ("fp32", "split16", "mixed16"):
        m.set_precision(mode)
        point_at(own)
        cands = {"classifier_4096": lambda: Z.classifier(m, ids, sizes, max_rows=4096),
                 "classifier_one_pass": lambda: Z.classifier(m, ids, sizes, max_rows=10 ** 9),
                 "encode_4096": lambda: m.encode_sentences(ids_t, max_rows=4096),
                 "encode_one_pass": lambda: m.encode_sentences(ids_t, max_rows=10 ** 9)}
        for fn in cands.values():
            for _ in range(2):
                timed(fn)
        point_at(ids_t)
        for _ in range(2):
            timed(padded)
        cands["padded"] = padded
        times, outs = {k: [] for k in cands}, {}
        for _ in range(a.reps):
            for k, fn in cands.items():
                t, outs[k] = timed(fn)
                times[k].append(t)
        point_at(own)
        ref = outs["padded"]
        row = {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                   "spread_pct": round(100 * (max(v) - min(v)) / statistics.median(v), 2)} for k, v in times.items()}
        row["one_pass_vs_padded_rel_l2"] = ((outs["encode_one_pass"] - ref).norm() / ref.norm()).item()
        row["chunked_vs_padded_rel_l2"] = ((outs["encode_4096"] - ref).norm() / ref.norm()).item()
        row["chunked_equals_one_pass"] = bool(torch.equal(outs["encode_4096"], outs["encode_one_pass"]))
        row["text_operands"] = str(m._cache().dtype)
        res["modes"][mode] = row
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
