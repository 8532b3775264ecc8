#!/usr/bin/env python3
"""Generate tests/golden/g_zeroshot.npz: the UPSTREAM REFERENCE's text features for sentences with DIFFERENT EOT positions
(models/ULIP_models.py:203-222 encode_text(token_embedding(ids), ids), imported through tests/golden/ref_import.py, CPU), for
ppt_amd/zeroshot.py.  Build container only; only arrays and strings are stored.

    python tests/golden/make_golden_zeroshot.py

Weights: ppt_amd.weights.ulip_pointbert_state_dict(seed=0, with_token_embedding=True).
(A) template set: 5 ModelNet40 names (the shortest- and the longest-tokenising one, a two-word one, two more) x the first 7
    strings of the reference's data/templates.json `modelnet40_64`, tokenised by the reference's utils/tokenizer.py:
    a_names, a_templates, a_sentences, a_ids [35, 77], a_feat [35, 512], a_W [5, 512].
(B) synthetic lengths: 12 sentences SOT, random ids below 49 406, EOT, zeros, of lengths 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65,
    77 in shuffled order: b_ids [12, 77], b_lens, b_offsets, b_feat [12, 512], b_groups (1, 4, 7), b_W [3, 512].
The classifiers follow ULIP's zero-shot rule in float64: normalise each sentence's feature, mean over the class, normalise.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_import as R                     # noqa: E402
from ppt_amd import weights as W           # noqa: E402

SOT, EOT = 49406, 49407
B_LENS = (2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 77)
B_GROUPS = (1, 4, 7)


def ulip_rule(feat, groups):
    f = torch.from_numpy(feat).double()
    f = f / f.norm(dim=-1, keepdim=True)
    out, a = [], 0
    for n in groups:
        w = f[a:a + n].mean(dim=0)
        out.append(w / w.norm())
        a += n
    return torch.stack(out).float().numpy()


def main():
    names40 = json.load(open(os.path.join(R.REF_ROOT, "data", "labels.json")))["modelnet40"]
    templates = json.load(open(os.path.join(R.REF_ROOT, "data", "templates.json")))["modelnet40_64"][:7]
    with R.reference_context():
        from utils.tokenizer import SimpleTokenizer
        tk = SimpleTokenizer()
    clean = [n.replace("_", " ") for n in names40]
    ntok = [len(tk.encode(n)) for n in clean]
    picked = [int(np.argmin(ntok)), int(np.argmax(ntok))]
    picked.append(next(i for i, n in enumerate(clean) if " " in n and i not in picked))
    picked += [i for i in range(len(clean)) if i not in picked][:2]
    names = [names40[i] for i in picked]
    sentences = [t.format(n.replace("_", " ")) for n in names for t in templates]
    a_ids = tk(sentences).numpy().astype(np.int64)
    assert a_ids.shape == (35, 77)

    rng = np.random.default_rng(20240)
    lens = np.asarray(B_LENS)[rng.permutation(len(B_LENS))]
    b_ids = np.zeros((len(lens), 77), np.int64)
    for s, n in enumerate(lens):
        b_ids[s, 0] = SOT
        b_ids[s, 1:n - 1] = rng.integers(1, SOT, size=n - 2)
        b_ids[s, n - 1] = EOT
    assert (b_ids.argmax(1) + 1 == lens).all()

    sd = W.ulip_pointbert_state_dict(seed=0, with_token_embedding=True)
    m = R.build_reference_ulip_pointbert(names40)
    msd = m.state_dict()
    m.load_state_dict({k: v for k, v in sd.items() if k in msd}, strict=False)
    assert torch.equal(m.token_embedding.weight, sd["token_embedding.weight"])
    m.eval()

    def feats(ids):
        t = torch.from_numpy(ids)
        with torch.no_grad():
            return m.encode_text(m.token_embedding(t), t).float().numpy()

    a_feat, b_feat = feats(a_ids), feats(b_ids)
    out = {"a_names": np.asarray(names), "a_templates": np.asarray(templates), "a_sentences": np.asarray(sentences),
           "a_ids": a_ids.astype(np.int32), "a_feat": a_feat, "a_W": ulip_rule(a_feat, [7] * 5),
           "b_ids": b_ids.astype(np.int32), "b_lens": lens.astype(np.int64),
           "b_offsets": np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), "b_feat": b_feat,
           "b_groups": np.asarray(B_GROUPS, np.int64), "b_W": ulip_rule(b_feat, B_GROUPS)}
    path = os.path.join(HERE, "g_zeroshot.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", names, [len(tk.encode(n.replace('_', ' '))) for n in names], lens.tolist())
    assert os.path.getsize(path) <= 256 * 1024


if __name__ == "__main__":
    main()
