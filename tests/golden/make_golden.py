#!/usr/bin/env python3
"""Generate the golden fixtures in tests/golden/ by running the UPSTREAM REFERENCE
(/root/reference, imported through tests/golden/ref_import.py) on deterministic synthetic
inputs and weights (ppt_amd.weights).  Build container only; the fixtures (data: inputs are
regenerated from seeds, expected outputs are stored) are committed, this script documents
how they were made.

    python tests/golden/make_golden.py            # rewrites tests/golden/*.npz, tests/golden/bpe_merges_subset.txt.gz
                                                  # and ppt_amd/data/classnames.json

While generating, every oracle function (oracle/oracle.py, oracle/ppt_oracle.c) is checked
against the reference output; the script aborts if the oracle is off.
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
from oracle import oracle as O             # noqa: E402

torch.set_num_threads(8)


def sets_equal_or_tied(ref_idx, ora_idx, kth):
    """neighbour sets equal, except rows whose k-th and (k+1)-th distances tie exactly."""
    a = np.sort(ref_idx, -1)
    b = np.sort(ora_idx, -1)
    bad = (a != b).any(-1)
    tied = kth[..., 0] == kth[..., 1]
    return int((bad & ~tied).sum()), int(bad.sum()), int(tied.sum())


def gen_tokens():
    labels = json.load(open(os.path.join(R.REF_ROOT, "data", "labels.json")))
    with R.reference_context():
        from utils.tokenizer import SimpleTokenizer
        tk = SimpleTokenizer()
        names = {}
        for ds, lst in labels.items():
            for n in lst:
                n2 = n.replace("_", " ")
                names[n2] = tk.encode(n2)
        out = {"_comment": "class lists = reference data/labels.json; token ids = reference "
                           "utils/tokenizer.py SimpleTokenizer.encode(name) captured by "
                           "tests/golden/make_golden.py (CLIP BPE; SURVEY.md §8(f) N3)",
               "sot": tk.encoder["<|startoftext|>"], "eot": tk.encoder["<|endoftext|>"],
               "placeholder": tk.encode("X")[0], "period": tk.encode(".")[0],
               "datasets": labels, "name_tokens": names}
        # sanity: full prompt tokenisation == our composition rule
        for n2, ids in list(names.items())[:20]:
            full = tk(" ".join(["X"] * 32) + " " + n2 + ".").tolist()
            mine = [out["sot"]] + [out["placeholder"]] * 32 + ids + [out["period"], out["eot"]]
            mine += [0] * (77 - len(mine))
            assert full == mine, n2
    os.makedirs(os.path.join(ROOT, "ppt_amd", "data"), exist_ok=True)
    with open(os.path.join(ROOT, "ppt_amd", "data", "classnames.json"), "w") as f:
        json.dump(out, f, indent=0)
    return out


# The strings tests/test_tokenizer_cpu.py encodes besides the class names of classnames.json (add any new one here).
BPE_TEXTS = ["X", ".", "a photo of a cat", "A  Photo\nof a CAT", "&amp;amp;", "&", "it's 42 tables, isn't it?", "a chair",
             "a table", "chair", "rocking horse", "lamp (floor)", "zebra crossing", "lamp (floor).", "zebra crossing."]


def gen_bpe_subset():
    """tests/golden/bpe_merges_subset.txt.gz: the CLIP merge table (1.3 MB, over the size of a committed file) cut down to
    what the tokenizer tests encode.  BPE on a piece only ever applies merges whose result is a substring of the piece (with
    its end-of-word mark), so every such merge keeps its line -- and with it its rank and its vocabulary id; every other line
    becomes a placeholder pair that can never match (its first symbol is no byte symbol) and whose token is unique."""
    import gzip
    from ppt_amd import tokenizer as T
    full = os.path.join(R.REF_ROOT, "utils", T.VOCAB_FILE)
    tk = T.SimpleTokenizer(full)
    names = list(json.load(open(os.path.join(ROOT, "ppt_amd", "data", "classnames.json")))["name_tokens"])
    texts = names + [n + "." for n in names] + BPE_TEXTS
    words = set()
    for t in texts:
        for piece in T._SPLIT.findall(tk.clean(t)):
            words.add("".join(tk.byte_sym[b] for b in piece.encode("utf-8")) + T.END)
    with gzip.open(full, "rt", encoding="utf-8") as f:
        lines = f.read().split("\n")
    out, kept = [lines[0]], 0
    for i, line in enumerate(lines[1:1 + T.N_MERGES]):
        a, b = line.split()
        if any(a + b in w for w in words):
            out.append(line)
            kept += 1
        else:
            out.append(f"␀ {i}")
    path = os.path.join(HERE, "bpe_merges_subset.txt.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:          # (mtime 0: the same bytes on every run)
        f.write("\n".join(out).encode("utf-8"))
    sub = T.SimpleTokenizer(path)
    for t in texts:
        assert sub.encode(t) == tk.encode(t), t
        assert sub(t).tolist() == tk(t).tolist(), t
    print(f"bpe subset: {kept} of {T.N_MERGES} merges kept, {os.path.getsize(path)} bytes")


def gen_index():
    """G1 FPS / G2 kNN / G3 ball-query fixtures from the reference's own functions."""
    out = {}
    with R.reference_context():
        from models.pointbert import misc, dvae
        from models.pointnet2 import pointnet2_utils as pn2
        cases = [("a", 4, 1024, False), ("b", 2, 2048, True), ("c", 1, 8192, False)]
        for tag, B, N, dup in cases:
            pc, start = W.synth_clouds(B, N, seed=1234, duplicates=dup)
            xyz = torch.from_numpy(pc)
            orig = torch.randint
            torch.randint = lambda *a, **k: torch.from_numpy(start)
            try:
                ref = misc.farthest_point_sample(xyz, 512).numpy()
            finally:
                torch.randint = orig
            ora = O.fps(pc, 512, start)
            assert np.array_equal(ref, ora), f"FPS oracle mismatch case {tag}"
            out[f"fps_{tag}_idx"] = ref.astype(np.int16)
            center = misc.index_points(xyz, torch.from_numpy(ref))
            for k in (32, 4):
                ridx = dvae.knn_point(k, xyz, center).numpy()
                oidx, kth = O.knn(pc, center.numpy(), k)
                hard, bad, tied = sets_equal_or_tied(ridx, oidx, kth)
                print(f"knn {tag} k={k}: set mismatches {bad} (tied rows {tied}, non-tied mismatches {hard})")
                assert hard == 0
                out[f"knn_{tag}_k{k}"] = np.sort(ridx, -1).astype(np.int16)
            # reference square_distance bit-identical to the C restatement
            rd = dvae.square_distance(center, xyz).numpy()
            od = O.square_distance(center.numpy(), pc)
            print(f"square_distance {tag}: bit-identical = {np.array_equal(rd, od)}, "
                  f"max|diff| = {np.abs(rd - od).max():.3e}, min = {rd.min():.3e}")
            assert np.array_equal(rd, od)
            if tag in ("a", "c"):
                for r, K in ((0.1, 16), (0.2, 32), (0.4, 128)):
                    rb = pn2.query_ball_point(r, K, xyz, center).numpy()
                    ob = O.ball_query(pc, center.numpy(), r, K)
                    assert np.array_equal(rb, ob), f"ball query mismatch {tag} r={r}"
                    out[f"ball_{tag}_r{r}_K{K}"] = rb.astype(np.int16)
        # dataset-side FPS (data/dataset_3d.py:40-61): numpy loop, random start injected; cloud with duplicates and 6 columns
        from data import dataset_3d as D3
        for tag, N, M, dup, cols in (("d", 8192, 1024, False, 3), ("e", 2048, 512, True, 6)):
            pc, start = W.synth_clouds(1, N, seed=4321, duplicates=dup)
            pts = pc[0].astype(np.float32)
            if cols == 6:
                pts = np.concatenate([pts, pts[:, ::-1] * 0.5], axis=1)
            orig_ri = np.random.randint
            np.random.randint = lambda *a, **k: int(start[0])
            try:
                ref = D3.farthest_point_sample(pts.copy(), M)
            finally:
                np.random.randint = orig_ri
            rows, idx = O.dataset_farthest_point_sample(pts, M, int(start[0]))
            assert np.array_equal(ref, rows), f"dataset FPS oracle mismatch case {tag}"
            # ... and the same walk as the tokenizer's FPS restatement (C oracle) on the fp32 coordinates
            assert np.array_equal(idx, O.fps(pts[None, :, :3], M, start[:1])[0]), tag
            out[f"dsfps_{tag}_idx"] = idx.astype(np.int16)
            out[f"dsfps_{tag}_start"] = np.int64(start[0])
    np.savez_compressed(os.path.join(HERE, "g_index.npz"), **out)
    print("g_index.npz:", {k: v.shape for k, v in out.items()})


def load_into_reference(m, sd, embedding):
    msd = m.state_dict()
    missing = [k for k in msd if k not in sd and k != "token_embedding.weight"]
    assert not missing, missing
    m.load_state_dict({k: v for k, v in sd.items() if k in msd}, strict=False)
    m.prompt_learner.embedding = embedding.clone()


def set_droppath(m, masks):
    """Force the stub DropPath modules (ref_import) to use injected per-sample factors."""
    for l, blk in enumerate(m.point_encoder.blocks.blocks):
        mk = masks[l]
        calls = {"n": 0}

        def fwd(x, mk=mk, calls=calls):
            f = mk[calls["n"] % 2]
            calls["n"] += 1
            return x * f.view(-1, 1, 1)
        blk.drop_path.forward = fwd


def gen_encoder_and_step(tok, head_types=(0, 1, 2, 3), profile=""):
    """profile "": the std-0.02 synthetic weights; "ckpt": the same train step on checkpoint-LIKE magnitudes
    (ppt_amd.weights.checkpoint_like: LayerNorm gains up to 10, outlier channels, 3 x larger weight matrices) -> g_step_h{n}_ckpt.npz."""
    names = tok["datasets"]["modelnet40"]
    name_lengths = [len(tok["name_tokens"][n.replace("_", " ")]) for n in names]
    sd = W.ulip_pointbert_state_dict(seed=0)
    if profile == "ckpt":
        sd = W.checkpoint_like(sd, seed=0)
    emb = W.synth_prompt_embedding(len(names), seed=0)
    B, N = 4, 1024
    pc_np, start = W.synth_clouds(B, N, seed=77)
    pc = torch.from_numpy(pc_np)
    rng = np.random.default_rng(5)
    labels = torch.from_numpy(rng.integers(0, len(names), size=(B,)))
    rates = np.linspace(0, 0.1, 12)
    masks = []
    for l in range(12):
        keep = 1.0 - rates[l]
        row = []
        for _ in range(2):
            row.append(torch.from_numpy((np.floor(keep + rng.random(B)) / keep).astype(np.float32)))
        masks.append(tuple(row))
    # make sure at least one sample is actually dropped somewhere (else the fixture is weak)
    masks[11] = (masks[11][0], torch.tensor([1 / 0.9, 0.0, 1 / 0.9, 1 / 0.9]))
    masks[6] = (torch.tensor([0.0, 1 / (1 - rates[6]), 1 / (1 - rates[6]), 1 / (1 - rates[6])], dtype=torch.float32), masks[6][1])

    for head_type in head_types:
        m = R.build_reference_ulip_pointbert(names, head_type=head_type)
        load_into_reference(m, sd, emb)
        eot = m.tokenized_prompts.argmax(-1).numpy()
        assert m.prompt_learner.name_lengths == name_lengths

        if head_type == 0 and not profile:
            # ---- G4: mini-PointNet in eval and train BN modes (dvae.py:184-215)
            cidx = O.fps(pc_np, 512, start)
            _, nb, ce = O.group(pc_np, cidx, 32)
            enc = {}
            for mode in ("eval", "train"):
                m.point_encoder.encoder.train(mode == "train")
                m.load_state_dict({k: v for k, v in sd.items() if "running" in k or "num_batches" in k}, strict=False)
                with torch.no_grad():
                    ref = m.point_encoder.encoder(torch.from_numpy(nb))
                ns = {}
                with torch.no_grad():
                    ora = O.mini_pointnet(sd, torch.from_numpy(nb), mode == "train", new_stats=ns)
                err = (ref - ora).abs().max().item()
                print(f"mini-PointNet {mode}: max|ref-oracle| = {err:.3e} (|ref|max {ref.abs().max():.3f})")
                assert err < 2e-4
                enc[f"{mode}_sub"] = ref[:, ::8].numpy()
                enc[f"{mode}_sum"] = np.float64(ref.double().sum().item())
                enc[f"{mode}_sqsum"] = np.float64((ref.double() ** 2).sum().item())
                if mode == "train":
                    msd = m.state_dict()
                    for k, v in ns.items():
                        r = msd[k]
                        e = (r.float() - v.float()).abs().max().item()
                        assert e < 1e-5, (k, e)
                        enc["stat_" + k] = r.numpy()
            np.savez_compressed(os.path.join(HERE, "g_encoder.npz"), **enc)
            m.load_state_dict({k: v for k, v in sd.items() if "running" in k or "num_batches" in k}, strict=False)

        # ---- G7: full train step (main_cls.py:179-214) with injected FPS starts + DropPath masks
        m.train()
        set_droppath(m, masks)
        opt = torch.optim.AdamW([p for p in m.parameters()], lr=3e-3, betas=(0.9, 0.98), eps=1e-8,
                                weight_decay=0.1)
        crit = torch.nn.CrossEntropyLoss(label_smoothing=0.2)
        orig = torch.randint
        torch.randint = lambda *a, **k: torch.from_numpy(start)
        try:
            opt.zero_grad()
            pred = m(pc)
            loss = crit(pred, labels)
            loss.backward(retain_graph=True)
        finally:
            torch.randint = orig
        grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.requires_grad}
        opt.step()
        newp = {k: p.detach().clone() for k, p in m.named_parameters() if p.requires_grad}
        msd = m.state_dict()

        res = O.train_step(sd, pc, labels, start, emb, name_lengths, eot, head_type=head_type,
                           dp_masks=masks)
        print(f"[h{head_type}] loss ref {loss.item():.6f} oracle {res['loss'].item():.6f}")
        e = (pred.detach() - res["logits"]).abs().max().item()
        print(f"[h{head_type}] logits max|diff| {e:.3e} (|logits|max {pred.abs().max().item():.2f})")
        assert e < (5e-3 if not profile else 5e-2) and abs(loss.item() - res["loss"].item()) < (1e-4 if not profile else 5e-3)
        assert sorted(grads) == sorted(res["grads"]), (sorted(grads), sorted(res["grads"]))
        fx = dict(logits=pred.detach().numpy(), loss=np.float32(loss.item()), labels=labels.numpy(),
                  eot=eot.astype(np.int16), fps_start=start,
                  dp_masks=np.stack([np.stack([a.numpy(), b.numpy()]) for a, b in masks]))
        for k in grads:
            g, go = grads[k], res["grads"][k]
            rel = ((g - go).norm() / (g.norm() + 1e-30)).item()
            # AdamW's first step is ~lr*sign(g): feed the oracle's update rule the REFERENCE gradient
            # so that the optimiser restatement is pinned tightly, independent of gradient noise.
            pe = (newp[k] - O.adamw_update(sd[k], g, {}, 3e-3)).abs().max().item()
            print(f"[h{head_type}] grad {k}: |g| {g.norm().item():.3e} rel.err {rel:.2e}; post-AdamW max|diff| {pe:.2e}")
            assert rel < (2e-3 if not profile else 2e-2) and pe < 1e-6
            if g.numel() <= 20000:
                fx["grad_" + k] = g.numpy()
                fx["new_" + k] = newp[k].numpy()
            else:       # big matrices: a strided sub-block + norms
                fx["gradsub_" + k] = g.flatten()[::97].numpy()
                fx["newsub_" + k] = newp[k].flatten()[::97].numpy()
                fx["gradnorm_" + k] = np.float64(g.double().norm().item())
        for k, v in res["new_stats"].items():
            ee = (msd[k].float() - v.float()).abs().max().item()
            assert ee < 1e-5, (k, ee)
            fx["stat_" + k] = msd[k].numpy()
        np.savez_compressed(os.path.join(HERE, f"g_step_h{head_type}{'_' + profile if profile else ''}.npz"), **fx)

        if head_type == 0 and not profile:
            # eval-mode forward (validate(), main_cls.py:237-299): running stats, no DropPath
            m.load_state_dict({k: v for k, v in sd.items()}, strict=False)
            m.prompt_learner.embedding = emb.clone()
            m.eval()
            for blk in m.point_encoder.blocks.blocks:
                blk.drop_path.forward = lambda x: x
            torch.randint = lambda *a, **k: torch.from_numpy(start)
            try:
                with torch.no_grad():
                    pe_feat = m.point_encoder(pc)
                    lg = m(pc)
                    prompts = m.prompt_learner()
                    te = m.encode_text(prompts, m.tokenized_prompts)
            finally:
                torch.randint = orig
            aux = {}
            with torch.no_grad():
                lo = O.ulip_logits(sd, pc, start, emb, name_lengths, eot, train=False, aux=aux)
                to = O.text_tower(sd, O.splice_prompts(emb, sd["prompt_learner.learnable_tokens"], name_lengths), eot)
            print("eval: pc_feat diff", (pe_feat - aux["pc_feat"]).abs().max().item(),
                  "text diff", (te - to).abs().max().item(), "logits diff", (lg - lo).abs().max().item())
            assert (pe_feat - aux["pc_feat"]).abs().max().item() < 1e-3
            assert (te - to).abs().max().item() < 1e-4
            np.savez_compressed(os.path.join(HERE, "g_eval.npz"), pc_feat=pe_feat.numpy(),
                                text_feat=te.numpy(), logits=lg.numpy(), prompts_sub=prompts[:, ::4, ::8].numpy())


def block_inputs():
    """Seeded inputs of the G5 / G6 fixtures (regenerated by the tests, not stored)."""
    g = torch.Generator().manual_seed(2024)
    x = torch.randn(2, 513, 384, generator=g) * 0.5
    pos = torch.randn(2, 513, 384, generator=g) * 0.1
    cot = torch.randn(2, 513, 384, generator=g)
    tcot = torch.randn(40, 512, generator=g)
    xt = torch.randn(37, 3, 512, generator=g) * 0.3            # [L, N, D] for one ResidualAttentionBlock call
    xtcot = torch.randn(37, 3, 512, generator=g)
    return x, pos, cot, tcot, xt, xtcot


def _sub(t, n=4099):
    """a strided sample (prime stride) + norm of a big tensor"""
    f = t.detach().flatten()
    step = max(1, f.numel() // n) | 1
    return f[::step].numpy(), np.float64(f.double().norm().item())


def gen_blocks(tok):
    """G5: one PointBERT Block forward / backward on [2,513,384] (point_encoder.py:76-79) plus its Mlp and Attention alone and
    the 12-block TransformerEncoder(x, pos) (:99-110);  G6: the text tower on the ModelNet40 prompts -> [40,512] with the gradient
    w.r.t. learnable_tokens (ULIP_models.py:203-222), and one ResidualAttentionBlock on [37,3,512] (:49-56)."""
    names = tok["datasets"]["modelnet40"]
    sd = W.ulip_pointbert_state_dict(seed=0)
    emb = W.synth_prompt_embedding(len(names), seed=0)
    m = R.build_reference_ulip_pointbert(names, head_type=3)
    load_into_reference(m, sd, emb)
    m.eval()                                         # DropPath off, no Dropout anywhere on these paths
    for p in m.parameters():
        p.requires_grad_(True)
    x, pos, cot, tcot, xt, xtcot = block_inputs()
    fx = {}
    blk = m.point_encoder.blocks.blocks[11]
    for name, fn in (("block", lambda t: blk(t)), ("mlp", lambda t: blk.mlp(t)), ("attn", lambda t: blk.attn(t)),
                     ("encoder", lambda t: m.point_encoder.blocks(t, pos))):
        m.zero_grad()
        xi = x.clone().requires_grad_(True)
        y = fn(xi)
        (y * cot).sum().backward()
        fx[f"{name}_y"], fx[f"{name}_ynorm"] = _sub(y)
        fx[f"{name}_dx"], fx[f"{name}_dxnorm"] = _sub(xi.grad)
        if name != "encoder":
            for k, p_ in blk.named_parameters():
                if p_.grad is not None and p_.grad.abs().sum() > 0:
                    fx[f"{name}_g_{k}"], fx[f"{name}_gn_{k}"] = _sub(p_.grad)
    part = m.point_encoder.blocks(x, pos, task='partseg')
    assert len(part) == 3
    fx["encoder_partseg_y3"], _ = _sub(part[0])
    # ---- G6
    m.zero_grad()
    prompts = m.prompt_learner()
    te = m.encode_text(prompts, m.tokenized_prompts)
    (te * tcot).sum().backward()
    fx["text_feat"] = te.detach().numpy()
    fx["text_gtok"] = m.prompt_learner.learnable_tokens.grad.numpy().copy()
    eot = m.tokenized_prompts.argmax(-1).numpy()
    with torch.no_grad():
        to = O.text_tower(sd, O.splice_prompts(emb, sd["prompt_learner.learnable_tokens"], m.prompt_learner.name_lengths), eot)
    e = (te.detach() - to).abs().max().item()
    print("G6 text tower: max|ref-oracle|", e)
    assert e < 1e-4
    rb = m.transformer.resblocks[0]
    m.zero_grad()
    xi = xt.clone().requires_grad_(True)
    rb.attn_mask = m.build_attention_mask()[:37, :37]
    y = rb(xi)
    (y * xtcot).sum().backward()
    fx["resblock_y"], fx["resblock_ynorm"] = _sub(y)
    fx["resblock_dx"], fx["resblock_dxnorm"] = _sub(xi.grad)
    for k, p_ in rb.named_parameters():
        fx[f"resblock_g_{k}"], fx[f"resblock_gn_{k}"] = _sub(p_.grad)
    np.savez_compressed(os.path.join(HERE, "g_blocks.npz"), **fx)
    print("g_blocks.npz:", len(fx), "arrays,", sum(v.nbytes for v in fx.values()) // 1024, "KiB")


def gen_pointnet2_msg():
    """G-PN2: Pointnet2_Msg forward (eval and train BN) vs the reference module (pointnet2.py:40-73)."""
    sd_all = W.synth_state_dict(W.pointnet2_msg_spec(prefix=""), seed=0)
    B, N = 2, 1024
    pc_np, s1 = W.synth_clouds(B, N, seed=31)
    _, s2 = W.synth_clouds(B, 512, seed=32)
    pc = torch.from_numpy(pc_np)
    rng = np.random.default_rng(9)
    dm = (torch.from_numpy((rng.random((B, 512)) > 0.4).astype(np.float32) / 0.6),
          torch.from_numpy((rng.random((B, 256)) > 0.5).astype(np.float32) / 0.5))
    with R.reference_context():
        from models.pointnet2.pointnet2 import Pointnet2_Msg
        m = Pointnet2_Msg()
    m.load_state_dict(sd_all)
    out = {}
    for mode in ("eval", "train"):
        m.load_state_dict(sd_all)
        m.train(mode == "train")
        if mode == "train":
            m.drop1.forward = lambda x: x * dm[0]
            m.drop2.forward = lambda x: x * dm[1]
        starts = [torch.from_numpy(s1), torch.from_numpy(s2)]
        orig = torch.randint
        torch.randint = lambda *a, **k: starts.pop(0)
        try:
            with torch.no_grad():
                ref = m(pc)
        finally:
            torch.randint = orig
        ns = {}
        with torch.no_grad():
            ora = O.pointnet2_msg(sd_all, pc, (s1, s2), train=(mode == "train"), drop_masks=dm if mode == "train" else None,
                                  prefix="", new_stats=ns)
        err = (ref - ora).abs().max().item()
        print(f"Pointnet2_Msg {mode}: max|ref-oracle| = {err:.3e} (|ref|max {ref.abs().max():.3f})")
        assert err < 1e-3
        out[mode] = ref.numpy()
        if mode == "train":
            msd = m.state_dict()
            for k, v in ns.items():
                e = (msd[k].float() - v.float()).abs().max().item()
                assert e < 1e-4 * max(1.0, msd[k].float().abs().max().item()), (k, e)
            for k in ("sa1.bn_blocks.2.2.running_var", "sa2.bn_blocks.1.0.running_mean", "sa3.mlp_bns.2.running_var",
                      "bn2.running_mean"):
                out["stat_" + k] = msd[k].numpy()
    out["drop1"], out["drop2"] = dm[0].numpy(), dm[1].numpy()
    out["start1"], out["start2"] = s1, s2
    np.savez_compressed(os.path.join(HERE, "g_pn2msg.npz"), **out)


def gen_pointnet2_ssg():
    """G-PN2S: Pointnet2_Ssg forward (eval and train BN) vs the reference module (pointnet2.py:6-38)."""
    sd_all = W.synth_state_dict(W.pointnet2_ssg_spec(prefix=""), seed=0)
    B, N = 2, 1024
    pc_np, s1 = W.synth_clouds(B, N, seed=41)
    _, s2 = W.synth_clouds(B, 512, seed=42)
    pc = torch.from_numpy(pc_np)
    rng = np.random.default_rng(19)
    dm = (torch.from_numpy((rng.random((B, 512)) > 0.4).astype(np.float32) / 0.6),
          torch.from_numpy((rng.random((B, 256)) > 0.4).astype(np.float32) / 0.6))
    with R.reference_context():
        from models.pointnet2.pointnet2 import Pointnet2_Ssg
        m = Pointnet2_Ssg()
    out = {}
    for mode in ("eval", "train"):
        m.load_state_dict(sd_all)
        m.train(mode == "train")
        if mode == "train":
            m.drop1.forward = lambda x: x * dm[0]
            m.drop2.forward = lambda x: x * dm[1]
        starts = [torch.from_numpy(s1), torch.from_numpy(s2)]
        orig = torch.randint
        torch.randint = lambda *a, **k: starts.pop(0)
        try:
            with torch.no_grad():
                ref = m(pc)
        finally:
            torch.randint = orig
        ns = {}
        with torch.no_grad():
            ora = O.pointnet2_ssg(sd_all, pc, (s1, s2), train=(mode == "train"), drop_masks=dm if mode == "train" else None,
                                  prefix="", new_stats=ns)
        err = (ref - ora).abs().max().item()
        print(f"Pointnet2_Ssg {mode}: max|ref-oracle| = {err:.3e} (|ref|max {ref.abs().max():.3f})")
        assert err < 1e-3
        out[mode] = ref.numpy()
        if mode == "train":
            msd = m.state_dict()
            for k, v in ns.items():
                e = (msd[k].float() - v.float()).abs().max().item()
                assert e < 1e-4 * max(1.0, msd[k].float().abs().max().item()), (k, e)
            for k in ("sa1.mlp_bns.2.running_var", "sa2.mlp_bns.0.running_mean", "sa3.mlp_bns.2.running_var", "bn2.running_mean"):
                out["stat_" + k] = msd[k].numpy()
    out["drop1"], out["drop2"] = dm[0].numpy(), dm[1].numpy()
    out["start1"], out["start2"] = s1, s2
    np.savez_compressed(os.path.join(HERE, "g_pn2ssg.npz"), **out)


def gen_pointmlp():
    """G-PMLP: pointMLP() forward (eval and train BN) vs the reference module (pointMLP.py:359-363, 320-334)."""
    sd_all = W.synth_state_dict(W.pointmlp_spec(prefix=""), seed=0)
    B, N = 2, 1024
    pc_np, s1 = W.synth_clouds(B, N, seed=61)
    starts_np = [s1] + [W.synth_clouds(B, n, seed=62 + i)[1] for i, n in enumerate((512, 256, 128))]
    pc = torch.from_numpy(pc_np)
    rng = np.random.default_rng(23)
    dm = (torch.from_numpy((rng.random((B, 512)) > 0.5).astype(np.float32) / 0.5),
          torch.from_numpy((rng.random((B, 256)) > 0.5).astype(np.float32) / 0.5))
    with R.reference_context():
        from models.pointmlp.pointMLP import pointMLP
        m = pointMLP()
    out = {}
    for mode in ("eval", "train"):
        m.load_state_dict(sd_all)
        m.train(mode == "train")
        if mode == "train":
            m.classifier[3].forward = lambda x: x * dm[0]
            m.classifier[7].forward = lambda x: x * dm[1]
        starts = [torch.from_numpy(s) for s in starts_np]
        orig = torch.randint
        torch.randint = lambda *a, **k: starts.pop(0)
        try:
            with torch.no_grad():
                ref = m(pc.permute(0, 2, 1).contiguous().permute(0, 2, 1))       # Model.forward takes [B,N,3] (:321-322)
        finally:
            torch.randint = orig
        assert not starts
        ns = {}
        with torch.no_grad():
            ora = O.pointmlp(sd_all, pc, starts_np, train=(mode == "train"), drop_masks=dm if mode == "train" else None,
                             prefix="", new_stats=ns)
        err = (ref - ora).abs().max().item()
        print(f"pointMLP {mode}: max|ref-oracle| = {err:.3e} (|ref|max {ref.abs().max():.3f})")
        assert err < 1e-3
        out[mode] = ref.numpy()
        if mode == "train":
            msd = m.state_dict()
            for k, v in ns.items():
                e = (msd[k].float() - v.float()).abs().max().item()
                assert e < 1e-4 * max(1.0, msd[k].float().abs().max().item()), (k, e)
            for k in ("embedding.net.1.running_var", "pre_blocks_list.0.transfer.net.1.running_mean",
                      "pre_blocks_list.2.operation.1.net2.1.running_var", "pos_blocks_list.3.operation.0.net1.1.running_mean",
                      "classifier.5.running_mean"):
                out["stat_" + k] = msd[k].numpy()
    out["drop1"], out["drop2"] = dm[0].numpy(), dm[1].numpy()
    for i, s in enumerate(starts_np):
        out[f"start{i + 1}"] = s
    np.savez_compressed(os.path.join(HERE, "g_pointmlp.npz"), **out)


def gen_partseg(tok):
    """G8: ULIP_PointBERT_partseg train step (main_partseg.py:204-215) on B=2 x 2048 points with duplicates."""
    import argparse
    names = tok["datasets"]["shapenetpart"]
    name_lengths = [len(tok["name_tokens"][n.replace("_", " ")]) for n in names]
    sd = W.ulip_partseg_state_dict(seed=0)
    emb = W.synth_prompt_embedding(len(names), seed=0)
    B, N = 2, 2048
    pc_np, s0 = W.synth_clouds(B, N, seed=55, duplicates=True)
    _, s1 = W.synth_clouds(B, N, seed=56)
    _, s2 = W.synth_clouds(B, N, seed=57)
    pc = torch.from_numpy(pc_np)
    rng = np.random.default_rng(6)
    onehot = torch.zeros(B, 16)
    onehot[0, 3] = 1
    onehot[1, 11] = 1
    labels = torch.from_numpy(rng.integers(0, 50, size=(B, N)))
    masks = [(torch.from_numpy((np.floor(0.95 + rng.random(B)) / 0.95).astype(np.float32)),
              torch.from_numpy((np.floor(0.95 + rng.random(B)) / 0.95).astype(np.float32))) for _ in range(12)]
    drop = torch.from_numpy((rng.random((B, N, 128)) > 0.5).astype(np.float32) * 2.0)
    with R.reference_context():
        import models.ULIP_models as M
        from models.pointbert.point_encoder import PointTransformer_partseg
        cfg = M.cfg_from_yaml_file("./models/pointbert/PointTransformer_8192point.yaml")
        pe = PointTransformer_partseg(cfg.model, args=argparse.Namespace())
        m = M.ULIP_WITH_IMAGE(embed_dim=512, point_encoder=pe, context_length=77, vocab_size=49408, classnames=names,
                              template_init="", class_name_position="middle", num_learnable_prompt_tokens=32,
                              transformer_width=512, transformer_heads=8, transformer_layers=12, pc_feat_dims=128, device=0,
                              task="partseg")
    backbone = {k for k, _ in W.pointbert_spec()}
    for name, param in m.named_parameters():        # ULIP_models.py:550-565: backbone + text tower frozen, decoder + prompt train
        if name.startswith("prompt_learner") or (name.startswith("point_encoder.") and name not in backbone):
            continue
        param.requires_grad = False
    load_into_reference(m, sd, emb)
    eot = m.tokenized_prompts.argmax(-1).numpy()
    m.train()
    set_droppath(m, masks)
    pe.drop1.forward = lambda x: x * drop.permute(0, 2, 1)
    starts = [torch.from_numpy(s0), torch.from_numpy(s1), torch.from_numpy(s2)]
    orig = torch.randint
    torch.randint = lambda *a, **k: starts.pop(0)
    try:
        pred = m(pc, onehot)
        loss = torch.nn.CrossEntropyLoss(label_smoothing=0.2)(pred.reshape(-1, 50), labels.reshape(-1))
        loss.backward()
    finally:
        torch.randint = orig
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.requires_grad and p.grad is not None}
    nograd = [k for k, p in m.named_parameters() if p.requires_grad and p.grad is None]
    print("trainable without grad (unused in forward):", nograd)

    sd2 = dict(sd)
    keys = sorted(grads)
    for k in keys:
        sd2[k] = sd[k].detach().clone().requires_grad_(True)
    ns = {}
    lo = O.partseg_logits(sd2, pc, onehot, (s0, s1, s2), emb, name_lengths, eot, train=True, dp_masks=masks, drop_mask=drop,
                          new_stats=ns)
    lo_loss = O.cross_entropy_ls(lo.reshape(-1, 50), labels.reshape(-1), 0.2)
    og = torch.autograd.grad(lo_loss, [sd2[k] for k in keys])
    e = (pred.detach() - lo.detach()).abs().max().item()
    print(f"partseg logits max|ref-oracle| {e:.3e} (|logits|max {pred.abs().max().item():.2f}); loss {loss.item():.6f} vs {lo_loss.item():.6f}")
    assert e < 2e-2 and abs(loss.item() - lo_loss.item()) < 1e-4
    fx = dict(logits_sub=pred.detach()[:, ::16].numpy(), loss=np.float32(loss.item()), labels=labels.numpy().astype(np.int16),
              eot=eot.astype(np.int16), s0=s0, s1=s1, s2=s2, onehot=onehot.numpy(),
              dp_masks=np.stack([np.stack([a.numpy(), b.numpy()]) for a, b in masks]), drop=np.packbits(drop.numpy() > 0))
    for k, g in zip(keys, og):
        rel = ((grads[k] - g).norm() / (grads[k].norm() + 1e-30)).item()
        print(f"  grad {k}: |g| {grads[k].norm().item():.3e} rel.err {rel:.2e}")
        # a bias in front of BatchNorm has zero gradient (noise only); BN-adjacent sums cancel heavily -> 3e-2
        assert rel < 3e-2 or grads[k].norm().item() < 1e-4, k
        fx["gradnorm_" + k] = np.float64(grads[k].double().norm().item())
        fx["gradsub_" + k] = grads[k].flatten()[::211].numpy()
    msd = m.state_dict()
    for k in ("point_encoder.propagation_0.mlp_bns.1.running_var", "point_encoder.bn1.running_mean"):
        assert (msd[k] - ns[k]).abs().max().item() < 1e-4
        fx["stat_" + k] = msd[k].numpy()
    fx["trainable"] = np.array(sorted(k for k, p in m.named_parameters() if p.requires_grad))
    np.savez_compressed(os.path.join(HERE, "g_partseg.npz"), **fx)


if __name__ == "__main__":
    assert R.reference_available(), "needs /root/reference"
    O.build_c_oracle(force=True)
    import sys
    if sys.argv[1:] == ["pn2ssg"]:              # one fixture only
        gen_pointnet2_ssg()
    elif sys.argv[1:] == ["pointmlp"]:
        gen_pointmlp()
    elif sys.argv[1:] == ["index"]:
        gen_index()
    elif sys.argv[1:] == ["bpe"]:
        gen_bpe_subset()
    elif sys.argv[1:] == ["blocks"]:
        gen_blocks(gen_tokens())
    elif sys.argv[1:2] == ["steps"]:            # the train-step fixtures of the given head_types only
        gen_encoder_and_step(gen_tokens(), tuple(int(h) for h in sys.argv[2:]))
    elif sys.argv[1:2] == ["ckpt"]:             # ... on checkpoint-like weight magnitudes (VERDICT r4 #4b)
        gen_encoder_and_step(gen_tokens(), tuple(int(h) for h in sys.argv[2:]) or (0, 3), profile="ckpt")
    else:
        tok = gen_tokens()
        gen_bpe_subset()
        gen_index()
        gen_encoder_and_step(tok)
        gen_encoder_and_step(tok, (0, 3), profile="ckpt")
        gen_pointnet2_msg()
        gen_pointnet2_ssg()
        gen_pointmlp()
        gen_partseg(tok)
        gen_blocks(tok)
    print("done")
