"""GPU: zero-shot classification (ppt_amd/zeroshot.py) -- the sentence-rows kernel, the ragged causal attention, the template
ensemble and the cosine head against torch / fp64, and encode_sentences / classifier against the reference's features
(tests/golden/g_zeroshot.npz, made by tests/golden/make_golden_zeroshot.py).

Bounds: attention, maximum absolute error against fp64 softmax attention of each sentence alone 2e-5 (fp32 operands) / 3e-3 (f16)
/ 2e-2 (bf16) -- those of tests/test_kernels_gpu.py -- and half of them against ops.attention_fwd on the sentence alone;
encode_sentences and classifier, relative L2 against the reference 2e-4 in "fp32" and "split16", 3e-2 in "mixed16" (those
tests/test_blocks_gpu.py holds encode_text to)."""
import contextlib
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ppt_amd import weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "g_zeroshot.npz"))
B_LENS = G["b_lens"].tolist()
FORMS = {"f32": (torch.float32, 2e-5), "f16": (torch.float16, 3e-3), "bf16": (torch.bfloat16, 2e-2)}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ppt_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def model():
    from ppt_amd.models import ULIP_models as M
    args = SimpleNamespace(classnames=M.dataset_classnames("modelnet40"), template_init='', class_name_position='middle',
                           num_learnable_prompt_tokens=32, gpu=0, task='cls', head_type=0, evaluate_3d=False, ulip2=False,
                           synthetic_weights=True)
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.ULIP_PointBERT(args)
    m.load_state_dict(W.ulip_pointbert_state_dict(seed=0, with_token_embedding=True), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding(len(args.classnames), seed=0)
    m.cuda().eval()
    return m


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


# ------------------------------------------------------------------ sentence rows
@pytest.mark.parametrize("case", ["one", "set_b", "pad32", "pad64", "pad128"])
def test_sentence_rows_bit_exact(ops, case):
    rng = np.random.default_rng(5)
    vocab, Wd = 1000, 512
    table = torch.from_numpy(rng.standard_normal((vocab, Wd)).astype(np.float32)).cuda()
    pos = torch.from_numpy(rng.standard_normal((77, Wd)).astype(np.float32)).cuda()
    lens = [9] if case == "one" else B_LENS
    ids = np.zeros((len(lens), 77), np.int64)
    for s, n in enumerate(lens):
        ids[s, :n] = rng.integers(0, vocab, size=n)
    off = _offsets(lens)
    M = int(off[-1])                                                       # 9, or 418 = 13 * 32 + 2
    mult = {"pad32": 32, "pad64": 64, "pad128": 128}.get(case, 1)
    rows = (M + mult - 1) // mult * mult
    assert mult == 1 or rows > M
    out = ops.sentence_rows(table, pos, torch.from_numpy(ids.astype(np.int32)).cuda(), torch.from_numpy(off).cuda(), rows)
    sent = np.repeat(np.arange(len(lens)), lens)
    p = np.arange(M) - off[sent]
    want = table[torch.from_numpy(ids[sent, p]).cuda()] + pos[torch.from_numpy(p).cuda()]
    assert out.shape == (rows, Wd) and torch.equal(out[:M], want)
    assert not out[M:].any()                                               # the padding rows come back zero


# ------------------------------------------------------------------ ragged attention
def _attn_ref64(qkv, lens, H):
    """fp64 softmax attention of every sentence alone (tests/test_kernels_gpu.py: _attn_ref, causal, scale 0.125)"""
    out, a0 = [], 0
    for n in lens:
        q, k, v = qkv[a0:a0 + n].double().view(n, 3, H, 64).permute(1, 2, 0, 3)
        a = (q @ k.transpose(-2, -1)) * 0.125 + torch.full((n, n), float("-inf"), dtype=torch.float64).triu(1)
        out.append((torch.softmax(a, -1) @ v).transpose(0, 1).reshape(n, H * 64))
        a0 += n
    return torch.cat(out)


LAYOUTS = {"one_len2": ([2], 8, 0), "one_len77": ([77], 8, 0), "set_b": (B_LENS, 8, 0),
           "many300": (np.random.default_rng(3).integers(6, 14, size=300).tolist(), 2, 0), "padded": ([5, 64, 70, 13, 16], 3, 27)}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("form", list(FORMS))
def test_ragged_attention(ops, form, layout, monkeypatch):
    dtype, tol = FORMS[form]
    lens, H, pad = LAYOUTS[layout]
    off = _offsets(lens)
    M = int(off[-1])
    rng = np.random.default_rng(M + H)
    qkv = torch.from_numpy(rng.standard_normal((M + pad, 3 * H * 64)).astype(np.float32)).cuda().to(dtype)
    off_d = torch.from_numpy(off).cuda()
    plan = torch.from_numpy(ops.ragged_attention_plan(lens)).cuda()
    if layout == "many300":
        assert plan.numel() // 64 * H > 2 * 4                                 # more (bin, head) pairs than a few workgroups take
    out = ops.attention_ragged_fwd(qkv, off_d, H, 0.125, plan=plan)
    assert out.shape == (M + pad, H * 64) and out.dtype == dtype
    ref = _attn_ref64(qkv.float().cpu(), lens, H)
    err = (out[:M].double().cpu() - ref).abs().max().item()
    # ... and the project's own kernels on each sentence alone (fp32: the VALU kernel, then the split16 one)
    def alone():
        return torch.cat([ops.attention_fwd(qkv[a:b].contiguous(), 1, int(b - a), H, 0.125, True, want_lse=False)[0]
                          for a, b in zip(off[:-1], off[1:])])

    monkeypatch.setattr(ops, "_SPLIT16", False)                                # (restored when the test ends)
    ref_alone = alone()
    err2 = (out[:M].float() - ref_alone.float()).abs().max().item()
    print(f"PARITY ragged attention {form} {layout}: vs fp64 {err:.3g} (bound {tol:.3g}), vs attention_fwd {err2:.3g} (bound {tol / 2:.3g})")
    assert err < tol and err2 < tol / 2
    # the same arithmetic as the streaming kernel on the sentence alone: the same BITS (16-bit forms: ppt_attention_fwd; fp32:
    # ppt_attention_fwd_split16, whose hi + lo products the ragged kernel's PPT_F32 form uses)
    if form == "f32":
        monkeypatch.setattr(ops, "_SPLIT16", True)
        monkeypatch.setattr(ops, "ATTN_SPLIT16", True)
        ref_alone = alone()
    assert torch.equal(out[:M], ref_alone)
    again = ops.attention_ragged_fwd(qkv, off_d, H, 0.125, plan=plan)
    assert torch.equal(again[:M], out[:M])                                     # deterministic
    auto = ops.attention_ragged_fwd(qkv, off_d, H, 0.125)                      # the plan built from the offsets
    assert torch.equal(auto[:M], out[:M])


# ------------------------------------------------------------------ ensemble, head
@pytest.mark.parametrize("groups", [(1, 4, 7), (64,) * 40])
def test_template_ensemble_against_fp64(ops, groups):
    rng = np.random.default_rng(len(groups))
    feat = torch.from_numpy((rng.standard_normal((sum(groups), 512)) * rng.uniform(0.5, 3.0, size=(sum(groups), 1))).astype(np.float32))
    goff = torch.from_numpy(_offsets(groups))
    Wd = ops.template_ensemble(feat.cuda(), goff.cuda())
    f = feat.double() / feat.double().norm(dim=-1, keepdim=True)
    want = torch.stack([f[a:b].mean(0) for a, b in zip(goff[:-1].tolist(), goff[1:].tolist())])
    want = want / want.norm(dim=-1, keepdim=True)
    err = (Wd.double().cpu() - want).abs().max().item()
    print(f"PARITY template ensemble {len(groups)} classes: {err:.3g} (bound 1e-6)")
    assert err <= 1e-6
    assert torch.equal(ops.template_ensemble(feat.cuda(), goff.cuda()), Wd)


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("C", [3, 40])
def test_cosine_head_against_fp64(ops, B, C):
    rng = np.random.default_rng(B + C)
    f = torch.from_numpy((rng.standard_normal((B, 512)) * 4).astype(np.float32))
    Wc = torch.from_numpy(rng.standard_normal((C, 512)).astype(np.float32))
    Wc = Wc / Wc.norm(dim=-1, keepdim=True)
    ls = torch.tensor(np.log(1 / 0.07), dtype=torch.float32)
    got = ops.cosine_head(f.cuda(), Wc.cuda(), ls.cuda())
    scale = ls.double().exp().item()
    want = scale * (f.double() / f.double().norm(dim=-1, keepdim=True)) @ Wc.double().t()
    err = (got.double().cpu() - want).abs().max().item() / scale
    print(f"PARITY cosine head B={B} C={C}: {err:.3g} of exp(logit_scale) (bound 1e-5)")
    assert got.shape == (B, C) and err <= 1e-5


# ------------------------------------------------------------------ the tower
@pytest.mark.parametrize("precision,tol", [("fp32", 2e-4), ("split16", 2e-4), ("mixed16", 3e-2)])
def test_encode_sentences_and_classifier_match_the_reference(model, precision, tol):
    from ppt_amd import zeroshot as Z
    model.set_precision(precision)
    for which, groups in (("a", [7] * 5), ("b", G["b_groups"].tolist())):
        ids = torch.from_numpy(G[which + "_ids"]).long()
        feat = model.encode_sentences(ids)
        ref = torch.from_numpy(G[which + "_feat"]).cuda()
        assert feat.shape == ref.shape and feat.dtype == torch.float32
        rel = _rel(feat, ref)
        Wc = Z.classifier(model, ids, groups)
        relw = _rel(Wc, torch.from_numpy(G[which + "_W"]).cuda())
        print(f"PARITY zeroshot {precision} set {which}: features rel {rel:.3g}, classifier rel {relw:.3g} (bound {tol:.3g})")
        assert rel < tol and relw < tol
    # set (B) in three chunks: 160 rows hold sentences 0-2 (64 + 65 + 31), then 3-8, then 9-11
    lens, _ = Z.ragged_layout(G["b_ids"])
    assert lens[:3].sum() == 160 and lens[3:9].sum() <= 160 < lens[3:10].sum() and lens[9:].sum() <= 160
    ids = torch.from_numpy(G["b_ids"]).long()
    whole, chunked = model.encode_sentences(ids), model.encode_sentences(ids, max_rows=160)
    if precision == "fp32":
        assert torch.equal(whole, chunked)                 # chunking changes no sentence's arithmetic
    else:
        assert _rel(chunked, torch.from_numpy(G["b_feat"]).cuda()) < tol


def test_zeroshot_module_and_validate(ops, model):
    from ppt_amd import evaluate
    from ppt_amd import zeroshot as Z
    model.set_precision("mixed16")
    names = [str(n) for n in G["a_names"]]
    Wc = Z.classifier(model, G["a_ids"], [7] * 5)
    zs = Z.ZeroShot(model, Wc, names)
    pc, start = W.synth_clouds(8, 1024, seed=77)
    pc = torch.from_numpy(pc).cuda()
    model.point_encoder.fps_start = torch.from_numpy(start[:4]).cuda()
    try:
        batches = [pc[:4].contiguous(), pc[4:].contiguous()]
        with torch.no_grad():
            want = [ops.cosine_head(model.encode_pc(b).float().contiguous(), Wc, model.logit_scale.detach()) for b in batches]
        got = [zs(b) for b in batches]
        assert got[0].shape == (4, 5) and all(torch.equal(g, w) for g, w in zip(got, want))
        labels = [torch.tensor([0, 1, 2, 3]), torch.tensor([4, 0, 1, 1])]
        args = SimpleNamespace(gpu=0, classnames=names)
        with contextlib.redirect_stdout(io.StringIO()):
            out = evaluate.validate(list(zip(batches, labels)), zs, torch.nn.CrossEntropyLoss(), args)
            out2 = Z.zeroshot_validate(list(zip(batches, labels)), model, G["a_ids"], [7] * 5, args)
    finally:
        model.point_encoder.fps_start = None
    pred = torch.cat(got).argmax(-1).cpu()
    acc = (pred == torch.cat(labels)).float().mean().item()                   # validate() reports the fraction
    assert abs(out["acc"] - acc) < 1e-6 and out["n"] == 8 and set(out["per_class_acc"]) <= set(names)
    assert abs(out2["acc"] - acc) < 1e-6 and abs(out2["loss"] - out["loss"]) < 1e-6


def test_errors_are_raised_before_anything_is_launched(ops, model):
    from ppt_amd import zeroshot as Z
    model.set_precision("fp32")
    ids = G["a_ids"][:3].astype(np.int64).copy()
    launches = []
    real = ops._lib.check
    ops._lib.check = lambda code, what="": (launches.append(what), real(code, what))[1]
    try:
        bad = ids.copy()
        bad[1, 2] = 49408
        with pytest.raises(ValueError):
            model.encode_sentences(bad)
        bad[1, 2] = -1
        with pytest.raises(ValueError):
            model.encode_sentences(bad)
        with pytest.raises(ValueError):
            model.encode_sentences(np.zeros((0, 77), np.int64))
        with pytest.raises(ValueError):
            model.encode_sentences([])
        with pytest.raises(ValueError):
            Z.classifier(model, ids, [2, 0, 1])
        with pytest.raises(ValueError):
            model.encode_sentences(ids, max_rows=3)
        assert launches == []
    finally:
        ops._lib.check = real
    off = torch.from_numpy(_offsets([4]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.attention_ragged_fwd(torch.zeros(4, 3 * 64), off, 1, 0.125)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sentence_rows(torch.zeros(10, 8), torch.zeros(77, 8), torch.zeros(1, 77, dtype=torch.int32), off, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.template_ensemble(torch.zeros(4, 8), off)
    with pytest.raises(RuntimeError, match="no CPU path"):
        Z.ZeroShot(model, torch.zeros(5, 512).cuda())(torch.zeros(1, 1024, 3))


def test_cli_scores_the_model_the_checkpoints_hold(tmp_path, monkeypatch):
    """main(): the weights of the model it validates are the checkpoint files' (the reference's on-disk layout, as
    tests/test_surface_cpu.py writes it; --ulip2 selects pointbert_ulip2.pt), not an initialisation; it returns validate()'s figures."""
    from ppt_amd import zeroshot as Z
    sd = W.ulip_pointbert_state_dict(seed=1, with_token_embedding=True)
    sd["logit_scale"] = sd["logit_scale"].reshape(())                                 # (the parameter is 0-dim)
    point = {"module." + k: v for k, v in sd.items() if k.startswith("point_encoder.") or k == "pc_projection"}
    slip = {"module." + k: v for k, v in sd.items() if "module." + k not in point}
    slip["module.pc_projection"] = torch.full_like(sd["pc_projection"], 9.0)          # the point checkpoint must win
    os.makedirs(tmp_path / "data" / "pretrained_models")
    os.makedirs(tmp_path / "data" / "initialize_models")
    torch.save({"state_dict": point}, tmp_path / "data" / "pretrained_models" / "pointbert_ulip2.pt")
    torch.save({"state_dict": slip}, tmp_path / "data" / "initialize_models" / "slip_base_100ep.pt")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("PPT_SYNTHETIC_WEIGHTS", raising=False)
    ids = np.concatenate([G["a_ids"], G["b_ids"][:5]])
    np.savez(tmp_path / "ids.npz", token_ids=ids, group_sizes=np.ones(40, np.int64))
    pc, _ = W.synth_clouds(6, 1024, seed=9)
    np.savez(tmp_path / "test.npz", points=pc.astype(np.float32), labels=np.asarray([0, 7, 39, 7, 1, 2]))
    seen = {}
    real = Z.zeroshot_validate
    monkeypatch.setattr(Z, "zeroshot_validate", lambda loader, model, *a, **k: (seen.update(model=model), real(loader, model, *a, **k))[1])
    argv = ["--test", str(tmp_path / "test.npz"), "--token_ids", str(tmp_path / "ids.npz"), "--npoints", "1024", "--batch_size", "4"]
    with pytest.raises(FileNotFoundError):                                            # pointbert.pt is not there
        Z.main(argv)
    with contextlib.redirect_stdout(io.StringIO()):
        out = Z.main(argv + ["--ulip2"])
    got = {k: v.detach().cpu() for k, v in seen["model"].state_dict().items()}
    for k in ("token_embedding.weight", "positional_embedding", "text_projection", "pc_projection", "logit_scale",
              "transformer.resblocks.11.mlp.c_proj.weight", "point_encoder.blocks.blocks.11.mlp.fc2.weight",
              "point_encoder.encoder.first_conv.0.weight"):
        assert torch.equal(got[k], sd[k]), k
    assert out["n"] == 6 and 0.0 <= out["acc"] <= 1.0 and np.isfinite(out["loss"]) and out["nonfinite_rows"] == 0
