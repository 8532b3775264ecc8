"""CPU: the host side of ppt_amd/zeroshot.py -- sentence building, the ragged layout and its EOT rule, the attention bin plan -- and
the fixture tests/golden/g_zeroshot.npz itself: the oracle's text tower, pooled at each sentence's own EOT, reproduces the
reference's features (tests/golden/make_golden_zeroshot.py), so the fixture is the reference's and the variable-EOT rule is the
one ULIP_models.py:219 applies."""
import os

import numpy as np
import pytest
import torch

from ppt_amd import ops, weights as W, zeroshot as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "g_zeroshot.npz"))
SOT, EOT = 49406, 49407


def test_ragged_layout_returns_the_stored_lengths_and_offsets():
    lens, off = Z.ragged_layout(G["b_ids"])
    assert np.array_equal(lens, G["b_lens"]) and np.array_equal(off, G["b_offsets"])
    assert sorted(lens.tolist()) == [2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 77]
    lens_t, off_t = Z.ragged_layout(torch.from_numpy(G["b_ids"]).long())            # the tokenizer returns a torch tensor
    assert np.array_equal(lens_t, lens) and np.array_equal(off_t, off)
    la, _ = Z.ragged_layout(G["a_ids"])
    assert all(G["a_ids"][s, n - 1] == EOT for s, n in enumerate(la))


def test_truncated_sentence_without_eot_takes_the_first_maximum():
    ids = np.zeros((2, 77), np.int64)
    ids[0] = 1000
    ids[0, 0] = SOT                     # no EOT: the tokenizer cut at 77; the start token is the largest id, at position 0
    ids[1] = 7
    ids[1, [5, 9]] = 40000              # the largest id twice: the first one counts (torch.argmax, ULIP_models.py:219)
    lens, off = Z.ragged_layout(ids)
    assert lens.tolist() == [1, 6] and off.tolist() == [0, 1, 7]
    assert lens.tolist() == (torch.from_numpy(ids).argmax(-1) + 1).tolist()


def test_build_sentences_is_class_major():
    s, sizes = Z.build_sentences(["night_stand", "bed"], ["a {}.", "the {} here", "{}"])
    assert s == ["a night stand.", "the night stand here", "night stand", "a bed.", "the bed here", "bed"]
    assert sizes == [3, 3]
    s, sizes = Z.build_sentences([str(n) for n in G["a_names"]], [str(t) for t in G["a_templates"]])
    assert s == [str(x) for x in G["a_sentences"]] and sizes == [7] * 5
    with pytest.raises(ValueError):
        Z.build_sentences([], ["a {}"])


def test_attention_plan_keeps_sentences_whole_and_aligned():
    lens = G["b_lens"]
    plan = ops.ragged_attention_plan(lens)
    assert plan.dtype == np.int32 and plan.size % 64 == 0
    used = plan[plan >= 0]
    assert used.size == lens.sum()
    for s, n in enumerate(lens.tolist()):
        at = np.nonzero((plan >> 8 == s) & (plan >= 0))[0]
        assert at.size == n and np.array_equal(plan[at] & 255, np.arange(n)) and np.array_equal(at, at[0] + np.arange(n))
        assert at[0] % 16 == 0
        if n <= 64:
            assert at[0] // 64 == at[-1] // 64                                     # inside one bin
        else:
            assert at[0] % 64 == 0                                                 # two bins of its own
            b = at[0] // 64
            assert set(np.unique(plan[b * 64:(b + 2) * 64] >> 8).tolist()) <= {s, -1}
    for bad in ([], [0, 3], [129]):
        with pytest.raises(ValueError):
            ops.ragged_attention_plan(bad)


def test_host_checks_raise_before_any_device_work():
    with pytest.raises(ValueError):
        Z.ragged_layout(np.zeros((0, 77), np.int64))
    with pytest.raises(ValueError):
        Z._group_offsets([3, 0, 4], 7)
    with pytest.raises(ValueError):
        Z._group_offsets([3, 3], 7)
    assert Z._group_offsets([1, 4, 7], 12).tolist() == [0, 1, 5, 12]


@pytest.mark.parametrize("which", ["a", "b"])
def test_oracle_text_tower_reproduces_the_fixture(which):
    from oracle import oracle as O
    sd = W.ulip_pointbert_state_dict(seed=0, with_token_embedding=True)
    ids = torch.from_numpy(G[which + "_ids"]).long()
    with torch.no_grad():
        feat = O.text_tower(sd, sd["token_embedding.weight"][ids], ids.argmax(-1))
    ref = torch.from_numpy(G[which + "_feat"])
    rel = ((feat - ref).norm() / ref.norm()).item()
    print(f"PARITY zeroshot oracle text tower ({which}): rel {rel:.3g} (bound 2e-4)")
    assert rel < 2e-4
    # ... and ULIP's rule on the stored features gives the stored classifier
    groups = [7] * 5 if which == "a" else G["b_groups"].tolist()
    f = ref.double() / ref.double().norm(dim=-1, keepdim=True)
    w = torch.stack([f[a:b].mean(0) for a, b in zip(np.cumsum([0] + groups)[:-1], np.cumsum(groups))])
    w = w / w.norm(dim=-1, keepdim=True)
    assert (w.float() - torch.from_numpy(G[which + "_W"])).abs().max().item() < 1e-6


def test_tokenizer_returns_the_stored_ids():
    from ppt_amd import tokenizer as T
    if T.find_vocab() is None:
        pytest.skip("no CLIP merge table reachable (ppt_amd.tokenizer.find_vocab)")
    ids = T.SimpleTokenizer()([str(s) for s in G["a_sentences"]])
    assert np.array_equal(ids.numpy(), G["a_ids"].astype(np.int64))


def test_cli_without_checkpoints_fails_loudly(tmp_path, monkeypatch):
    """python -m ppt_amd.zeroshot scores the PRETRAINED model: with no checkpoint files under ./data and no opt-in to synthetic
    weights it raises as the reference's torch.load does -- on the host, before a device is touched -- instead of printing the
    figures of a randomly initialised model."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("PPT_SYNTHETIC_WEIGHTS", raising=False)
    ids = np.concatenate([G["a_ids"], G["b_ids"][:5]])
    np.savez(tmp_path / "ids.npz", token_ids=ids, group_sizes=np.ones(40, np.int64))
    for extra in ([], ["--ulip2"]):
        with pytest.raises(FileNotFoundError):
            Z.main(["--test", str(tmp_path / "absent.npz"), "--token_ids", str(tmp_path / "ids.npz")] + extra)
