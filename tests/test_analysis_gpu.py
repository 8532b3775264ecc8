"""GPU: csrc/nearest.hip against direct-form fp64 distances with a stable argsort, and the checkpoint readers of
ppt_amd/analysis.py on top of it.

Tolerance (derived, not measured): gamma = (D + 2) * 2^-24 bounds the relative error of an fp32 sum of D non-negative terms
(q_j - t_j)^2 in any order followed by the square root, so every returned distance lies within gamma * d64 of the fp64 distance of
the row it names, and two rows can only change places when their fp64 distances are closer than 2 gamma d64 (the "band")."""
import contextlib
import functools
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ppt_amd import weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_VOCAB = os.path.join(ROOT, "tests", "golden", "bpe_merges_subset.txt.gz")

# (Q, V, D, k, ld, seed): one query, k close to V, the smallest D, a table below one slice | V one past a power of two, padded
# rows | the real D | the real Q, several slices, a ragged last one | the LDS limit Q D = 32768 (two passes over the query groups)
# | 67 lists of 64 keys per query: more than the 4096 keys the merge pass holds in registers
CASES = [(1, 70, 4, 64, 4, 3), (3, 257, 96, 32, 128, 2), (5, 1000, 512, 10, 512, 0), (32, 4099, 512, 10, 512, 1),
         (64, 2000, 512, 5, 512, 4), (2, 8500, 8, 64, 8, 5)]
IDS = ["Q%d-V%d-D%d-k%d" % c[:4] for c in CASES]


def make_inputs(Q, V, D, seed):
    """rows N(0, 0.02^2) scaled per row by U[0.2, 2] (V table rows, then Q query rows, drawn as one block); row 300 a copy of
    row 5; query 0 a copy of the last table row, query 1 row 7 plus N(0, 0.002^2)"""
    rs = np.random.RandomState(seed)
    rows = (rs.randn(V + Q, D) * 0.02 * rs.uniform(0.2, 2.0, (V + Q, 1))).astype(np.float32)
    table, q = rows[:V].copy(), rows[V:].copy()
    if V > 300:
        table[300] = table[5]
    q[0] = table[V - 1]
    if Q > 1:
        q[1] = table[7] + (rs.randn(D) * 0.002).astype(np.float32)
    return q, table


@functools.lru_cache(maxsize=None)
def reference(case):
    """inputs, fp64 direct-form distances [Q, V] and their stable ascending order [Q, V]; computed once per case"""
    Q, V, D, k, ld, seed = case
    q, table = make_inputs(Q, V, D, seed)
    d64 = np.empty((Q, V), np.float64)
    t64 = table.astype(np.float64)
    for i in range(Q):
        diff = t64 - q[i].astype(np.float64)
        d64[i] = np.sqrt((diff * diff).sum(1))
    order = np.argsort(d64, axis=1, kind="stable")
    for a in (q, table, d64, order):
        a.setflags(write=False)
    return q, table, d64, order


@functools.lru_cache(maxsize=None)
def launched(case):
    """the kernel's answer for the case, once"""
    from ppt_amd import ops
    Q, V, D, k, ld, seed = case
    q, table, _, _ = reference(case)
    bank = torch.zeros((V, ld), dtype=torch.float32)
    bank[:, :D] = torch.tensor(table)
    if ld > D:
        bank[:, D:] = float("nan")                       # the padding is never read
    bank = bank.cuda()[:, :D]
    qd = torch.tensor(q).cuda()
    idx, dist = ops.nearest_rows(qd, bank, k)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and idx.shape == dist.shape == (Q, k)
    return idx.cpu().numpy(), dist.cpu().numpy(), (qd, bank)


def band_mask(case):
    """[Q, k] bool: positions whose fp64 distance is within 2 gamma d64 of a neighbour's in the reference order"""
    Q, V, D, k, ld, seed = case
    _, _, d64, order = reference(case)
    gamma = (D + 2) * 2.0 ** -24
    n = min(V, k + 1)
    r = np.take_along_axis(d64, order[:, :n], 1)
    inside = np.zeros((Q, k), bool)
    for j in range(k):
        tol = 2 * gamma * r[:, j]
        if j > 0:
            inside[:, j] |= (r[:, j] - r[:, j - 1]) <= tol
        if j + 1 < n:
            inside[:, j] |= (r[:, j + 1] - r[:, j]) <= tol
    return inside


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_nearest_rows_against_fp64(case):
    Q, V, D, k, ld, seed = case
    q, table, d64, order = reference(case)
    gamma = (D + 2) * 2.0 ** -24
    inside = band_mask(case)
    print(f"{inside.sum()} of {inside.size} positions inside the band")
    assert inside.sum() <= 0.15 * inside.size, "the reference itself leaves too few positions for the exact-order check"

    idx, dist, _ = launched(case)
    assert (idx >= 0).all() and (idx < V).all()
    d_named = np.take_along_axis(d64, idx.astype(np.int64), 1)                     # fp64 distance of the rows the kernel names
    err = np.abs(dist.astype(np.float64) - d_named)
    print("max |dist - d64| / (gamma d64):", float((err / np.maximum(gamma * d_named, 1e-300)).max()))
    assert (err <= gamma * d_named).all()
    assert dist[0, 0] == 0.0 and idx[0, 0] == V - 1
    assert (np.diff(dist.astype(np.float64), axis=1) >= 0).all()
    for i in range(Q):
        assert len(set(idx[i].tolist())) == k, f"query {i}: repeated rows"
    want = order[:, :k]
    r = np.take_along_axis(d64, want, 1)
    exact = ~inside
    assert (idx[exact] == want[exact]).all(), np.argwhere(exact & (idx != want))[:5]
    assert (np.abs(d_named - r)[inside] <= (2 * gamma * r)[inside]).all()
    for i in range(Q):                                                             # the copied pair: equal distances, lower row first
        row = idx[i].tolist()
        if 5 in row and 300 in row:
            assert row.index(5) < row.index(300), f"query {i}: row 300 precedes its copy, row 5"


def test_copied_rows_tie_goes_to_the_lower_row():
    """a query next to the copied pair sees both at the same distance, row 5 first (the generic cases only meet the pair by chance)"""
    from ppt_amd import ops
    case = CASES[3]
    q, table, _, _ = reference(case)
    qq = np.array(q[:2], copy=True)
    qq[1] = table[5] * np.float32(1.001)
    idx, dist = ops.nearest_rows(torch.from_numpy(qq).cuda(), launched(case)[2][1], 4)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert idx[1, :2].tolist() == [5, 300] and dist[1, 0] == dist[1, 1]


def test_nearest_rows_is_deterministic():
    from ppt_amd import ops
    case = CASES[3]
    idx, dist, (qd, bank) = launched(case)
    for _ in range(2):
        i2, d2 = ops.nearest_rows(qd, bank, case[3])
        assert np.array_equal(i2.cpu().numpy(), idx)
        assert np.array_equal(d2.cpu().numpy().view(np.int32), dist.view(np.int32))


def test_nearest_rows_orders_non_finite_rows_last_and_rejects_bad_shapes():
    from ppt_amd import ops
    q, table = make_inputs(2, 300, 8, 9)
    table = np.array(table, copy=True)
    table[3, 2] = np.nan
    table[299, 0] = np.inf
    table[17] = q[1]
    idx, dist = ops.nearest_rows(torch.from_numpy(q).cuda(), torch.from_numpy(table).cuda(), 64)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert np.isfinite(dist).all() and not ({3, 299} & set(idx.reshape(-1).tolist()))
    assert idx[1, 0] == 17 and dist[1, 0] == 0.0
    # k = V = 5: every row is returned, the finite ones first, then the infinite one, then the NaN
    sub = table[:5, :4].copy()
    sub[1, 0] = np.inf
    idx, dist = ops.nearest_rows(torch.from_numpy(q[:1, :4].copy()).cuda(), torch.from_numpy(sub).cuda(), 5)
    idx, d = idx.cpu().numpy()[0], dist.cpu().numpy()[0]
    assert sorted(idx[:3].tolist()) == [0, 2, 4] and np.isfinite(d[:3]).all()
    assert idx[3:].tolist() == [1, 3] and np.isinf(d[3]) and np.isnan(d[4])
    with pytest.raises(RuntimeError, match="unsupported|-3"):
        ops.nearest_rows(torch.zeros(2, 6).cuda(), torch.zeros(10, 6).cuda(), 2)
    with pytest.raises(RuntimeError, match="unsupported|-3"):
        ops.nearest_rows(torch.zeros(2, 8).cuda(), torch.zeros(10, 8).cuda(), 11)


# ---- the readers ---------------------------------------------------------------------------------------------------------------
def _table_and_ctx():
    from ppt_amd import tokenizer as T
    tok = T.SimpleTokenizer(GOLDEN_VOCAB)
    # two ids below 4099 whose words survive in the cut-down merge table: a byte symbol with its end-of-word mark and a merge
    word_ids = [tok.encoder["a" + T.END]] + [i for i in range(512, 4099) if not tok.decoder[i].startswith("␀")][:1]
    assert len(word_ids) == 2
    _, table, _, _ = reference(CASES[3])
    ctx = (np.random.RandomState(8).randn(4, 512) * 0.02).astype(np.float32)
    ctx[0], ctx[1] = table[word_ids[0]], table[word_ids[1]]
    model = SimpleNamespace(token_embedding=SimpleNamespace(weight=torch.tensor(table).cuda()))
    return tok, word_ids, model, torch.from_numpy(ctx)


def test_nearest_tokens_and_interpret_prompt(monkeypatch, tmp_path, capsys):
    from ppt_amd import analysis
    tok, word_ids, model, ctx = _table_and_ctx()
    ids, dist = analysis.nearest_tokens(ctx.double(), model.token_embedding.weight, 3)
    assert ids.is_cuda and ids.dtype == torch.int64 and dist.dtype == torch.float32 and ids.shape == dist.shape == (4, 3)
    assert ids[:2, 0].tolist() == word_ids and dist[:2, 0].tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        analysis.nearest_tokens(ctx.view(2, 2, 512), model.token_embedding.weight, 3)

    capsys.readouterr()
    rows = analysis.interpret_prompt({"state_dict": {"learnable_tokens": ctx}}, model, 3, bpe_path=GOLDEN_VOCAB)
    lines = capsys.readouterr().out.splitlines()
    assert len(rows) == 4 and rows[0][1] == ids[0].tolist() and rows[0][2] == dist[0].tolist()
    word = tok.decoder[word_ids[0]]
    assert rows[0][0][0] == word
    line = next(l for l in lines if l.startswith("1: "))
    assert line.startswith(f"1: ['{word}', ") and "] ['0.0000', " in line
    assert line == f"1: {rows[0][0]} {[f'{d:.4f}' for d in rows[0][2]]}"
    assert next(l for l in lines if l.startswith("2: ")).startswith(f"2: ['{tok.decoder[word_ids[1]]}', ")

    # no merge table anywhere: ids instead of words, and one line that says so
    monkeypatch.delenv("PPT_BPE_VOCAB", raising=False)
    monkeypatch.chdir(tmp_path)
    from ppt_amd import tokenizer as T
    if T.find_vocab() is None:
        rows = analysis.interpret_prompt({"learnable_tokens": ctx}, model, 3)
        out = capsys.readouterr().out
        assert all(r[0] is None for r in rows) and rows[1][1][0] == word_ids[1]
        assert "merge table was not found" in out and f"1: [{word_ids[0]}, " in out


def test_recognition_logits_equal_the_model_batch_by_batch():
    """ULIP_PointBERT, head_type 2, synthetic weights, 3 classes, batches of 3 and 2 clouds of 1024 points with injected FPS starts"""
    from ppt_amd import analysis
    from ppt_amd.models import ULIP_models as M
    names = M.dataset_classnames("modelnet40")[:3]
    args = SimpleNamespace(classnames=names, template_init='', class_name_position='middle', num_learnable_prompt_tokens=32, gpu=0,
                           task='cls', head_type=2, evaluate_3d=False, ulip2=False, synthetic_weights=True)
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.ULIP_PointBERT(args)
    m.load_state_dict(W.ulip_pointbert_state_dict(seed=0), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding(3, seed=0)
    m.cuda()
    m.train()
    mode = m.precision_name
    pc_np, start = W.synth_clouds(5, 1024, seed=13)
    pc, start = torch.from_numpy(pc_np), torch.from_numpy(start)
    labels = torch.tensor([2, 0, 1, 1, 0], dtype=torch.int32)
    cuts = [(0, 3), (3, 5)]

    def batches():
        for lo, hi in cuts:
            m.point_encoder.fps_start = start[lo:hi].cuda()
            yield pc[lo:hi], labels[lo:hi], "ignored"

    logits, labs = analysis.recognition_logits(m, batches())
    assert m.training and m.precision_name == mode
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.shape == (5, 3)
    assert labs.is_cuda and labs.dtype == torch.int64 and labs.tolist() == labels.tolist()
    m.eval()
    with torch.no_grad():
        for lo, hi in cuts:
            m.point_encoder.fps_start = start[lo:hi].cuda()
            assert torch.equal(logits[lo:hi], m(pc[lo:hi].cuda()).float()), (lo, hi)
    assert torch.isfinite(logits).all()
