"""GPU: ragged clouds on packed rows -- the per-point tail of the part-segmentation decoder (ppt_knn_group_packed_f32,
ppt_three_nn_interp_packed_fwd, ppt_scatter_rows_packed_bwd, ppt_pack_rows / ppt_unpack_rows, ppt_partseg_metrics_ragged,
ppt_train_meter_partseg_ragged), PartsegMetrics.update(lengths=), ULIP_PointBERT_partseg.forward_ragged(pc, onehot, lengths)
against the CPU oracle per cloud and against tests/partseg_ragged_ref.py, validate_partseg over whole shapes and the loader's
whole-shape mode.

The yardstick of every kernel test is the UNIFORM entry point run on each cloud alone at N = lengths[b] (and the C oracle for the
neighbour search): every comparison is torch.equal / np.array_equal.  B = 3, Nmax = 704, lengths [700, 513, 300]: R = 1513 is no
multiple of any tile, the cloud boundaries fall inside a wave, one cloud is a row over the 512 anchors and one under them, and
3 * lengths[b] is no multiple of the scatter's staging chunk.  Padding rows hold NaN: one read behind a cloud's end shows."""
import numpy as np
import pytest
import torch

import validate_ref as V
from oracle import oracle as O
from ppt_amd import weights as W

pytestmark = pytest.mark.gpu

NMAX, LENGTHS, S = 704, [700, 513, 300], 512


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def case():
    """pc [B, Nmax, 3] with NaN padding, anchors [B, 512, 3] (rows of the cloud, repeated where it is shorter), lengths, offsets"""
    L = np.asarray(LENGTHS, dtype=np.int32)
    pc, _ = W.synth_clouds(len(L), NMAX, seed=71)
    anchors = np.stack([pc[b, (np.arange(S) * 5) % n] for b, n in enumerate(L)])
    for b, n in enumerate(L):
        pc[b, n:] = np.nan
    off = np.concatenate([[0], np.cumsum(L)]).astype(np.int32)
    return pc, anchors, L, off


def _packed_knn(ops, case, k):
    pc, anchors, L, off = case
    return ops.knn_group(dev(anchors), dev(pc), k, want_nbhd=False, want_dist=True, query_lengths=dev(L), query_offsets=dev(off),
                         total_rows=int(off[-1]))


# ------------------------------------------------------------------ neighbour search
@pytest.mark.parametrize("k", [3, 4])
def test_knn_packed_equals_the_uniform_kernel_and_the_oracle_per_cloud(case, k):
    from ppt_amd import ops
    pc, anchors, L, off = case
    idx, _, dist = _packed_knn(ops, case, k)
    assert tuple(idx.shape) == (off[-1], k) and tuple(dist.shape) == (off[-1], k)
    for b, n in enumerate(L):
        ui, _, ud = ops.knn_group(dev(anchors[b:b + 1]), dev(pc[b:b + 1, :n]), k, want_nbhd=False, want_dist=True)
        assert torch.equal(idx[off[b]:off[b + 1]], ui[0]) and torch.equal(dist[off[b]:off[b + 1]], ud[0]), (b, n)
        want = O.three_nn(pc[b:b + 1, :n], anchors[b:b + 1])[0] if k == 3 else O.knn(anchors[b:b + 1], pc[b:b + 1, :n], k)[0]
        assert np.array_equal(host(idx[off[b]:off[b + 1]]), want[0]), (b, n)


def test_knn_packed_writes_the_neighbourhoods_and_leaves_the_rest_alone(case):
    """neighbourhood output in packed rows; ragged SOURCES together with ragged queries; an output buffer longer than R keeps
    its bytes behind row R"""
    from ppt_amd import _lib, ops
    pc, anchors, L, off = case
    R, k = int(off[-1]), 4
    src_len = np.asarray([512, 300, 37], dtype=np.int32)
    src = anchors.copy()
    for b, n in enumerate(src_len):
        src[b, n:] = np.nan
    idx, nb = ops.knn_group(dev(src), dev(pc), k, lengths=dev(src_len), query_lengths=dev(L), total_rows=R)
    for b, n in enumerate(L):
        ui, un = ops.knn_group(dev(src[b:b + 1, :src_len[b]]), dev(pc[b:b + 1, :n]), k)
        assert torch.equal(idx[off[b]:off[b + 1]], ui[0]) and torch.equal(nb[off[b]:off[b + 1]], un[0]), (b, n)
    big = torch.full((R + 64, k), -7, dtype=torch.int64, device="cuda")
    p = ops._p
    a_d, pc_d, L_d, off_d = dev(anchors), dev(pc), dev(L), dev(off)
    _lib.check(_lib.lib().ppt_knn_group_packed_f32(p(a_d), p(pc_d), 3, S, NMAX, k, None, p(L_d), p(off_d), R, p(big),
                                                   None, None, ops._stream()), "ppt_knn_group_packed_f32")
    torch.cuda.synchronize()
    assert bool((big[R:] == -7).all()) and bool((big[:R] >= 0).all())


# ------------------------------------------------------------------ interpolation
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_interp_packed_equals_the_uniform_kernel_per_cloud(case, dtype):
    """propagation_0's operand: [one-hot(16) | xyz(3) | interpolated(D2) | 0] -- the class row and the padded cloud go in as they
    are; the uniform kernel gets the concatenated points1 of each cloud alone"""
    from ppt_amd import ops
    pc, anchors, L, off = case
    B, D2, mult = len(L), 40, 8 if dtype != torch.float32 else 4
    rng = np.random.default_rng(5)
    p2 = dev(rng.standard_normal((B, S, D2)).astype(np.float32))
    cls = torch.zeros(B, 16, device="cuda")
    cls[torch.arange(B), torch.tensor([3, 0, 15])] = 1
    idx, _, dist = _packed_knn(ops, case, 3)
    rows, w = ops.three_nn_interp_packed(cls, dev(pc), p2, idx, dist, dev(off), dtype, mult)
    ld = (19 + D2 + mult - 1) // mult * mult
    assert tuple(rows.shape) == (off[-1], ld) and rows.dtype == dtype and tuple(w.shape) == (off[-1], 3)
    for b, n in enumerate(L):
        sl = slice(off[b], off[b + 1])
        p1 = torch.cat([cls[b].expand(n, 16), dev(pc[b, :n])], dim=1)[None].contiguous()
        ur, uw = ops.three_nn_interp(p1, p2[b:b + 1].contiguous(), idx[sl][None].contiguous(), dist[sl][None].contiguous(), dtype, mult)
        assert torch.equal(rows[sl].view(torch.int16 if dtype != torch.float32 else torch.int32),
                           ur.view(torch.int16 if dtype != torch.float32 else torch.int32)), (b, n)
        assert torch.equal(w[sl], uw[0]), (b, n)
    assert bool(torch.isfinite(rows.float()).all())
    # either half of points1 may be absent
    r2, _ = ops.three_nn_interp_packed(None, dev(pc), p2, idx, dist, dev(off), dtype, mult)
    assert torch.equal(r2[:, :3 + D2].float(), rows[:, 16:19 + D2].float())


# ------------------------------------------------------------------ interpolation backward
@pytest.mark.parametrize("C,col_off,weighted", [(40, 19, True), (200, 0, False)])
def test_scatter_packed_equals_the_uniform_kernel_per_cloud(case, C, col_off, weighted):
    from ppt_amd import ops
    pc, anchors, L, off = case
    R = int(off[-1])
    idx, _, dist = _packed_knn(ops, case, 3)
    rng = np.random.default_rng(6)
    d_rows = dev(rng.standard_normal((R, col_off + C + 5)).astype(np.float32))
    wgt = dev(rng.random((R, 3)).astype(np.float32)) if weighted else None
    got = ops.scatter_rows_packed_bwd(idx.view(-1), None if wgt is None else wgt.view(-1), d_rows, col_off, 3, dev(off), S, C)
    assert tuple(got.shape) == (len(L), S, C)
    for b, n in enumerate(L):
        sl = slice(off[b], off[b + 1])
        want = ops.scatter_rows_bwd(idx[sl].reshape(1, 3 * n).contiguous(), None if wgt is None else wgt[sl].reshape(1, 3 * n).contiguous(),
                                    d_rows[sl].contiguous(), col_off, 3, S, C)
        assert torch.equal(got[b], want[0]), (b, n)


def test_scatter_packed_with_lists_longer_than_the_staging_chunk():
    """cloud lists of 3 * 3000 and 3 * 2731 entries: both over the 8192-entry staging chunk, neither a multiple of it, and
    different from workgroup to workgroup"""
    from ppt_amd import ops
    L = np.asarray([3000, 40, 2731], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(L)]).astype(np.int32)
    R, S2, C = int(off[-1]), 96, 24
    rng = np.random.default_rng(8)
    idx = dev(rng.integers(0, S2, (R, 3)).astype(np.int64))
    wgt = dev(rng.random((R, 3)).astype(np.float32))
    d_rows = dev(rng.standard_normal((R, C)).astype(np.float32))
    got = ops.scatter_rows_packed_bwd(idx.view(-1), wgt.view(-1), d_rows, 0, 3, dev(off), S2, C)
    for b, n in enumerate(L):
        sl = slice(off[b], off[b + 1])
        want = ops.scatter_rows_bwd(idx[sl].reshape(1, -1).contiguous(), wgt[sl].reshape(1, -1).contiguous(), d_rows[sl].contiguous(),
                                    0, 3, S2, C)
        assert torch.equal(got[b], want[0]), (b, n)


# ------------------------------------------------------------------ pack / unpack
@pytest.mark.parametrize("C,dtype", [(50, torch.float32), (128, torch.float32), (128, torch.float16), (7, torch.uint8)])
def test_pack_unpack_rows(case, C, dtype):
    from ppt_amd import ops
    _, _, L, off = case
    R, B = int(off[-1]), len(L)
    g = torch.Generator().manual_seed(C)
    packed = (torch.randint(1, 200, (R, C), generator=g).to(dtype)).cuda()
    padded = ops.unpack_rows(packed, dev(off), NMAX)
    assert tuple(padded.shape) == (B, NMAX, C) and padded.dtype == dtype
    for b, n in enumerate(L):
        assert torch.equal(padded[b, :n], packed[off[b]:off[b + 1]]) and not bool(padded[b, n:].any()), (b, n)
    # pack reads nothing behind a cloud's end: poison it
    poisoned = padded.clone()
    for b, n in enumerate(L):
        poisoned[b, n:] = 77
    assert torch.equal(ops.pack_rows(poisoned, dev(off), R), packed)
    # a view one element into a buffer: the address allows narrower accesses only
    if dtype == torch.float32:
        shifted = torch.empty(R * C + 1, dtype=dtype, device="cuda")[1:].view(R, C)
        shifted.copy_(packed)
        assert torch.equal(ops.unpack_rows(shifted, dev(off), NMAX), padded)


# ------------------------------------------------------------------ metrics
def _metric_case(Nmax, lengths, seed):
    """logits [B, Nmax, 50] / labels [B, Nmax] of ShapeNetPart categories, NaN logits and label -100 behind every cloud's end"""
    c2p = V.category2part()
    cats = list(c2p.values())
    g = torch.Generator().manual_seed(seed)
    B = len(lengths)
    logits = torch.randn(B, Nmax, 50, generator=g) * 3
    labels = torch.full((B, Nmax), -100, dtype=torch.int64)
    for b, n in enumerate(lengths):
        parts = cats[(5 * b + seed) % len(cats)]
        labels[b, :n] = torch.tensor(parts)[torch.randint(0, len(parts), (n,), generator=g)]
        logits[b, n:] = float("nan")
    return logits, labels, c2p


@pytest.mark.parametrize("Nmax,lengths", [(NMAX, LENGTHS), (NMAX, [1, NMAX, 65])])
def test_partseg_metrics_ragged_equals_the_uniform_records_per_cloud(Nmax, lengths):
    from ppt_amd import evaluate
    logits, labels, c2p = _metric_case(Nmax, lengths, seed=3)
    m = evaluate.PartsegMetrics(c2p, 0.2)
    m.update(logits.cuda(), labels.cuda(), lengths=lengths)
    m_dev = evaluate.PartsegMetrics(c2p, 0.2)
    m_dev.update(logits.cuda(), labels.cuda(), lengths=dev(np.asarray(lengths, dtype=np.int32)), total_rows=sum(lengths))
    got = m.records.host()
    assert np.array_equal(got, m_dev.records.host()) and m.records.batches == m_dev.records.batches      # the same launch
    lone = evaluate.PartsegMetrics(c2p, 0.2)
    for b, n in enumerate(lengths):
        lone.update(logits[b:b + 1, :n].contiguous().cuda(), labels[b:b + 1, :n].contiguous().cuda())
    want = lone.records.host()
    assert np.array_equal(got[:len(lengths)], want), (got[:, :8], want[:, :8])          # every byte, the loss sums included
    # the loss sums against float64 on the host: the bound tests/test_validate_gpu.py holds the uniform kernel to
    for b, n in enumerate(lengths):
        ref = V.partseg_records(logits[b:b + 1, :n], labels[b:b + 1, :n], c2p, 0.2).numpy()      # the plain torch recomputation
        keep = [c for c in range(32) if c != 4]
        assert np.array_equal(got[b, keep], ref[0, keep]), (b, n)
        x, t = logits[b, :n].double(), labels[b, :n]
        lse = torch.logsumexp(x, dim=1)
        loss64 = (0.8 * (lse - x.gather(1, t[:, None])[:, 0]) + 0.2 * (lse - x.mean(dim=1))).sum().item()
        loss32 = float(got[b:b + 1, 4].copy().view(np.float32)[0])
        assert abs(loss32 - loss64) <= 1e-6 * abs(loss64), (b, n, loss32, loss64)
    out, out_lone = m.result(), lone.result()
    assert out["n"] == out_lone["n"] == len(lengths) and out["nonfinite_rows"] == 0
    assert V.same_bits(out["mean_inst_iou"], out_lone["mean_inst_iou"])
    assert V.same_bits(list(out["category_ious"].values()), list(out_lone["category_ious"].values()))
    R = sum(lengths)
    assert out["acc"] == (torch.tensor(int(got[:len(lengths), 2].sum())) / R).item()
    loss_all = got[:len(lengths), 4].copy().view(np.float32).astype(np.float64).sum() / R
    assert abs(out["loss"] - loss_all) <= 1e-12 * loss_all


@pytest.mark.parametrize("Nmax,lengths", [(NMAX, LENGTHS), (NMAX, [1, NMAX, 65])])
def test_train_meter_partseg_ragged(Nmax, lengths):
    """the record after one metered step: acc = correct / sum(lengths) with the correct count of the clouds alone; the scratch
    ends all zero, and a second step folds on top"""
    from ppt_amd import evaluate, ops
    logits, labels, c2p = _metric_case(Nmax, lengths, seed=4)
    start, count = (dev(t) for t in evaluate.part_tables(c2p))
    loss = torch.tensor(1.25, device="cuda")
    L = dev(np.asarray(lengths, dtype=np.int32))
    rec = torch.zeros(ops.METER_REC, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(ops.METER_SCRATCH, dtype=torch.int32, device="cuda")
    ops.train_meter_partseg(logits.cuda(), labels.cuda(), loss, start, count, rec, scratch, weight=float(len(lengths)), lengths=L)
    assert not bool(scratch.any())
    correct = 0
    for b, n in enumerate(lengths):
        r1 = torch.zeros(ops.METER_REC, dtype=torch.float64, device="cuda")
        ops.train_meter_partseg(logits[b:b + 1, :n].contiguous().cuda(), labels[b:b + 1, :n].contiguous().cuda(), loss, start, count, r1, scratch)
        correct += round(r1[6].item() * n)
    acc = float(np.float32(correct) / np.float32(sum(lengths)))
    want = [1.25 * len(lengths), acc * len(lengths), float(len(lengths)), 1.0, 0.0, 1.25, acc, 0.0]
    assert rec.tolist() == want, (rec.tolist(), want)
    ops.train_meter_partseg(logits.cuda(), labels.cuda(), loss, start, count, rec, scratch, weight=float(len(lengths)), lengths=L)
    assert rec[3].item() == 2.0 and rec[6].item() == acc and not bool(scratch.any())


# =================================================================== the model: ULIP_PointBERT_partseg.forward_ragged(pc, onehot, lengths)
import contextlib                                                      # noqa: E402
import io                                                              # noqa: E402
import json                                                            # noqa: E402
import os                                                              # noqa: E402
from types import SimpleNamespace                                      # noqa: E402

import partseg_ragged_ref as R                                         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_LENGTHS = [700, 513, 640]


def _model(precision):
    from ppt_amd.models import ULIP_models as M
    args = SimpleNamespace(classnames=M.dataset_classnames("shapenetpart"), template_init='', class_name_position='middle',
                           num_learnable_prompt_tokens=32, gpu=0, task='partseg', head_type=0, evaluate_3d=False, ulip2=False,
                           synthetic_weights=True)
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.ULIP_PointBERT_partseg(args)
    m.load_state_dict(W.ulip_partseg_state_dict(seed=0), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding(50, seed=0)
    m.cuda().set_precision(precision)
    m.overlap_text_tower = False
    return m


def _batch(Nmax, lengths, seed, fill=np.nan):
    """pc [B,Nmax,3] (padding = fill), onehot [B,16], labels [B,Nmax] (-100 padding), starts 3 x [B], DropPath factors [12,2,B],
    dropout mask [B,Nmax,128] -- all numpy / CPU; the valid rows do not depend on Nmax or fill"""
    B = len(lengths)
    rng = np.random.default_rng(seed)
    base, _ = W.synth_clouds(B, max(lengths), seed=seed)
    pc = np.full((B, Nmax, 3), fill, dtype=np.float32)
    labels = np.full((B, Nmax), -100, dtype=np.int64)
    drop = np.zeros((B, Nmax, 128), dtype=np.float32)
    for b, n in enumerate(lengths):
        pc[b, :n] = base[b, :n]
        labels[b, :n] = rng.integers(0, 50, n)
        drop[b, :n] = (rng.random((n, 128)) > 0.5).astype(np.float32) * 2.0
    onehot = np.zeros((B, 16), dtype=np.float32)
    onehot[np.arange(B), rng.integers(0, 16, B)] = 1
    starts = tuple(rng.integers(0, np.asarray(lengths)).astype(np.int64) for _ in range(3))
    dp = (np.floor(0.9 + rng.random((12, 2, B))) / 0.9).astype(np.float32)
    return pc, onehot, labels, starts, dp, drop


def _inject(m, starts, dp, drop):
    pe = m.point_encoder
    pe.fps_start = tuple(dev(s) for s in starts)
    pe.drop_path_factors = None if dp is None else dev(dp)
    pe.dropout_mask = None if drop is None else dev(drop)


def _step(m, pc, onehot, labels, lengths):
    """forward (+ CE with the default ignore_index and backward in train mode) -> (logits, {name: grad})"""
    m.zero_grad(set_to_none=True)
    if not m.training:
        with torch.no_grad():
            return (m(dev(pc), dev(onehot)) if lengths is None else m.forward_ragged(dev(pc), dev(onehot), lengths)), {}
    logits = m(dev(pc), dev(onehot)) if lengths is None else m.forward_ragged(dev(pc), dev(onehot), lengths)
    loss = torch.nn.CrossEntropyLoss(label_smoothing=0.2)(logits.reshape(-1, 50), dev(labels).reshape(-1))
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}, loss.detach()


@pytest.mark.parametrize("train", [False, True])
def test_nothing_behind_a_clouds_end_matters(train):
    """NaN padding, zero padding and the clouds re-laid at Nmax = 1024: the same bits on every valid row and in every gradient;
    the returned padding rows are exactly zero"""
    m = _model(torch.float32)
    m.train(train)
    outs = []
    for Nmax, fill in ((NMAX, np.nan), (NMAX, 0.0), (1024, np.nan)):
        pc, onehot, labels, starts, dp, drop = _batch(Nmax, LENGTHS, seed=83, fill=fill)
        _inject(m, starts, dp if train else None, drop if train else None)
        outs.append(_step(m, pc, onehot, labels, LENGTHS))
    for o in outs:
        assert tuple(o[0].shape)[::2] == (3, 50) and bool(torch.isfinite(o[0]).all())
        for b, n in enumerate(LENGTHS):
            assert torch.equal(o[0][b, :n], outs[0][0][b, :n]), (b, n)
            assert not bool(o[0][b, n:].any()), (b, n)
    if train:
        assert len(outs[0][1]) > 10
        for o in outs[1:]:
            assert sorted(o[1]) == sorted(outs[0][1]) and torch.equal(o[2], outs[0][2])
            for k, g in o[1].items():
                assert torch.equal(g, outs[0][1][k]), k


@pytest.mark.parametrize("train", [False, True])
def test_uniform_lengths_equal_the_uniform_call(train):
    """lengths = [N] * B with injected starts, DropPath and dropout mask against the call without lengths (eager): logits and every
    gradient bit for bit, B = 2, N = 640"""
    m = _model(torch.float32)
    m.point_encoder.use_hip_graphs = False
    m.use_hip_graphs = False
    m.train(train)
    pc, onehot, labels, starts, dp, drop = _batch(640, [640, 640], seed=85)
    _inject(m, starts, dp if train else None, drop if train else None)
    a = _step(m, pc, onehot, labels, [640, 640])
    b = _step(m, pc, onehot, labels, None)
    assert torch.equal(a[0], b[0])
    if train:
        assert len(a[1]) > 10 and sorted(a[1]) == sorted(b[1]) and torch.equal(a[2], b[2])
        for k, g in a[1].items():
            assert torch.equal(g, b[1][k]), k


def _text_side():
    tok = json.load(open(os.path.join(ROOT, "ppt_amd", "data", "classnames.json")))
    nl = [len(tok["name_tokens"][n.replace("_", " ")]) for n in tok["datasets"]["shapenetpart"]]
    eot = np.load(os.path.join(ROOT, "tests", "golden", "g_partseg.npz"), allow_pickle=False)["eot"].astype(np.int64)
    return W.synth_prompt_embedding(50, seed=0), nl, eot


@pytest.fixture(scope="module")
def oracle_eval():
    """the CPU oracle on each cloud alone (B = 1, N = lengths[b]), eval mode: computed once for the three modes"""
    pc, onehot, _, starts, _, _ = _batch(NMAX, ORACLE_LENGTHS, seed=87)
    sd = W.ulip_partseg_state_dict(seed=0)
    emb, nl, eot = _text_side()
    with torch.no_grad():
        ref = [O.partseg_logits(sd, torch.from_numpy(pc[b:b + 1, :n]), torch.from_numpy(onehot[b:b + 1]), tuple(s[b:b + 1] for s in starts),
                                emb, nl, eot).numpy()[0] for b, n in enumerate(ORACLE_LENGTHS)]
    return pc, onehot, starts, ref


@pytest.mark.parametrize("precision", [torch.float32, "split16", torch.bfloat16])
def test_ragged_eval_logits_match_the_oracle_per_cloud(oracle_eval, precision):
    """bounds of tests/test_model_gpu.py::test_partseg_train_step_matches_golden for logits: 2e-2 fp32-grade, 0.3 mixed.  The
    unchanged uniform path on each cloud alone is printed beside it: the figure the ragged error is to be judged against."""
    pc, onehot, starts, ref = oracle_eval
    m = _model(precision)
    m.eval()
    _inject(m, starts, None, None)
    with torch.no_grad():
        got = host(m.forward_ragged(dev(pc), dev(onehot), ORACLE_LENGTHS))
    bound = 0.3 if precision == torch.bfloat16 else 2e-2
    errs = []
    for b, n in enumerate(ORACLE_LENGTHS):
        _inject(m, tuple(s[b:b + 1] for s in starts), None, None)
        with torch.no_grad():
            lone = host(m(dev(pc[b:b + 1, :n]), dev(onehot[b:b + 1])))[0]
        errs.append((np.abs(got[b, :n] - ref[b]).max(), np.abs(lone - ref[b]).max()))
        assert not got[b, n:].any()
    print(f"PARITY ragged partseg {precision} logits abs err per cloud (ragged batch, uniform path alone):", errs, f"(bound {bound})")
    assert max(e[0] for e in errs) < bound


def test_ragged_training_statistics_match_the_float64_reference():
    """train mode, fp32, injected RNG: logits, loss (labels padded with -100), the gradients of conv1 / bn1 / the prompt tokens (2e-3
    relative L2) and of propagation_0 (6e-2), and bn1's running statistics after the step (1e-5: padding rows in the statistics
    would move them by the padded share) against tests/partseg_ragged_ref.py"""
    L = ORACLE_LENGTHS
    pc, onehot, labels, starts, dp, drop = _batch(NMAX, L, seed=89)
    m = _model(torch.float32)
    m.train()
    _inject(m, starts, dp, drop)
    logits, grads, loss = _step(m, pc, onehot, labels, L)
    sd = W.ulip_partseg_state_dict(seed=0)
    keys = [k for k in grads if k.startswith(("point_encoder.conv1.", "point_encoder.bn1.", "point_encoder.propagation_0.", "prompt_learner."))]
    assert len(keys) >= 12
    sd2 = dict(sd)
    for k in keys:
        sd2[k] = sd[k].detach().clone().requires_grad_(True)
    emb, nl, eot = _text_side()
    ns = {}
    masks = [(torch.from_numpy(a[0]), torch.from_numpy(a[1])) for a in dp]
    ref = R.partseg_logits_ragged(sd2, pc, L, torch.from_numpy(onehot), starts, emb, nl, eot, train=True, dp_masks=masks,
                                  drop_mask=torch.from_numpy(drop), new_stats=ns)
    tgt = torch.cat([torch.from_numpy(labels[b, :n]) for b, n in enumerate(L)])
    ref_loss = torch.nn.functional.cross_entropy(ref, tgt, label_smoothing=0.2)
    ref_grads = dict(zip(keys, torch.autograd.grad(ref_loss, [sd2[k] for k in keys])))
    got = torch.cat([logits[b, :n] for b, n in enumerate(L)]).cpu().double()
    e_logits, e_loss = (got - ref.detach()).abs().max().item(), abs(loss.item() - ref_loss.item())
    print(f"PARITY ragged partseg train: logits abs err {e_logits:.4g} (bound 2e-2), loss abs err {e_loss:.4g} (bound 1e-3)")
    assert e_logits < 2e-2 and e_loss < 1e-3
    for k in keys:
        r = ref_grads[k].double().flatten()
        if r.norm().item() < 1e-4:                # biases in front of a BatchNorm: mathematically zero gradient
            continue
        rel = ((grads[k].cpu().double().flatten() - r).norm() / r.norm()).item()
        bound = 6e-2 if "propagation_0" in k else 2e-3
        print(f"PARITY ragged partseg train grad {k}: rel-L2 {rel:.4g} (bound {bound})")
        assert rel < bound, (k, rel)
    live = m.state_dict()
    for k in ("point_encoder.bn1.running_mean", "point_encoder.bn1.running_var"):
        d = (live[k].cpu().double() - ns[k].double()).abs().max().item()
        print(f"PARITY ragged partseg train {k}: max abs diff {d:.4g}")
        assert torch.allclose(live[k].cpu().double(), ns[k].double(), rtol=1e-5, atol=1e-5), k


# =================================================================== validation and the loader
def _shape_set(seed=91):
    from ppt_amd.data import DeviceCloudSet
    rng = np.random.default_rng(seed)
    c2p = V.category2part()
    cats = list(c2p)
    lens = [704, 300, 513, 640, 455, 700]
    cls = np.array([0, 3, 3, 8, 15, 0])
    clouds = [W.synth_clouds(1, n, seed=seed + i)[0][0] for i, n in enumerate(lens)]
    seg = [np.asarray(c2p[cats[c]])[rng.integers(0, len(c2p[cats[c]]), n)].astype(np.int32) for c, n in zip(cls, lens)]
    return DeviceCloudSet(clouds, cls, seg=seg), lens, c2p


class _Starts:
    """a model wrapper that injects each batch's FPS starts: sample i always walks from start[i], in a batch or alone"""

    def __init__(self, m, starts):
        self.m, self.starts, self.at = m, starts, 0

    def eval(self):
        self.m.eval()

    def _inject(self, B):
        self.m.point_encoder.fps_start = tuple(dev(s[self.at:self.at + B]) for s in self.starts)
        self.at += B

    def __call__(self, pc, onehot):
        self._inject(pc.shape[0])
        return self.m(pc, onehot)

    def forward_ragged(self, pc, onehot, lengths, total_rows=None):
        self._inject(pc.shape[0])
        return self.m.forward_ragged(pc, onehot, lengths, total_rows=total_rows)


def test_validate_partseg_over_whole_shapes_equals_the_shapes_alone():
    from ppt_amd import evaluate
    from ppt_amd.data import DeviceBatchLoader
    cset, lens, c2p = _shape_set()
    loader = DeviceBatchLoader(cset, 4, 2048, "shapenetpart", False, shuffle=False, ragged=True)
    assert loader.ragged and loader.plan() == ("cloud_prep",) and len(loader) == 2
    batches = [tuple(t.clone() for t in b) for b in loader]
    assert [tuple(b[0].shape) for b in batches] == [(4, 704, 3), (2, 704, 3)]
    o = 0
    for pc, cls, seg, L in batches:
        assert L.dtype == torch.int32 and L.tolist() == lens[o:o + len(L)] and seg.dtype == torch.int64 and cls.dtype == torch.int32
        pad = torch.arange(704, device="cuda")[None] >= L[:, None]
        assert bool((seg[pad] == -100).all()) and bool((seg[~pad] >= 0).all()) and bool(torch.isfinite(pc).all())
        for b, n in enumerate(L.tolist()):
            assert torch.equal(pc[b, :n], cset.points[o + b, :n]) and torch.equal(seg[b, :n], cset.seg[o + b, :n].long())
        o += len(L)
    rng = np.random.default_rng(7)
    starts = tuple(rng.integers(0, np.asarray(lens)).astype(np.int64) for _ in range(3))
    m = _model(torch.float32)
    args = SimpleNamespace(gpu=0, category2part=c2p)
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.3)
    with contextlib.redirect_stdout(io.StringIO()):
        out = evaluate.validate_partseg(loader, _Starts(m, starts), crit, args)
    # every shape alone through the uniform path, the records combined on the host with the ragged batches' point counts
    lone = evaluate.PartsegMetrics(c2p, 0.3)
    model = _Starts(m, starts)
    with torch.no_grad():
        for pc, cls, seg, L in batches:
            for b, n in enumerate(L.tolist()):
                onehot = evaluate.to_categorical(cls[b:b + 1], len(c2p))
                lone.update(model(pc[b:b + 1, :n].contiguous(), onehot), seg[b:b + 1, :n].contiguous())
    want = evaluate.finalize_partseg(lone.records.host(), [(4, 704, sum(lens[:4])), (2, 704, sum(lens[4:]))], c2p)
    for k in ("acc", "mean_inst_iou", "n", "nonfinite_rows", "category_counts"):
        assert out[k] == want[k], (k, out[k], want[k])
    assert V.same_bits(out["mean_class_iou"], want["mean_class_iou"])
    assert V.same_bits(list(out["category_ious"].values()), list(want["category_ious"].values()))
    assert abs(out["loss"] - want["loss"]) <= 1e-6 * want["loss"]


def test_default_loader_on_a_ragged_part_set_is_unchanged():
    """without ragged=True: the resampled batches, three elements, the same bits run after run for a fixed seed"""
    from ppt_amd.data import DeviceBatchLoader
    cset, lens, _ = _shape_set()
    runs = []
    for _ in range(2):
        ld = DeviceBatchLoader(cset, 4, 256, "shapenetpart", True, shuffle=True, seed=5)
        assert not ld.ragged and ld.plan() == ("cloud_draws", "cloud_prep")
        runs.append([tuple(t.clone() for t in b) for b in ld])
    assert all(len(b) == 3 and tuple(b[0].shape)[1:] == (256, 3) and tuple(b[2].shape)[1:] == (256,) for b in runs[0])
    assert all(torch.equal(x, y) for a, b in zip(*runs) for x, y in zip(a, b))
