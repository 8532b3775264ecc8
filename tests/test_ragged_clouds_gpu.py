"""GPU: clouds of differing length in one batch -- per-cloud row counts through FPS, kNN grouping and the ball queries
(ppt_fps_ragged_f32, ppt_knn_group_ragged_f32, ppt_ball_query{,_multi}_ragged_f32), the loader's ragged=True and the lengths=
argument of PointBERT / PointNet++.

The yardstick for index work is the C oracle called per cloud on pc[b:b+1, :n] (what pins the uniform kernels to the reference):
every index comparison is np.array_equal.  The padding rows of every input are NaN, so a single read behind a cloud's end shows
in the output.  Encoder bounds are the ones the uniform tests of the same mode already hold (tests/test_model_gpu.py)."""
import contextlib
import io
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import oracle as O
from ppt_amd import weights as W

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def ragged(Nmax, lengths, seed):
    """-> (pc [B, Nmax, 3] with NaN behind every cloud's end, start [B] below each length, lengths int32 [B])"""
    lengths = np.asarray(lengths, dtype=np.int32)
    pc, start = W.synth_clouds(len(lengths), Nmax, seed=seed)
    for b, n in enumerate(lengths):
        pc[b, n:] = np.nan
    return pc, start % lengths, lengths


def rows_of(pc, b, idx, n):
    """pc[b, min(idx, n-1)]: the gather of the grouped outputs (the fill value n of an empty ball clamps to the last row)"""
    return pc[b][np.minimum(idx, n - 1)]


# ------------------------------------------------------------------ FPS
@pytest.mark.parametrize("Nmax,lengths,M", [(300, [300, 257, 64, 1, 37], 48),          # n < M, n = 1, n = Nmax
                                            (1100, [1100, 1024, 513, 70], 128),        # a wider template
                                            (12500, [12500, 9000], 16)])               # the variant without the cloud in LDS
def test_fps_ragged_equals_the_oracle_per_cloud(Nmax, lengths, M):
    from ppt_amd import ops
    pc, start, L = ragged(Nmax, lengths, seed=7)
    idx, ctr = ops.fps(dev(pc), M, dev(start), lengths=dev(L))
    idx, ctr = host(idx), host(ctr)
    for b, n in enumerate(L):
        want = O.fps(pc[b:b + 1, :n], M, start[b:b + 1])[0]
        assert np.array_equal(idx[b], want), (b, n)
        assert np.array_equal(ctr[b], pc[b, want]), (b, n)
        if n == 1:
            assert not idx[b].any()                                  # a lone point: index 0 from then on


def test_fps_ragged_all_duplicates_takes_the_tie_path():
    from ppt_amd import ops
    pc = np.tile(np.array([0.25, -0.5, 0.125], dtype=np.float32), (1, 300, 1))
    pc[0, 200:] = np.nan
    start = np.array([137], dtype=np.int64)
    idx, ctr = ops.fps(dev(pc), 24, dev(start), lengths=dev(np.array([200], dtype=np.int32)))
    want = O.fps(pc[:, :200], 24, start)[0]
    assert np.array_equal(host(idx)[0], want) and np.array_equal(host(ctr)[0], pc[0, want])


# ------------------------------------------------------------------ kNN grouping
def _knn_check(pc, L, ctr, k, idx, nb):
    for b, n in enumerate(L):
        want, _ = O.knn(pc[b:b + 1, :n], ctr[b:b + 1], k)
        assert np.array_equal(idx[b], want[0]), (b, n)
        assert np.array_equal(nb[b], pc[b][want[0]] - ctr[b][:, None, :]), (b, n)


def test_knn_ragged_equals_the_oracle_per_cloud():
    from ppt_amd import ops
    G, k = 16, 32
    pc, _, L = ragged(300, [300, 64, 33, 32], seed=11)                                 # n = k
    ctr = np.stack([pc[b, (np.arange(G) * 7) % n] for b, n in enumerate(L)])
    idx, nb = ops.knn_group(dev(pc), dev(ctr), k, lengths=dev(L))
    _knn_check(pc, L, ctr, k, host(idx), host(nb))


def test_knn_ragged_fallback_on_a_cloud_of_identical_points():
    """cloud 1 is 700 copies of one point: every distance ties, the survivor list overflows and the k-round path runs at n = 700"""
    from ppt_amd import ops
    G, k = 16, 32
    pc, _, L = ragged(1024, [1024, 700], seed=12)
    pc[1, :700] = np.array([0.5, 0.25, -0.125], dtype=np.float32)
    ctr = np.stack([pc[b, (np.arange(G) * 7) % n] for b, n in enumerate(L)])
    ctr[1, 1:] += np.float32(0.03125)                                                  # centres off the point as well as on it
    idx, nb = ops.knn_group(dev(pc), dev(ctr), k, lengths=dev(L))
    _knn_check(pc, L, ctr, k, host(idx), host(nb))


def test_knn_ragged_shorter_than_k_stays_inside_the_cloud():
    """k <= lengths[b] is the caller's precondition; a cloud that breaks it gets its n neighbours in order and slot 0's neighbour
    behind them (memory safety, not a reference semantic): nothing of the NaN padding is read"""
    from ppt_amd import ops
    G, k, n = 4, 32, 8
    pc, _, L = ragged(64, [n], seed=13)
    ctr = pc[:, :G].copy()
    idx, nb, nd = ops.knn_group(dev(pc), dev(ctr), k, want_dist=True, lengths=dev(L))
    idx, nb, nd = host(idx), host(nb), host(nd)
    want, _ = O.knn(pc[:, :n], ctr, n)
    assert np.array_equal(idx[0, :, :n], want[0])
    assert np.array_equal(nb[0, :, :n], pc[0][want[0]] - ctr[0][:, None, :])
    assert np.array_equal(idx[0, :, n:], np.repeat(idx[0, :, :1], k - n, axis=1))
    assert np.array_equal(nb[0, :, n:], np.repeat(nb[0, :, :1], k - n, axis=1))
    assert np.array_equal(nd[0, :, n:], np.repeat(nd[0, :, :1], k - n, axis=1))
    assert not np.isnan(nb).any() and not np.isnan(nd).any()


# ------------------------------------------------------------------ ball query
BALLS = [(0.1, 16), (0.2, 32), (0.4, 128)]


@pytest.fixture(scope="module")
def ball_case():
    S = 32
    pc, _, L = ragged(1024, [1024, 600, 50], seed=17)
    ctr = np.stack([pc[b, (np.arange(S) * 13) % n] for b, n in enumerate(L)])
    ctr[:, S - 1] = 9.0                                                                # nothing inside: the fill value is the cloud's n
    want = [[O.ball_query(pc[b:b + 1, :n], ctr[b:b + 1], r, K)[0] for b, n in enumerate(L)] for r, K in BALLS]
    for w in want:
        for b, n in enumerate(L):
            assert (w[b][S - 1] == n).all()
    return pc, L, ctr, want


def _ball_check(pc, L, ctr, want, idx, g):
    for b, n in enumerate(L):
        assert np.array_equal(idx[b], want[b]), (b, n)
        assert np.array_equal(g[b], rows_of(pc, b, want[b], n) - ctr[b][:, None, :]), (b, n)


def test_ball_query_ragged_equals_the_oracle_per_cloud(ball_case):
    from ppt_amd import ops
    pc, L, ctr, want = ball_case
    for (r, K), w in zip(BALLS, want):
        idx, g = ops.ball_query(dev(pc), dev(ctr), r, K, want_grouped=True, lengths=dev(L))
        _ball_check(pc, L, ctr, w, host(idx), host(g))
        assert np.array_equal(host(ops.ball_query(dev(pc), dev(ctr), r, K, lengths=dev(L))), host(idx))


def test_ball_query_multi_ragged_equals_the_oracle_per_cloud(ball_case):
    from ppt_amd import ops
    pc, L, ctr, want = ball_case
    outs = ops.ball_query_multi(dev(pc), dev(ctr), BALLS, want_grouped=True, lengths=dev(L))
    for (idx, g), w in zip(outs, want):
        _ball_check(pc, L, ctr, w, host(idx), host(g))
    for (idx, g), w in zip(ops.ball_query_multi(dev(pc), dev(ctr), BALLS, lengths=dev(L)), want):
        assert g is None and all(np.array_equal(host(idx)[b], w[b]) for b in range(len(L)))


# ------------------------------------------------------------------ unchanged behaviour
def test_full_lengths_give_the_uniform_launch_bytes():
    from ppt_amd import ops
    B, N, S = 3, 300, 16
    pc_np, start = W.synth_clouds(B, N, seed=19)
    pc, st, full = dev(pc_np), dev(start), dev(np.full(B, N, dtype=np.int32))
    ctr = pc[:, :S].contiguous()

    def same(a, b):
        a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
        return all(torch.equal(x, y) for x, y in zip(a, b))
    assert same(ops.fps(pc, 40, st), ops.fps(pc, 40, st, lengths=full))
    assert same(ops.knn_group(pc, ctr, 32, want_dist=True), ops.knn_group(pc, ctr, 32, want_dist=True, lengths=full))
    assert same(ops.ball_query(pc, ctr, 0.2, 32, want_grouped=True), ops.ball_query(pc, ctr, 0.2, 32, want_grouped=True, lengths=full))
    for u, r in zip(ops.ball_query_multi(pc, ctr, BALLS, want_grouped=True), ops.ball_query_multi(pc, ctr, BALLS, want_grouped=True, lengths=full)):
        assert same(u, r)


# ------------------------------------------------------------------ loader
NPOINTS = 32


def _cloud_list(with_exact):
    rng = np.random.default_rng(23)
    lens = [96, 64, 80, 33, 64, 96, 33, 80, 96, 64, 33, 80]
    if with_exact:
        lens[4] = NPOINTS
    return [rng.standard_normal((n, 3)).astype(np.float32) for n in lens]


def _nan_padded_set(clouds):
    """the set DeviceCloudSet(list) builds, with NaN instead of zeros behind every cloud's end"""
    from ppt_amd.data import DeviceCloudSet
    lens = np.asarray([len(c) for c in clouds], dtype=np.int32)
    pts = np.full((len(clouds), int(lens.max()), 3), np.nan, dtype=np.float32)
    for i, c in enumerate(clouds):
        pts[i, :len(c)] = c
    return DeviceCloudSet(pts, np.arange(len(clouds)) % 40, lengths=lens)


def _expected(clouds, recipe, train, seed, batch):
    """every cloud on its own: the draws in batch order, oracle FPS at the cloud's length, the existing ops.cloud_prep"""
    from ppt_amd import ops
    from ppt_amd.data import numpy_draws
    rs = np.random.RandomState([seed, 0, 0])
    out = []
    for c in clouds:
        d = numpy_draws(rs, recipe, train, len(c), NPOINTS)
        sel = O.fps(c[None], NPOINTS, np.array([d["start"]]))[0] if "start" in d else np.arange(NPOINTS)
        kw = dict(scale=dev(d["scale"][None]), shift=dev(d["shift"][None]), perm=dev(d["perm"][None].astype(np.int32))) if "scale" in d else {}
        out.append(host(ops.cloud_prep(dev(c[None]), dev(np.zeros(1, np.int64)), NPOINTS, sel=dev(sel[None]), normalize=True, **kw))[0])
    return np.stack(out)


def test_loader_ragged_modelnet_numpy_draws_equal_the_per_cloud_batches():
    from ppt_amd.data import DeviceBatchLoader
    clouds = _cloud_list(with_exact=True)
    ld = DeviceBatchLoader(_nan_padded_set(clouds), 5, NPOINTS, "modelnet", True, shuffle=False, seed=41, draws="numpy", ragged=True)
    assert ld.plan() == ("fps", "cloud_prep")
    got = host(torch.cat([b[0] for b in ld]))
    want = _expected(clouds, "modelnet", True, 41, 5)
    assert np.array_equal(got, want)
    # the cloud of exactly npoints rows comes through unsampled: pc_normalize of its stored rows, translated and shuffled
    ld = DeviceBatchLoader(_nan_padded_set(clouds), 5, NPOINTS, "modelnet", False, shuffle=False, seed=41, draws="numpy", ragged=True)
    from ppt_amd.data import pc_normalize
    got = host(torch.cat([b[0] for b in ld]))
    assert np.array_equal(got[4], pc_normalize(clouds[4]))
    assert np.array_equal(got, _expected(clouds, "modelnet", False, 41, 5))


@pytest.mark.parametrize("batch", [1, 2, 3])
@pytest.mark.parametrize("train", [True, False])
def test_loader_ragged_batches_made_of_unsampled_clouds_only(batch, train):
    """numpy draws: a batch whose clouds all have exactly npoints rows draws no FPS start at all (batch 1: the clouds on their own;
    batch 2: the last, partial batch; batch 3: clouds 3 .. 5) -- it still comes out as the per-cloud expectation"""
    from ppt_amd.data import DeviceBatchLoader
    rng = np.random.default_rng(27)
    clouds = [rng.standard_normal((n, 3)).astype(np.float32) for n in (96, NPOINTS, 80, NPOINTS, NPOINTS, NPOINTS, NPOINTS)]
    ld = DeviceBatchLoader(_nan_padded_set(clouds), batch, NPOINTS, "modelnet", train, shuffle=False, seed=13, draws="numpy", ragged=True)
    got = host(torch.cat([b[0] for b in ld]))
    assert np.array_equal(got, _expected(clouds, "modelnet", train, 13, batch))


def test_loader_ragged_device_draws_repeat_and_stay_inside_each_cloud(monkeypatch):
    from ppt_amd import ops
    from ppt_amd.data import DeviceBatchLoader
    seen = []
    real = ops.fps

    def spy(xyz, M, start, lengths=None):
        idx, ctr = real(xyz, M, start, lengths=lengths)
        seen.append((idx, start, lengths))
        return idx, ctr
    monkeypatch.setattr(ops, "fps", spy)
    ld = DeviceBatchLoader(_nan_padded_set(_cloud_list(with_exact=True)), 5, NPOINTS, "modelnet", True, shuffle=True, seed=3, draws="device", ragged=True)
    assert ld.plan() == ("cloud_draws", "fps", "cloud_prep")
    a = [tuple(t.clone() for t in b) for b in ld]
    b = [tuple(t.clone() for t in b) for b in ld]
    assert len(a) == len(ld) == 3
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))
    assert all(torch.isfinite(x[0]).all() for x in a)
    assert len(seen) == 6
    for idx, start, lengths in seen:
        assert lengths is not None and lengths.dtype == torch.int32
        assert bool((idx < lengths.long()[:, None]).all()) and bool((start < lengths.long()).all()) and bool((idx >= 0).all())


def test_loader_ragged_shapenet55_test_split():
    from ppt_amd.data import DeviceBatchLoader
    clouds = _cloud_list(with_exact=False)
    ld = DeviceBatchLoader(_nan_padded_set(clouds), 4, NPOINTS, "shapenet55", False, shuffle=False, seed=9, draws="numpy", ragged=True)
    got = host(torch.cat([b[0] for b in ld]))
    assert np.array_equal(got, _expected(clouds, "shapenet55", False, 9, 4))


# ------------------------------------------------------------------ encoders
def _pointbert(head_type):
    from test_model_gpu import build
    return build(head_type, torch.float32)


def test_pointbert_ragged_matches_the_oracle_per_cloud():
    """fp32 mode, eval: the absolute feature bound test_eval_forward_matches_golden holds for this mode, 5e-4"""
    m, sd = _pointbert(0)
    m.eval()
    pc, start, L = ragged(1024, [1024, 700, 300], seed=29)
    pe = m.point_encoder
    pe.fps_start = dev(start)
    with torch.no_grad():
        feat = host(pe(dev(pc), lengths=[1024, 700, 300]))
        feat_dev = host(pe(dev(pc), lengths=dev(L)))                 # the device form: the same launches
        logits = m(dev(pc), lengths=L)
    assert np.array_equal(feat, feat_dev) and tuple(logits.shape) == (3, 40) and bool(torch.isfinite(logits).all())
    with torch.no_grad():
        ref = np.concatenate([O.point_transformer(sd, torch.from_numpy(pc[b:b + 1, :n]), start[b:b + 1]).numpy() for b, n in enumerate(L)])
    err = np.abs(feat - ref).max(axis=1)
    print("PARITY ragged PointBERT feature abs err per cloud:", err, "(bound 5e-4)")
    assert err.max() < 5e-4


@pytest.mark.parametrize("kind", ["msg", "ssg"])
def test_pointnet2_ragged_matches_the_oracle_per_cloud(kind):
    """fp32 mode, eval: test_pointnet2_msg_matches_golden's own bound, 2e-3 of max|ref|"""
    from ppt_amd.models.pointnet2 import pointnet2 as P
    cls, spec, oracle = {"msg": (P.Pointnet2_Msg, W.pointnet2_msg_spec, O.pointnet2_msg),
                         "ssg": (P.Pointnet2_Ssg, W.pointnet2_ssg_spec, O.pointnet2_ssg)}[kind]
    m = cls()
    sd = W.synth_state_dict(spec(prefix=""), seed=0)
    m.load_state_dict(sd)
    m.cuda().eval()
    m.precision = torch.float32
    pc, s1, L = ragged(1024, [1024, 600], seed=31)
    _, s2 = W.synth_clouds(2, 512, seed=32)
    m.fps_start = (dev(s1), dev(s2))
    out = m(dev(pc), lengths=L).cpu()
    with torch.no_grad():
        ref = torch.cat([oracle(sd, torch.from_numpy(pc[b:b + 1, :n]), (s1[b:b + 1], s2[b:b + 1]), prefix="") for b, n in enumerate(L)])
    err = (out - ref).abs().max().item() / max(ref.abs().max().item(), 0.05)
    print(f"PARITY ragged pn2{kind} abs err / max|ref|: {err:.4g} (bound 2e-3)")
    assert err < 2e-3


def test_training_path_with_full_lengths_is_bit_equal():
    """ULIP_PointBERT, head_type 3, eager: forward + a plain loss.backward() with lengths = [N, N] and without -- the grouping
    stage is the only thing lengths touches, so logits and every trainable gradient have the same bits"""
    m, _ = _pointbert(3)
    m.train()
    m.use_hip_graphs = False
    m.point_encoder.use_hip_graphs = False
    pc_np, start = W.synth_clouds(2, 1024, seed=37)
    pc, labels = dev(pc_np), torch.tensor([3, 17]).cuda()
    rng = np.random.default_rng(0)
    m.point_encoder.fps_start = dev(start)
    m.point_encoder.drop_path_factors = dev((np.floor(0.9 + rng.random((12, 2, 2))) / 0.9).astype(np.float32))
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.2)
    runs = []
    for lengths in ([1024, 1024], None):
        m.zero_grad(set_to_none=True)
        logits = m(pc) if lengths is None else m(pc, lengths=lengths)
        crit(logits, labels).backward()
        torch.cuda.synchronize()
        runs.append((logits.detach().clone(), {k: q.grad.detach().clone() for k, q in m.named_parameters() if q.requires_grad}))
    assert len(runs[0][1]) > 4 and sorted(runs[0][1]) == sorted(runs[1][1])
    assert torch.equal(runs[0][0], runs[1][0])
    for k, g in runs[0][1].items():
        assert torch.equal(g, runs[1][1][k]), k


def test_encoders_that_normalise_over_all_rows_refuse_lengths():
    from ppt_amd.models import ULIP_models as M
    kw = dict(template_init='', class_name_position='middle', num_learnable_prompt_tokens=32, gpu=0, head_type=0, evaluate_3d=False,
              ulip2=False, synthetic_weights=True)
    pc = dev(W.synth_clouds(2, 1024, seed=41)[0])
    with contextlib.redirect_stdout(io.StringIO()):
        part = M.ULIP_PointBERT_partseg(SimpleNamespace(classnames=M.dataset_classnames("shapenetpart"), task='partseg', **kw))
    part.load_state_dict(W.ulip_partseg_state_dict(seed=0), strict=False)
    part.prompt_learner.embedding = W.synth_prompt_embedding(50, seed=0)
    part.cuda().eval()
    onehot = torch.zeros(2, 16, device="cuda")
    onehot[:, 3] = 1
    with pytest.raises(ValueError, match="lengths"):
        part(pc, onehot, lengths=[1024, 700])
    mlp = M.ULIP_PN_MLP(SimpleNamespace(classnames=M.dataset_classnames("modelnet40"), task='cls', **kw))
    mlp.load_state_dict(W.ulip_pn_mlp_state_dict(seed=0), strict=False)
    mlp.cuda().eval()
    with pytest.raises(ValueError, match="lengths"):
        mlp(pc, lengths=[1024, 700])
    m, _ = _pointbert(0)
    with pytest.raises(ValueError, match="lengths"):
        m.forward_loss(pc, torch.tensor([1, 2]).cuda(), 0.2, lengths=[1024, 700])
    from ppt_amd.train import Trainer
    with pytest.raises(ValueError, match="lengths"):
        Trainer(m, distributed=False).step(pc, torch.tensor([1, 2]).cuda(), lengths=[1024, 700])
