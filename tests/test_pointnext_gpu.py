"""GPU: the PointNeXt-S encoder (csrc/pointnext.hip, engine.pointnext_forward, models/pointnext) against the reference outputs of
tests/golden/g_pointnext.npz and the fp64 restatement of tests/pointnext_ref.py.

Bounds (none of them comes from the code under test):
  fp32 / split16 forward and running statistics: 8 x ref_err of the case -- ref_err is the reference's own distance from the fp64
    restatement, the factor 8 is room for the device's other summation order;
  mixed mode: 4 x e16 of the case and format -- e16 is the distance of the restatement with operands rounded to that format from the
    fp64 restatement; measured against the fp64 restatement, never against another mode of the code under test;
  indices, pool_res_finish, cloud_height, graph replay, the ahead stage: exact."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pointnext_ref as P
from ppt_amd import weights as W
from test_pointnext_cpu import CASES, case_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g_pointnext.npz")))


@pytest.fixture(scope="module")
def ops():
    from ppt_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def sd():
    return W.synth_state_dict(W.pointnext_spec(prefix=""), seed=0)


@pytest.fixture(scope="module")
def ref64(g, sd):
    """The fp64 restatement of every golden case, computed once: tag -> output [B,256] float64 array."""
    out = {}
    for tag in CASES:
        pc, train, masks = case_inputs(g, tag)
        out[tag] = P.forward(sd, pc, train, masks, dtype=torch.float64)[0].numpy()
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def build(sd, precision, train=False, masks=None, graphs_on=False):
    from ppt_amd.models.pointnext.pointnext import PointNEXT
    m = PointNEXT()
    m.load_state_dict(sd)
    m.cuda()
    m.precision = torch.float32 if precision in ("fp32", "split16") else torch.bfloat16
    m.split16 = precision == "split16"
    m.use_hip_graphs = graphs_on
    m.train(train)
    if masks is not None:
        m.dropout_masks = tuple(torch.from_numpy(x) for x in masks)
    return m


# ------------------------------------------------------------------------------------------------ indices
def test_grouping_indices_equal_the_recorded_tensors(g):
    """FPS from index 0 and the strict ball query of all four stages on the N = 200 eval clouds (duplicates, the boundary point):
    every index equal to the fixture's."""
    from ppt_amd import engine
    pc = g["pc_n200"]
    out = engine.pointnext_group(dev(pc[..., :3]))
    N = pc.shape[1]
    for i in range(4):
        rows, new_xyz, nidx = out[3 * i:3 * i + 3]
        B, S, K = nidx.shape
        cidx = (rows.view(B, S) - torch.arange(B, device="cuda").view(B, 1) * N).cpu().numpy()
        assert (S, K) == (N // 2, 32)
        assert np.array_equal(cidx, g[f"fps{i}"].astype(np.int64)), i
        assert np.array_equal(nidx.cpu().numpy(), g[f"ball{i}"].astype(np.int64)), i
        N = S
    assert 1 not in out[2][2, 0].tolist() and 0 in out[2][2, 0].tolist()      # `<`: the point at distance exactly r stays outside


def _ball_case(name, g):
    rng = np.random.default_rng(11)
    if name == "n200":                          # the fixture's clouds, centres = every second point
        xyz = g["pc_n200"][..., :3]
        return xyz, xyz[:, ::2], 0.15, 32
    if name == "n67":                           # no multiple of 64, more than one centre tile, K close to S
        xyz = W.synth_clouds(2, 67, seed=21)[0]
        return xyz, xyz[:, :33] + np.float32(0.01), 0.5, 32
    if name == "n1":                            # K larger than N; the single point is its own centre
        xyz = rng.random((2, 1, 3), dtype=np.float32)
        return xyz, xyz.copy(), 0.15, 32
    if name == "empty":                         # nothing inside: all indices 0
        xyz = rng.random((1, 70, 3), dtype=np.float32)
        return xyz, xyz[:, :5] + np.float32(10.0), 0.15, 16
    if name == "boundary":                      # points at distance exactly float32(r) along each axis, both directions
        r = np.float32(0.225)
        c = np.zeros((1, 1, 3), np.float32)
        pts = np.concatenate([np.eye(3, dtype=np.float32) * r, -np.eye(3, dtype=np.float32) * r,
                              np.eye(3, dtype=np.float32) * np.nextafter(r, np.float32(0)), np.zeros((1, 3), np.float32)])
        return pts[None], c, 0.225, 8
    if name == "duplicates":                    # every point four times: full balls of identical coordinates
        base = W.synth_clouds(1, 40, seed=22)[0]
        xyz = np.tile(base, (1, 4, 1))
        return xyz, base[:, :20].copy(), 0.3375, 64
    raise KeyError(name)


@pytest.mark.parametrize("name", ["n200", "n67", "n1", "empty", "boundary", "duplicates"])
def test_ball_query_lt_equals_the_stand_in(ops, g, name):
    xyz, ctr, r, K = _ball_case(name, g)
    xyz, ctr = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(ctr, np.float32)
    want = P.ball_query_lt(xyz, ctr, r, K)
    idx, gx = ops.ball_query_lt(dev(xyz), dev(ctr), r, K, want_grouped=True)
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(ops.ball_query_lt(dev(xyz), dev(ctr), r, K).cpu().numpy(), want)
    B = xyz.shape[0]
    gw = xyz[np.arange(B)[:, None, None], want] - ctr[:, :, None, :]
    assert np.array_equal(gx.cpu().numpy(), gw)
    if name == "boundary":
        assert sorted(set(want[0, 0].tolist())) == [6, 7, 8, 9]
    if name == "empty":
        assert not want.any()


@pytest.mark.parametrize("N", [200, 67, 1])
def test_fps_from_zero_equals_the_stand_in(ops, g, N):
    # (N = 1: a cloud of one point cannot be normalised to the unit sphere -- plain uniform draws)
    xyz = g["pc_n200"][..., :3] if N == 200 else np.random.default_rng(23).random((3, N, 3), dtype=np.float32)
    xyz = np.ascontiguousarray(xyz, np.float32)
    S = max(N // 2, 1)
    idx, ctr = ops.fps(dev(xyz), S, torch.zeros(xyz.shape[0], dtype=torch.int64, device="cuda"))
    want = P.fps_from_zero(xyz, S)
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(ctr.cpu().numpy(), np.take_along_axis(xyz, want[:, :, None], 1))


# ------------------------------------------------------------------------------------------------ the two small kernels
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("fold", [1, 2])
@pytest.mark.parametrize("C", [64, 512])
def test_pool_res_finish_is_the_torch_expression(ops, C, fold, out_dtype):
    G = 13
    gen = torch.Generator().manual_seed(C + fold)
    pmax = torch.randn(G * fold, C, generator=gen).cuda()
    pmin = pmax - torch.rand(G * fold, C, generator=gen).cuda()
    scale = torch.randn(C, generator=gen).cuda()                    # about half of them negative
    scale[3] = 0.0
    shift = torch.randn(C, generator=gen).cuda()
    ident = torch.randn(G, C, generator=gen).cuda()
    assert (scale < 0).any() and (scale > 0).any()
    mx, mn = pmax.view(G, fold, C).max(1)[0], pmin.view(G, fold, C).min(1)[0]
    sel = torch.where(scale >= 0, mx, mn)
    want = torch.relu(scale * sel + shift + ident).to(out_dtype)
    got = ops.pool_res_finish(pmax, pmin, fold, scale, shift, ident, out_dtype)
    assert got.dtype == out_dtype and torch.equal(got, want)
    assert torch.equal(ops.pool_res_finish(pmax, pmin, fold, scale, shift, None, out_dtype), torch.relu(scale * sel + shift).to(out_dtype))


@pytest.mark.parametrize("y_dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_gather_add_output_formats_are_exact(ops, y_dtype):
    """ppt_gather_add writes y = P[idx] + Q (one fp32 sum) rounded once to the output format -- IEEE half is the format this encoder
    adds; the BatchNorm partials are those of the un-rounded fp32 rows whatever the format."""
    B, N, S, K, C = 2, 37, 5, 32, 64
    gen = torch.Generator().manual_seed(3)
    Pm = torch.randn(B * N, C, generator=gen).cuda()
    Q = torch.randn(B * S, C, generator=gen).cuda()
    idx = torch.randint(0, N, (B, S, K), generator=gen).cuda()
    y, (ps, pm) = ops.gather_add(Pm, Q, idx, N, y_dtype, want_stats=True)
    rows = (idx + torch.arange(B, device="cuda").view(B, 1, 1) * N).view(-1)
    full = Pm[rows] + Q.repeat_interleave(K, 0)
    assert y.dtype == y_dtype and torch.equal(y, full.to(y_dtype))
    y32, (ps32, pm32) = ops.gather_add(Pm, Q, idx, N, torch.float32, want_stats=True)
    assert torch.equal(ps, ps32) and torch.equal(pm, pm32)


def test_cloud_height_is_the_numpy_expression(ops):
    pc = W.synth_clouds(3, 333, seed=24)[0]
    pc[1, 200, 1] = pc[1, :, 1].min()                               # the minimum occurs twice
    assert (pc[1, :, 1] == pc[1, :, 1].min()).sum() == 2
    want = np.stack([np.concatenate((c, c[:, 1:2] - c[:, 1:2].min()), axis=1) for c in pc])
    assert np.array_equal(ops.cloud_height(dev(pc)).cpu().numpy(), want)
    one = np.float32([[[0.5, -2.0, 1.0]]])
    assert np.array_equal(ops.cloud_height(dev(one)).cpu().numpy(), np.float32([[[0.5, -2.0, 1.0, 0.0]]]))


def test_loader_use_height_adds_the_column_to_the_finished_cloud():
    """DeviceBatchLoader(use_height=True): [B,n,4]; the first three columns are what the same loader yields without it (same seed:
    same augmentation and shuffle), the fourth is their height."""
    from ppt_amd.data.device_loader import DeviceBatchLoader, DeviceCloudSet
    pts = W.synth_clouds(6, 96, seed=25)[0]
    cs = DeviceCloudSet(pts, np.arange(6, dtype=np.int64))
    kw = dict(batch_size=4, npoints=64, recipe="scanobjectnn", train=True, shuffle=True, seed=3)
    plain = [(pc.cpu().numpy(), t.cpu().numpy()) for pc, t in DeviceBatchLoader(cs, **kw)]
    tall = [(pc.cpu().numpy(), t.cpu().numpy()) for pc, t in DeviceBatchLoader(cs, use_height=True, **kw)]
    assert [p.shape for p, _ in tall] == [(4, 64, 4), (2, 64, 4)]
    for (p3, t3), (p4, t4) in zip(plain, tall):
        assert np.array_equal(t3, t4) and np.array_equal(p4, P.cloud_height(p3))


# ------------------------------------------------------------------------------------------------ forward
def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("precision", ["fp32", "split16"])
@pytest.mark.parametrize("tag", CASES)
def test_forward_matches_the_reference(g, sd, tag, precision):
    pc, train, masks = case_inputs(g, tag)
    m = build(sd, precision, train, masks)
    out = m(dev(pc)).cpu().numpy()
    bound = 8 * float(g["ref_err_" + tag])
    err = _rel(out, g[tag])
    print(f"PARITY pointnext {tag} {precision}: err / max|ref| {err:.3g} (bound {bound:.3g}, ref_err {float(g['ref_err_' + tag]):.3g})")
    worst = ("", 0.0)
    if train:
        msd = m.state_dict()
        pre = f"stat.{tag}."
        for k in g:
            if k.startswith(pre):
                e = _rel(msd[k[len(pre):]].cpu().numpy(), g[k])
                worst = max(worst, (k[len(pre):], e), key=lambda t: t[1])
        print(f"PARITY pointnext {tag} {precision}: worst running statistic {worst[0]} {worst[1]:.3g}")
        assert int(msd["encoder.encoder.3.0.convs.1.1.num_batches_tracked"]) == 1
    assert out.shape == g[tag].shape and err <= bound
    assert worst[1] <= bound, worst


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("tag", CASES)
def test_mixed_mode_forward_against_fp64(g, sd, ref64, tag, fmt, monkeypatch):
    from ppt_amd import engine
    monkeypatch.setattr(engine, "POINTNEXT_F16", fmt == "f16")       # PPT_POINTNEXT_F16: the operand format of the mixed mode
    pc, train, masks = case_inputs(g, tag)
    m = build(sd, "mixed16", train, masks)
    out = m(dev(pc)).cpu().numpy()
    assert m._wc.dtype == (torch.float16 if fmt == "f16" else torch.bfloat16)
    e16 = float(g[f"e16_{fmt}_{tag}"])
    err = _rel(out.astype(np.float64), ref64[tag])
    print(f"PARITY pointnext {tag} mixed {fmt}: err / max|fp64| {err:.3g} (bound {4 * e16:.3g}, e16 {e16:.3g})")
    assert err <= 4 * e16


def test_mixed_mode_does_not_follow_the_process_wide_split16_switch(g, sd, ops):
    """The 16-bit modes run their fp32 coordinate GEMMs (K = 4) on the fp32 MFMA whatever another model left in ops.set_split16:
    the same bits either way, so a captured graph and an eager call cannot differ by call history."""
    pc, _, _ = case_inputs(g, "eval_n200")
    outs = []
    try:
        for on in (False, True):
            m = build(sd, "mixed16")
            ops.set_split16(on)
            outs.append(m(dev(pc)))
            assert ops.split16_enabled() == on                 # ... and the encoder leaves the switch as it found it
    finally:
        ops.set_split16(False)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("train", [False, True])
def test_graph_replay_and_ahead_stage_equal_eager(g, sd, train):
    from ppt_amd import graphs
    pc, _, masks = case_inputs(g, "train")
    masks = masks if train else None
    x = dev(pc)
    eager = build(sd, "mixed16", train, masks)(x)
    results = []
    for ahead in (False, True):
        m = build(sd, "mixed16", train, masks, graphs_on=True)
        if ahead:
            m.group_ahead = graphs.shared_group_stream()
        # (train mode normalises with the batch statistics: the running buffers the earlier calls moved do not enter the output)
        for _ in range(graphs.WARMUP_CALLS + 4):           # eager warm-up, capture (both slots of the ahead stage), replays
            out = m(x)
        torch.cuda.synchronize()
        kinds = sorted(str(k[0]) for k in m._graphs.entries)
        assert kinds == (["pointnext", "pointnext_group", "pointnext_group"] if ahead else ["pointnext"]), kinds
        results.append(out)
    assert torch.equal(results[0], eager) and torch.equal(results[1], eager)


# ------------------------------------------------------------------------------------------------ the factory
def test_ulip_pn_next_step_and_validate(g):
    from ppt_amd.models import ULIP_models as M
    from ppt_amd.train import Trainer
    names = M.dataset_classnames("modelnet40")[:5]
    args = SimpleNamespace(classnames=names, template_init='', class_name_position='middle', num_learnable_prompt_tokens=32, gpu=0,
                           task='cls', head_type=0, evaluate_3d=False, ulip2=False, synthetic_weights=True)
    m = M.ULIP_PN_NEXT(args)
    m.load_state_dict(W.ulip_pn_next_state_dict(seed=0), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding(5, seed=0)
    m.cuda().train()
    pc = dev(g["pc_train"][:4])
    label = torch.tensor([0, 3, 1, 4], device="cuda")
    with pytest.raises(ValueError, match="use_height"):
        m.point_encoder(pc[..., :3])
    before = {k: v.clone() for k, v in m.state_dict().items()}
    tr = Trainer(m, distributed=False)
    loss, pred = tr.step(pc, label)
    tr.finish()
    assert np.isfinite(loss.item()) and pred.shape == (4, 5)
    after = m.state_dict()
    changed = {k for k in before if before[k].dtype.is_floating_point and not torch.equal(before[k], after[k]) and "running_" not in k}
    assert changed == {"prompt_learner.learnable_tokens"}, changed
    grads = {n for n, p in m.named_parameters() if p.grad is not None}
    assert grads == {"prompt_learner.learnable_tokens"}, grads                 # every other parameter's .grad is None
    tg = m.prompt_learner.learnable_tokens.grad
    assert torch.isfinite(tg).all() and tg.abs().max().item() > 0
    m.eval()
    batches = [(dev(g["pc_train"][:4]), label), (dev(g["pc_train"][4:]), label)]
    stats = M.validate(batches, m, torch.nn.CrossEntropyLoss(), SimpleNamespace(gpu=0, classnames=names))
    assert stats["n"] == 8 and np.isfinite(stats["loss"]) and 0.0 <= stats["acc"] <= 100.0
