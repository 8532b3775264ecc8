"""GPU: csrc/render.hip and ppt_amd/viz.py against the numpy restatements of tests/viz_ref.py.  The renderer is compared with
np.array_equal -- integer depths, exact double products and a defined tie rule leave no room for a tolerance; the per-point
predictions against argmax over the category's columns and against the counts ppt_partseg_metrics makes of the same logits."""
import contextlib
import io
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import viz_ref as R

pytestmark = pytest.mark.gpu


def _render(ixyz, colors, H, W, r, bg):
    from ppt_amd import ops
    return ops.render_balls(torch.tensor(ixyz).cuda(), torch.tensor(colors).cuda(), H, W, r, bg)         # (copies: the cases are read-only)


@pytest.mark.parametrize("name", list(R.RENDER_CASES))
def test_render_equals_the_restatement(name):
    c = R.render_case(name)
    for bg in R.BACKGROUNDS:
        got = _render(c["ixyz"][None], c["colors"][None], c["H"], c["W"], c["r"], bg)
        assert got.shape == (1, 2, c["H"], c["W"], 3) and got.dtype == torch.uint8
        got = got.cpu().numpy()[0]
        want = c["pictures"][bg]
        bad = np.argwhere((got != want).any(-1))
        assert np.array_equal(got, want), (name, bg, len(bad), bad[:5])
    share = (c["win"] < 0).mean()
    print(f"VIZ {name}: background share {share:.3f}")
    if name in ("small", "wide_ball"):                     # the comparison cannot pass on a blank or a fully covered picture
        assert 0.10 < share < 0.90
        assert ((got[0] == np.asarray(R.BACKGROUNDS[-1], np.uint8)).all(-1)).mean() >= share


@pytest.mark.parametrize("K", [1, 2, 3])
def test_render_three_geometries_in_one_call_and_twice(K):
    """G = 3 geometries with K colourings each in one call; a second call on the same inputs returns the same bytes"""
    H, W, n, r, depth = R.RENDER_CASES["small"]
    geo = [R.make_geometry(H, W, n, r, depth, seed, K) for seed in (21, 22, 23)]
    ixyz, colors = np.stack([g[0] for g in geo]), np.stack([g[1] for g in geo])
    bg = R.BACKGROUNDS[1]
    first = _render(ixyz, colors, H, W, r, bg)
    second = _render(ixyz, colors, H, W, r, bg)
    assert first.shape == (3, K, H, W, 3)
    assert torch.equal(first, second)
    got = first.cpu().numpy()
    for g in range(3):
        want, _ = R.render_vectorised(ixyz[g], colors[g], H, W, r, bg)
        assert np.array_equal(got[g], want), g


def test_render_through_viz_and_caller_owned_buffers():
    """viz.render_balls over leading axes [B, V] with and without a K axis; ops.render_balls into the caller's output and
    workspace"""
    from ppt_amd import ops, viz
    H, W, n, r, depth = R.RENDER_CASES["small"]
    geo = [R.make_geometry(H, W, n, r, depth, seed, 2) for seed in (31, 32, 33, 34)]
    ixyz = torch.from_numpy(np.stack([g[0] for g in geo]).reshape(2, 2, n, 3)).cuda()
    colors = torch.from_numpy(np.stack([g[1] for g in geo]).reshape(2, 2, 2, n, 3)).cuda()
    img = viz.render_balls(ixyz, colors, (H, W), radius=r)
    assert img.shape == (2, 2, 2, H, W, 3)
    for i, g in enumerate(geo):
        want, _ = R.render_vectorised(g[0], g[1], H, W, r, (255, 255, 255))
        assert np.array_equal(img[i // 2, i % 2].cpu().numpy(), want)
    one = viz.render_balls(ixyz, colors[:, :, 1], (H, W), radius=r)
    assert one.shape == (2, 2, H, W, 3) and torch.equal(one, img[:, :, 1])
    out = torch.full((4, 2, H, W, 3), 7, dtype=torch.uint8, device="cuda")
    ws = torch.empty(ops.render_balls_workspace_bytes(4, n, H, W, r), dtype=torch.uint8, device="cuda")
    back = ops.render_balls(ixyz.view(4, n, 3), colors.view(4, 2, n, 3), H, W, r, out=out, workspace=ws)
    assert back is out and torch.equal(out.view(2, 2, 2, H, W, 3), img)


def test_render_limits():
    """radius 17 raises; the entry point itself returns PPT_EUNSUPPORTED for it and for H = 4097 with nothing launched"""
    from ppt_amd import _lib, ops
    c = R.render_case("small")
    with pytest.raises(RuntimeError, match="render_balls"):
        _render(c["ixyz"][None], c["colors"][None], c["H"], c["W"], 17, (255, 255, 255))
    with pytest.raises(RuntimeError, match="render_balls"):
        _render(c["ixyz"][None], c["colors"][None], 4097, c["W"], 4, (255, 255, 255))
    ixyz, colors = torch.from_numpy(c["ixyz"].copy()).cuda(), torch.from_numpy(c["colors"].copy()).cuda()
    out = torch.full((2, 8, 8, 3), 7, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(256, dtype=torch.uint8, device="cuda")
    pat = torch.from_numpy(ops.ball_pattern_host(16)).cuda()
    args = lambda radius, H: (ixyz.data_ptr(), colors.data_ptr(), pat.data_ptr(), bytes([0, 0, 0]), radius, 1, 2, ixyz.shape[0], H, 8,
                              out.data_ptr(), ws.data_ptr(), 256, None)
    assert _lib.lib().ppt_render_balls(*args(17, 8)) == -3
    assert _lib.lib().ppt_render_balls(*args(4, 4097)) == -3
    torch.cuda.synchronize()
    assert (out == 7).all() and (ws == 0).all()


# ---- per-point predictions ----------------------------------------------------------------------------------------------------
def _logits(B, N, seed):
    """values on a grid of 1/4 so that exact ties are common, inside and outside every category's range"""
    rng = np.random.RandomState(seed)
    return (rng.randint(-12, 13, (B, N, 50)) / 4.0).astype(np.float32)


@pytest.mark.parametrize("N", [1, 257, 2048])
def test_predict_parts_equals_the_masked_argmax_and_the_metric_counts(N):
    from ppt_amd import evaluate, ops, viz
    B = 5
    logits = _logits(B, N, seed=N)
    rng = np.random.RandomState(N + 1)
    anchor = np.array([30, 4, 12, 49, 16])                                     # Motorbike (6 parts), Bag, Chair, Table, Earphone
    labels = np.stack([rng.choice(R.CATEGORY2PART[k], N) for k in ("Motorbike", "Bag", "Chair", "Table", "Earphone")]).astype(np.int64)
    labels[:, 0] = anchor
    if N > 4:                                                                  # a whole row of equal logits: the first column of the range
        logits[2, 3, :] = 1.5
    want = R.predict_parts(logits, anchor)
    assert (want >= 0).all()
    lg, lb = torch.from_numpy(logits).cuda(), torch.from_numpy(labels).cuda()
    pred = viz.predict_parts(lg, lb, R.CATEGORY2PART)
    assert pred.dtype == torch.int32 and pred.shape == (B, N)
    assert np.array_equal(pred.cpu().numpy(), want)
    assert torch.equal(viz.predict_parts(lg, lb[:, 0].contiguous(), R.CATEGORY2PART), pred)       # an anchor per cloud
    if N > 4:
        assert int(pred[2, 3]) == 12
    # torch's own statement (show_balls.py:262)
    for b, a in enumerate(anchor):
        parts = [p for v in R.CATEGORY2PART.values() if a in v for p in v]
        assert torch.equal(pred[b].long(), lg[b][:, parts[0]:parts[0] + len(parts)].argmax(-1) + parts[0])
    # one cloud with an anchor that is no part id: -1 for its points, the others untouched
    bad = lb[:, 0].clone()
    bad[1] = 50
    got = viz.predict_parts(lg, bad, R.CATEGORY2PART).cpu().numpy()
    assert (got[1] == -1).all() and np.array_equal(np.delete(got, 1, 0), np.delete(want, 1, 0))
    bad[1] = -1
    assert (viz.predict_parts(lg, bad, R.CATEGORY2PART)[1] == -1).all()
    # ppt_partseg_metrics on the same inputs counts what these predictions say
    m = evaluate.PartsegMetrics(R.CATEGORY2PART, 0.0)
    m.update(lg, lb)
    rec = m.records.host()
    assert np.array_equal(rec[:, 2], (want == labels).sum(1))
    for b in range(B):
        start, count = int(rec[b, 0]), int(rec[b, 1])
        for j in range(ops.PARTSEG_MAX_PARTS):
            part = start + j
            counts = [(labels[b] == part).sum(), (want[b] == part).sum(), ((labels[b] == part) & (want[b] == part)).sum()] \
                if j < count else [0, 0, 0]
            assert rec[b, 8 + 3 * j:11 + 3 * j].tolist() == [int(v) for v in counts], (b, j)


def test_predict_limits_and_determinism():
    from ppt_amd import _lib, evaluate, ops
    lg = torch.from_numpy(_logits(2, 300, seed=3)).cuda()
    anchor = torch.tensor([0, 47], device="cuda")
    start, count = (torch.from_numpy(t).cuda() for t in evaluate.part_tables(R.CATEGORY2PART))
    a = ops.partseg_predict(lg, anchor, start, count)
    out = torch.full((2, 300), 9, dtype=torch.int32, device="cuda")
    assert ops.partseg_predict(lg, anchor, start, count, pred=out) is out and torch.equal(a, out)
    wide = torch.zeros(2, 8, 65, device="cuda")
    tbl = torch.zeros(65, dtype=torch.int32, device="cuda")
    keep = torch.full((2, 8), 9, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="ppt_partseg_predict"):
        ops.partseg_predict(wide, anchor, tbl, tbl, pred=keep)
    torch.cuda.synchronize()
    assert (keep == 9).all()                                                   # nothing was launched
    assert _lib.lib().ppt_partseg_predict(wide.data_ptr(), anchor.data_ptr(), 2, 8, 65, tbl.data_ptr(), tbl.data_ptr(),
                                          keep.data_ptr(), None) == -3


# ---- the contact sheet --------------------------------------------------------------------------------------------------------
class _Recording(torch.nn.Module):
    """hands the model's own logits on and keeps a copy of them"""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, []

    def forward(self, *a):
        out = self.inner(*a)
        self.seen.append(out.detach().clone())
        return out


def test_partseg_sheet_end_to_end():
    """ULIP_PointBERT_partseg on synthetic weights, B = 2 x 2048 points, two views, size 128, radius 4: the sheet's shape, its
    prediction panels against render_balls(camera(pc), palette[pred - start]) called by hand, ground-truth panels that are not
    blank, the error row's colours, and the training flag restored"""
    from ppt_amd import viz, weights as W
    from ppt_amd.models import ULIP_models as M
    args = SimpleNamespace(classnames=M.dataset_classnames("shapenetpart"), template_init='', class_name_position='middle',
                           num_learnable_prompt_tokens=32, gpu=0, task='partseg', head_type=0, evaluate_3d=False, ulip2=False,
                           synthetic_weights=True)
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.ULIP_PointBERT_partseg(args)
    m.load_state_dict(W.ulip_partseg_state_dict(seed=0), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding(50, seed=0)
    m.cuda().train()
    pc, _ = W.synth_clouds(2, 2048, seed=55)
    pc = torch.from_numpy(pc).cuda()
    g = torch.Generator().manual_seed(5)
    cls = torch.tensor([[10], [1]])                                            # Motorbike (6 parts), Bag (2)
    part = torch.stack([torch.randint(30, 36, (2048,), generator=g), torch.randint(4, 6, (2048,), generator=g)]).cuda()
    views = viz.views_from_mouse([(0.5, 0.5), (0.3, 0.7)])
    size, radius, V = 128, 4, 2
    model = _Recording(m)
    model.train()
    sheet = viz.partseg_sheet(model, pc, cls, part, R.CATEGORY2PART, views=views, size=size, radius=radius)
    assert model.training and len(model.seen) == 1
    assert sheet.shape == (2, 3 * size, V * size, 3) and sheet.dtype == torch.uint8 and sheet.is_cuda
    logits = model.seen[0].float()
    assert logits.shape == (2, 2048, 50)
    pred = viz.predict_parts(logits, part, R.CATEGORY2PART)
    assert np.array_equal(pred.cpu().numpy(), R.predict_parts(logits.cpu().numpy(), part[:, 0].cpu().numpy()))
    pal = viz.palette_tensor(device="cuda")
    start = torch.tensor([30, 4], device="cuda")
    ixyz = viz.camera(pc, views, size)
    by_hand = viz.render_balls(ixyz, pal[(pred.long() - start.view(-1, 1))][:, None].expand(2, V, 2048, 3), size, radius=radius)
    truth = viz.render_balls(ixyz, pal[(part - start.view(-1, 1))][:, None].expand(2, V, 2048, 3), size, radius=radius)
    white = torch.tensor([255, 255, 255], dtype=torch.uint8, device="cuda")
    for b in range(2):
        for v in range(V):
            cols = slice(v * size, (v + 1) * size)
            assert torch.equal(sheet[b, size:2 * size, cols], by_hand[b, v]), (b, v)
            assert torch.equal(sheet[b, :size, cols], truth[b, v]), (b, v)
            covered = (sheet[b, :size, cols] != white).any(-1).float().mean().item()
            assert 0.05 < covered < 0.95, covered                              # a picture, neither blank nor full
            # the three rows share one visibility
            for row in (1, 2):
                assert torch.equal((sheet[b, row * size:(row + 1) * size, cols] != white).any(-1), (sheet[b, :size, cols] != white).any(-1))
    # the device camera is the numpy camera (outside the 1e-9 band around integers)
    want, values = R.camera(pc.cpu().numpy(), views, size)
    assert not ((ixyz.cpu().numpy() != want) & ~R.in_band(values)).any()
    # two rows only without the error map (a second forward: its own logits, e.g. other random FPS starts; the same ground truth)
    two = viz.partseg_sheet(model, pc, cls, part, R.CATEGORY2PART, views=views, size=size, radius=radius, error_map=False)
    assert two.shape == (2, 2 * size, V * size, 3) and torch.equal(two[:, :size], sheet[:, :size])
    pred2 = viz.predict_parts(model.seen[1].float(), part, R.CATEGORY2PART)
    by_hand = viz.render_balls(ixyz, pal[(pred2.long() - start.view(-1, 1))][:, None].expand(2, V, 2048, 3), size, radius=radius)
    assert torch.equal(two[:, size:], by_hand.permute(0, 2, 1, 3, 4).reshape(2, size, V * size, 3))
