"""GPU: the device augmentations (csrc/cloud_augment.hip, ppt_amd/data/augment.py, the loader's "shapenet55" recipe and `augment=`)
against what the reference's functions produced (tests/golden/g_augment.npz, made by tests/golden/make_golden_augment.py) and against
the numpy / Python restatement of the kernels (tests/augment_ref.py).

Dropout, scale, shift, jitter, affine and the height column are compared bit for bit.  A rotation is np.dot(pc, R) in the reference: a
BLAS dgemm whose summation may fuse or reorder, so its float64 result can differ in the last bit before the float32 rounding.  Against
the FIXTURE a rotated cloud therefore has to satisfy `rotate_ok`: |delta| <= one float32 ulp of the row's largest coordinate magnitude
and >= 99.9 % of the elements bit-equal (while generating the fixture every rotated element it checks, 24 720 in all, was bit-equal to
the stated order).  Against the RESTATEMENT the kernel is always compared bit for bit."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_ref as A
from ppt_amd import weights as W
from ppt_amd.data import augment as AUG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (3, 64, 257, 512)
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def g():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g_augment.npz")))


@pytest.fixture(scope="module")
def gd():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g_datapipe.npz")))


@pytest.fixture(scope="module")
def ops():
    from ppt_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(dtype) if dtype is not None else t


def host(t):
    return t.cpu().numpy()


def rotate_ok(got, want):
    """[..., n, 3] clouds; the criterion of the module text"""
    bound = A.ulp32(np.abs(want).max(axis=-1, keepdims=True))
    close = np.abs(got.astype(np.float64) - want.astype(np.float64)) <= bound
    return bool(close.all() and (got == want).mean() >= 0.999)


def fixture_case(g, n):
    c = {k: g[f"c{n}_{k}"] for k in ("norm", "drop", "scale", "shift", "pert", "rot", "height")}
    d = {k: g[f"c{n}_d_{k}"] for k in ("ratio", "u", "scale", "shift", "perturb", "rotate")}
    d["mask"] = (d["u"] <= d["ratio"][:, None]).astype(np.uint8)
    return c, d


# ------------------------------------------------------------------ 1. the kernel, stage by stage
@pytest.mark.parametrize("n", NS)
def test_each_stage_and_the_chain_against_the_fixture(g, ops, n):
    c, d = fixture_case(g, n)
    t = {k: dev(v) for k, v in d.items()}
    norm = dev(c["norm"])
    before = norm.clone()
    assert np.array_equal(host(ops.cloud_augment(norm, [("dropout", t["mask"])])), c["drop"])
    assert torch.equal(norm, before)                                            # a new tensor: the input is not written
    assert np.array_equal(host(ops.cloud_augment(dev(c["drop"]), [("scale", t["scale"])])), c["scale"])
    assert np.array_equal(host(ops.cloud_augment(dev(c["scale"]), [("shift", t["shift"])])), c["shift"])
    for src, R, dst in (("shift", "perturb", "pert"), ("pert", "rotate", "rot")):
        got = host(ops.cloud_augment(dev(c[src]), [("rotate", t[R])]))
        assert rotate_ok(got, c[dst]), (src, (got == c[dst]).mean())
        assert np.array_equal(got, np.stack([A.rotate(p, r) for p, r in zip(c[src], d[R])]))
    want4 = np.concatenate([c["rot"], c["height"][:, :, None]], axis=2)
    assert np.array_equal(host(ops.cloud_augment(dev(c["rot"]), [], height=True)), want4)
    assert np.array_equal(host(ops.cloud_augment(dev(c["rot"]), [("height",)])), want4)
    assert np.array_equal(host(ops.cloud_height(dev(c["rot"]))), want4)          # and the separate launch agrees
    stages = [("dropout", t["mask"]), ("scale", t["scale"]), ("shift", t["shift"]), ("rotate", t["perturb"]), ("rotate", t["rotate"])]
    got = host(ops.cloud_augment(norm, stages))
    got4 = host(ops.cloud_augment(norm, stages, height=True))
    assert rotate_ok(got, c["rot"]) and np.array_equal(got4[:, :, :3], got)
    for i in range(len(got)):
        one = [("dropout", d["mask"][i]), ("scale", d["scale"][i]), ("shift", d["shift"][i]), ("rotate", d["perturb"][i]),
               ("rotate", d["rotate"][i])]
        assert np.array_equal(got4[i], A.chain(c["norm"][i], one, with_height=True))


def test_jitter_and_affine_are_bit_exact(g, gd, ops):
    x = g["c64_norm"][:2]
    got = ops.cloud_augment(dev(x), [("jitter", dev(g["jit_noise"]))])
    assert got.dtype == torch.float32 and np.array_equal(host(got), g["jit_out"].astype(np.float32))
    # translate_pointcloud as a stage: what ppt_cloud_prep_f32 makes of the same normalised clouds (g_datapipe.npz)
    got = ops.cloud_augment(dev(gd["mn_train_norm"]), [("affine", dev(gd["mn_train_scale"]), dev(gd["mn_train_shift"]))])
    assert np.array_equal(host(got), gd["mn_train_trans"])


def test_every_stage_at_8192_rows(gd, ops):
    """one 8192-row cloud (96 KB of LDS, the opt-in) through all seven kinds -- the full list of 8 stages -- against the restatement"""
    p = np.ascontiguousarray(gd["big"][:1])
    n = p.shape[1]
    rs = np.random.RandomState(7)
    d = {}
    for st in AUG.STAGES:
        d.update(AUG.host_stage_draws(rs, st, 1, n))
    sc, sh = rs.uniform(2. / 3., 3. / 2., (1, 3)), rs.uniform(-0.2, 0.2, (1, 3))
    names = (("dropout", "mask"), ("scale", "scale"), ("shift", "shift"), ("rotate", "perturb"), ("jitter", "noise"), ("rotate", "rotate"))
    stages = [(k, dev(d[v])) for k, v in names] + [("affine", dev(sc), dev(sh))]
    got = host(ops.cloud_augment(dev(p), stages, height=True))
    one = [(k, d[v][0]) for k, v in names] + [("affine", sc[0], sh[0])]
    assert d["mask"].sum() > 0 and np.array_equal(got[0], A.chain(p[0], one, with_height=True))


def test_edge_masks(g, ops):
    c, _ = fixture_case(g, 257)
    p = c["norm"][:3]
    masks = np.zeros((3, 257), np.uint8)
    masks[0] = 1                                                                # all rows dropped: every row is row 0
    masks[2, 0] = 1                                                             # only row 0: it takes itself
    got = host(ops.cloud_augment(dev(p), [("dropout", dev(masks))]))
    assert np.array_equal(got[0], np.tile(p[0, :1], (257, 1))) and np.array_equal(got[1], p[1]) and np.array_equal(got[2], p[2])
    masks[1] = 255                                                              # any non-zero byte is "set"
    masks[1, 5] = 0
    got = host(ops.cloud_augment(dev(p), [("dropout", dev(masks))]))
    assert np.array_equal(got[1], A.dropout(p[1], masks[1]))


def test_reference_named_functions(g, gd):
    """ppt_amd.data's six functions with rs=: sample 0 of the n = 257 chain, function after function on the reference's generator"""
    from ppt_amd import data as PD
    c, _ = fixture_case(g, 257)
    rs = np.random.RandomState([int(g["seed"]), 0, 0])
    assert rs.randint(0, gd["small"].shape[1]) == g["c257_d_start"][0]           # the FPS start comes first
    x = dev(c["norm"][:1])
    x = PD.random_point_dropout(x, rs=rs); assert np.array_equal(host(x), c["drop"][:1])
    x = PD.random_scale_point_cloud(x, rs=rs); assert np.array_equal(host(x), c["scale"][:1])
    x = PD.shift_point_cloud(x, rs=rs); assert np.array_equal(host(x), c["shift"][:1])
    x = PD.rotate_perturbation_point_cloud(x, rs=rs); assert rotate_ok(host(x), c["pert"][:1])
    x = PD.rotate_point_cloud(x, rs=rs); assert rotate_ok(host(x), c["rot"][:1])
    jit = PD.jitter_point_cloud(dev(g["c64_norm"][:2]), rs=np.random.RandomState([int(g["seed"]), 1, 0]))
    assert jit.dtype == torch.float32 and np.array_equal(host(jit), g["jit_out"].astype(np.float32))
    # seed=: the device's draws for the named samples, whatever the batch
    idx = np.array([5, 77, 123456], dtype=np.int64)
    pc = dev(c["norm"][:3])
    a = host(PD.rotate_point_cloud(pc, seed=9, epoch=2, index=dev(idx)))
    b = host(PD.rotate_point_cloud(pc[1:2], seed=9, epoch=2, index=dev(idx[1:2])))
    assert np.array_equal(a[1:2], b)
    from ppt_amd import ops
    R = host(ops.cloud_draws_aug(dev(idx), 257, 9, 2, rotate=True)["rotate"])     # (pinned to the counter function further down)
    assert all(np.array_equal(a[i], A.rotate(c["norm"][i], R[i])) for i in range(3))


# ------------------------------------------------------------------ 2. the loader
def _collect(ld):
    batches = list(ld)
    assert len(batches) == len(ld)
    return [torch.cat([b[k] for b in batches]) for k in range(len(batches[0]))]


@pytest.mark.parametrize("batch", [4, 3])
def test_loader_numpy_draws_reproduce_the_reference(g, gd, batch):
    from ppt_amd.data import DeviceBatchLoader, DeviceCloudSet
    seed, labels = int(g["seed"]), np.array([3, 9, 27, 11])
    s = DeviceCloudSet(gd["small"], labels)
    c, _ = fixture_case(g, 257)
    pc, target = _collect(DeviceBatchLoader(s, batch, 257, "shapenet55", True, shuffle=False, seed=seed, draws="numpy"))
    assert pc.dtype == torch.float32 and tuple(pc.shape) == (4, 257, 3) and host(target).tolist() == labels.tolist()
    assert rotate_ok(host(pc), c["rot"])
    pc4, _ = _collect(DeviceBatchLoader(s, batch, 257, "shapenet55", True, shuffle=False, seed=seed, draws="numpy", use_height=True))
    assert tuple(pc4.shape) == (4, 257, 4) and np.array_equal(host(pc4)[:, :, :3], host(pc))
    assert np.array_equal(host(pc4), np.stack([A.height(p) for p in host(pc)]))
    if np.array_equal(host(pc), c["rot"]):                                      # (always, unless a rotation met its one-ulp case)
        assert np.array_equal(host(pc4)[:, :, 3], c["height"])
    # the test split: the normalised sample, no augmentation
    pc, _ = _collect(DeviceBatchLoader(s, batch, 257, "shapenet55", False, shuffle=False, seed=seed, draws="numpy"))
    rs = np.random.RandomState([seed, 0, 0])
    from oracle import oracle as O
    from ppt_amd.data import pc_normalize
    for i in range(4):
        rows, _ = O.dataset_farthest_point_sample(gd["small"][i], 257, rs.randint(0, 2048))
        assert np.array_equal(host(pc[i]), pc_normalize(rows[:, :3]))
    # clouds of exactly npoints rows: random_sample's persistent permutation
    s64 = DeviceCloudSet(np.ascontiguousarray(gd["small"][:, :64]), labels)
    pc, _ = _collect(DeviceBatchLoader(s64, batch, 64, "shapenet55", True, shuffle=False, seed=seed, draws="numpy"))
    assert rotate_ok(host(pc), g["rs_final"])
    # an augment list on an old recipe: the recipe's own draws, then the stages' draws, sample after sample
    pc, _ = _collect(DeviceBatchLoader(s, batch, 512, "scanobjectnn", True, shuffle=False, seed=seed, draws="numpy",
                                       augment=("rotate", "jitter")))
    assert rotate_ok(host(pc), g["so_aug_final"])


@pytest.mark.parametrize("recipe", ["modelnet", "scanobjectnn", "shapenetpart"])
def test_augment_none_is_todays_batch(gd, ops, recipe):
    """augment=None: byte-identical to ops.cloud_draws + ops.fps + ops.cloud_prep called as the loader called them before"""
    from ppt_amd.data import DeviceBatchLoader, DeviceCloudSet
    part = recipe == "shapenetpart"
    s = DeviceCloudSet(gd["small"], np.arange(4), seg=gd["seg"] if part else None)
    n, seed = 512, 17
    for kw in ({}, {"augment": None}, {"augment": ()}):
        got = next(iter(DeviceBatchLoader(s, 4, n, recipe, True, shuffle=False, seed=seed, **kw)))
        item = dev(np.arange(4, dtype=np.int64))
        fps = recipe == "modelnet"
        d = ops.cloud_draws(item, n, seed, 0, rows=None, rows_all=2048, start=fps, affine=not part, perm=not part, sel=part)
        sel = d.get("sel")
        if fps:
            sel, _ = ops.fps(s.points, n, d["start"])
        want = ops.cloud_prep(s.points, item, n, sel=sel, lengths=None, normalize=fps, scale=d.get("scale"), shift=d.get("shift"),
                              perm=d.get("perm"), seg_src=s.seg if part else None)
        if part:
            assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[1])
        else:
            assert torch.equal(got[0], want)


# ------------------------------------------------------------------ 3. device draws
def _within_ulps(got, want, k):
    return bool((np.abs(got - want) <= k * np.spacing(np.abs(want))).all())


def test_device_draws_are_the_documented_function_of_the_counter(ops):
    """ppt_cloud_draws_aug equals the Python statement (tests/augment_ref.py): exactly where only Philox words, integer-to-double
    conversions and single multiply-adds are involved; within 4 ulp where log / sqrt / sin / cos take part (the angles and the
    noise, relative to the value; the matrices' entries, sums of products of sines and cosines that cancel, relative to 1)."""
    seed, n = 0x1234567887654321, 37
    pairs = [(0, 0), (7, 3), (123456, 3), (2 ** 31 + 5, 1)]
    for epoch in sorted({e for _, e in pairs}):
        index = np.array([i for i, e in pairs if e == epoch], dtype=np.int64)
        d = ops.cloud_draws_aug(dev(index), n, seed, epoch, dropout=True, scale=True, shift=True, rotate_perturbation=True, rotate=True,
                                jitter=True)
        again = ops.cloud_draws_aug(dev(index), n, seed, epoch, dropout=True, scale=True, shift=True, rotate_perturbation=True,
                                    rotate=True, jitter=True)
        assert all(torch.equal(d[k], again[k]) for k in d)
        d = {k: host(v) for k, v in d.items()}
        assert d["mask"].dtype == np.uint8 and d["noise"].shape == (len(index), n, 3)
        for b, ix in enumerate(index.tolist()):
            w = A.device_draws(ix, epoch, seed, n)
            for k in ("ratio", "scale", "angle"):
                assert d[k][b] == w[k], (k, ix)
            assert np.array_equal(d["mask"][b], w["mask"]) and np.array_equal(d["shift"][b], w["shift"])
            assert _within_ulps(d["angles"][b], w["angles"], 4) and _within_ulps(d["noise"][b], w["noise"], 4)
            assert np.abs(d["perturb"][b] - w["perturb"]).max() <= 4 * EPS and np.abs(d["rotate"][b] - w["rotate"]).max() <= 4 * EPS
    # other magnitudes: the same uniforms and normals, scaled and clipped by the given values
    d2 = ops.cloud_draws_aug(dev(np.array([7], dtype=np.int64)), n, seed, 3, dropout=True, scale=True, shift=True, jitter=True,
                             max_dropout=0.5, scale_low=0.9, scale_high=1.1, shift_range=0.3, jitter_sigma=0.02, jitter_clip=0.03)
    w = A.device_draws(7, 3, seed, n, max_dropout=0.5, scale_low=0.9, scale_high=1.1, shift_range=0.3, jitter_sigma=0.02, jitter_clip=0.03)
    assert host(d2["ratio"])[0] == w["ratio"] and host(d2["scale"])[0] == w["scale"] and np.array_equal(host(d2["shift"])[0], w["shift"])
    assert _within_ulps(host(d2["noise"])[0], w["noise"], 4) and np.abs(host(d2["noise"])).max() <= 0.03
    assert (np.abs(w["noise"]) == 0.03).any()                                   # (1.5 sigma: the clip is exercised)


def test_device_draws_ranges_and_moments(ops):
    """Ranges, orthogonality, and sample moments within 5 standard errors of their expectations (fixed seed: deterministic)."""
    B, n = 256, 128
    d = ops.cloud_draws_aug(dev(np.arange(B, dtype=np.int64) * 131), n, 2024, 1, dropout=True, scale=True, shift=True,
                            rotate_perturbation=True, rotate=True, jitter=True)
    d = {k: host(v) for k, v in d.items()}
    assert d["scale"].min() >= 0.8 and d["scale"].max() < 1.25 and np.abs(d["shift"]).max() <= 0.1
    assert np.abs(d["angles"]).max() <= 0.18 and np.abs(d["noise"]).max() <= 0.05
    assert d["ratio"].min() >= 0 and d["ratio"].max() < 0.875 and d["angle"].min() >= 0 and d["angle"].max() <= 2 * np.pi
    assert set(np.unique(d["mask"])) <= {0, 1}
    for R in (d["perturb"], d["rotate"]):
        assert np.abs(np.einsum("bji,bjk->bik", R, R) - np.eye(3)).max() <= 8 * EPS
        assert np.allclose(np.linalg.det(R), 1.0, atol=1e-14)
    # uniform on [a, b): sd (b - a) / sqrt(12)
    for k, a, b in (("scale", 0.8, 1.25), ("shift", -0.1, 0.1), ("ratio", 0.0, 0.875), ("angle", 0.0, 2 * np.pi)):
        v = d[k].reshape(-1)
        assert abs(v.mean() - (a + b) / 2) < 5 * (b - a) / np.sqrt(12 * v.size), k
    # the noise is 0.01 z clipped at 5 sigma (P(|z| > 5) = 6e-7: the clip moves E z^2 by ~2e-5, far inside the bound):
    # mean of z: sd 1 / sqrt(N); mean of z^2: sd sqrt(2 / N); the two Box-Muller outputs alternate over the elements
    z = d["noise"].reshape(-1) / 0.01
    N = z.size
    assert N == 98304 and abs(z.mean()) < 5 / np.sqrt(N) and abs((z ** 2).mean() - 1) < 5 * np.sqrt(2 / N)
    assert abs(z[0::2].mean()) < 5 / np.sqrt(N / 2) and abs(z[1::2].mean()) < 5 / np.sqrt(N / 2)
    assert abs((z[0::2] * z[1::2]).mean()) < 5 / np.sqrt(N / 2)                 # the pair is uncorrelated
    # the angles are 0.06 z clipped at 3 sigma: symmetric, so the mean stays 0 and the sd is at most 0.06
    a = d["angles"].reshape(-1)
    assert abs(a.mean()) < 5 * 0.06 / np.sqrt(a.size)
    # given its ratio a row is dropped with probability ratio: the count is a sum of Bernoullis
    expect, var = (n * d["ratio"]).sum(), (n * d["ratio"] * (1 - d["ratio"])).sum()
    assert abs(d["mask"].sum() - expect) < 5 * np.sqrt(var)


def _by_index(loader, epoch=0):
    loader.set_epoch(epoch)
    out, order, k = {}, loader.indices(), 0
    for batch in loader:
        for row in host(batch[0]):
            out.setdefault(int(order[k]), row)
            k += 1
    assert k == len(order)
    return out


@pytest.mark.parametrize("recipe,npoints,augment", [("shapenet55", 33, None), ("shapenet55", 96, ("jitter",)), ("modelnet", 33, AUG.STAGES)])
def test_device_draws_do_not_depend_on_batching(recipe, npoints, augment):
    from ppt_amd.data import DeviceBatchLoader, DeviceCloudSet
    r = np.random.default_rng(2)
    m, rows = 30, 96
    s = DeviceCloudSet(r.standard_normal((m, rows, 3)).astype(np.float32), np.arange(m) % 7)

    def mk(bs, world=1, rank=0, seed=5):
        return DeviceBatchLoader(s, bs, npoints, recipe, True, seed=seed, world_size=world, rank=rank, augment=augment, use_height=True)
    a = _by_index(mk(8))
    assert sorted(a) == list(range(m)) and a[0].shape == (npoints, 4) and all(np.isfinite(v).all() for v in a.values())
    for other in (_by_index(mk(8)), _by_index(mk(7))):                # the same seed again; another batch size
        assert all(np.array_equal(a[i], other[i]) for i in range(m))
    halves = {**_by_index(mk(8, 2, 0)), **_by_index(mk(8, 2, 1))}     # two ranks
    assert sorted(halves) == list(range(m)) and all(np.array_equal(a[i], halves[i]) for i in range(m))
    nxt = _by_index(mk(8), epoch=1)
    assert not any(np.array_equal(a[i], nxt[i]) for i in range(m))    # another epoch, other draws
    other_seed = _by_index(mk(8, seed=6))
    assert not any(np.array_equal(a[i], other_seed[i]) for i in range(m))


def test_loader_device_draws_are_the_stated_chain(ops):
    """a "shapenet55" device-draw batch (clouds of exactly npoints rows: the Philox permutation selects) is the restatement's chain
    on the sample's draws, bit for bit; the draws themselves are pinned to the counter function above"""
    from ppt_amd.data import DeviceBatchLoader, DeviceCloudSet, pc_normalize
    r = np.random.default_rng(4)
    m, n = 5, 40
    clouds = r.standard_normal((m, n, 3)).astype(np.float32) + np.float32(0.5)
    ld = DeviceBatchLoader(DeviceCloudSet(clouds, np.arange(m)), 5, n, "shapenet55", True, shuffle=False, seed=77, use_height=True)
    ld.set_epoch(2)
    pc, _ = next(iter(ld))
    item = dev(np.arange(m, dtype=np.int64))
    perm = host(ops.cloud_draws(item, n, 77, 2, perm=True)["perm"])
    d = {k: host(v) for k, v in ops.cloud_draws_aug(item, n, 77, 2, **{st: True for st in AUG.SHAPENET_CHAIN}).items()}
    for i in range(m):
        w = A.device_draws(i, 2, 77, n)
        assert np.array_equal(d["mask"][i], w["mask"]) and d["scale"][i] == w["scale"] and np.array_equal(d["shift"][i], w["shift"])
        stages = [("dropout", w["mask"]), ("scale", w["scale"]), ("shift", w["shift"]), ("rotate", d["perturb"][i]), ("rotate", d["rotate"][i])]
        assert np.array_equal(host(pc[i]), A.chain(pc_normalize(clouds[i][perm[i]]), stages, with_height=True))


# ------------------------------------------------------------------ 4. a training step
def test_trainer_steps_from_a_shapenet55_loader():
    import contextlib
    import io
    from ppt_amd.data import DeviceBatchLoader, DeviceCloudSet
    from ppt_amd.models import ULIP_models as M
    from ppt_amd.train import Trainer
    names = M.dataset_classnames("modelnet40")
    args = SimpleNamespace(classnames=names, template_init='', class_name_position='middle', num_learnable_prompt_tokens=32, gpu=0,
                           task='cls', head_type=0, evaluate_3d=False, ulip2=False, synthetic_weights=True)
    with contextlib.redirect_stdout(io.StringIO()):
        m = M.ULIP_PointBERT(args)
    m.load_state_dict(W.ulip_pointbert_state_dict(seed=0), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding_from_tokens(m.tokenized_prompts, seed=0)
    m.cuda().set_precision("mixed16")
    m.train()
    tr = Trainer(m, lr=3e-3, label_smoothing=0.2, distributed=False)
    pc, _ = W.synth_clouds(32, 2048, seed=5)
    s = DeviceCloudSet(pc, np.arange(32) % len(names))
    losses = []
    for pcb, target in DeviceBatchLoader(s, 32, 1024, "shapenet55", True, seed=1):
        assert pcb._ppt_ready is not None and tuple(pcb.shape) == (32, 1024, 3)
        loss, _ = tr.step(pcb, target)
        losses.append(loss)
    tr.finish()
    torch.cuda.synchronize()
    assert len(losses) == 1 and np.isfinite(float(losses[0].detach())), losses
