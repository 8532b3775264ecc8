"""CPU: the host side of the device augmentations (ppt_amd/data/augment.py, the loader's "shapenet55" recipe and `augment=`) -- draw
order and generator state, the kernel-order restatement (tests/augment_ref.py) against what the reference produced
(tests/golden/g_augment.npz), validation, and the two C entry points' argument checks."""
import ctypes
import os

import numpy as np
import pytest

import augment_ref as A
from ppt_amd import data as PD
from ppt_amd.data import augment as AUG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (3, 64, 257, 512)


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g_augment.npz")))


@pytest.fixture(scope="module")
def small():
    return np.load(os.path.join(ROOT, "tests", "golden", "g_datapipe.npz"))["small"]


def test_fixture_was_made_with_numpy_2(g):
    assert int(str(g["numpy"]).split(".")[0]) >= 2


def _expected_aug(b, stage, n):
    """the reference function's own statements for pc[None] (data/dataset_3d.py), on the generator `b`"""
    if stage == "dropout":
        ratio = b.random_sample() * 0.875
        u = b.random_sample((n,))
        return {"aug_ratio": ratio, "aug_u": u, "aug_mask": (u <= ratio).astype(np.uint8)}
    if stage == "scale":
        return {"aug_scale": b.uniform(0.8, 1.25, 1)[0]}
    if stage == "shift":
        return {"aug_shift": b.uniform(-0.1, 0.1, (1, 3))[0]}
    if stage == "rotate_perturbation":
        angles = np.clip(0.06 * b.randn(3), -0.18, 0.18)
        return {"aug_angles": angles, "aug_perturb": AUG.perturbation_matrix(angles)}
    if stage == "rotate":
        angle = b.uniform() * 2 * np.pi
        return {"aug_angle": angle, "aug_rotate": AUG.up_axis_matrix(angle)}
    return {"aug_noise": np.clip(0.01 * b.randn(1, n, 3), -0.05, 0.05)[0]}


def test_numpy_draw_order_and_generator_state():
    n = 48
    cases = [("shapenet55", True, 200, ()), ("shapenet55", False, 200, ()), ("shapenet55", True, n, ()), ("shapenet55", True, 200, ("jitter",)),
             ("modelnet", True, 200, ("rotate", "jitter")), ("scanobjectnn", False, 200, ("jitter", "dropout", "scale")),
             ("shapenetpart", True, 131, ("shift", "rotate_perturbation"))]
    for recipe, train, rows, augment in cases:
        a, b = np.random.RandomState(99), np.random.RandomState(99)
        perm_a, perm_b = np.arange(n), np.arange(n)
        d = PD.numpy_draws(a, recipe, train, rows, n, augment, perm_a)
        want = {}
        stages = tuple(augment)
        if recipe == "shapenetpart":
            want["sel"] = b.choice(rows, n, replace=True)
        elif recipe == "shapenet55":
            if n < rows:
                want["start"] = b.randint(0, rows)
            else:
                b.shuffle(perm_b)
                want["sel"] = perm_b[:n]
            if train:
                stages = ("dropout", "scale", "shift", "rotate_perturbation", "rotate") + stages
        else:
            if recipe == "modelnet" and rows > n:
                want["start"] = b.randint(0, rows)
            if train:
                want["scale"], want["shift"], want["perm"] = b.uniform(2. / 3., 3. / 2., 3), b.uniform(-0.2, 0.2, 3), b.permutation(n)
        for st in stages:
            want.update(_expected_aug(b, st, n))
        assert sorted(d) == sorted(want), (recipe, train, rows, augment)
        for k in want:
            assert np.array_equal(d[k], want[k]), (recipe, k)
        assert a.randint(0, 1 << 30) == b.randint(0, 1 << 30) and np.array_equal(perm_a, perm_b)
    # the persistent permutation is shuffled cumulatively: the second sample's rows are a shuffle of the first's order
    a, perm = np.random.RandomState(3), np.arange(n)
    first = PD.numpy_draws(a, "shapenet55", False, n, n, permutation=perm)["sel"]
    b = np.random.RandomState(3)
    mine = np.arange(n)
    b.shuffle(mine)
    assert np.array_equal(first, mine)
    second = PD.numpy_draws(a, "shapenet55", False, n, n, permutation=perm)["sel"]
    b.shuffle(mine)
    assert np.array_equal(second, mine) and not np.array_equal(first, second)


@pytest.mark.parametrize("n", NS)
def test_replay_reproduces_the_fixture_draws_and_state(g, small, n):
    """numpy_draws on RandomState([seed, 0, 0]) gives the draws the reference made, and ends where the reference's generator did"""
    rs = np.random.RandomState([int(g["seed"]), 0, 0])
    count = g[f"c{n}_norm"].shape[0]
    for i in range(count):
        d = PD.numpy_draws(rs, "shapenet55", True, small.shape[1], n)
        assert d["start"] == g[f"c{n}_d_start"][i]
        for k in ("ratio", "u", "scale", "shift", "angles", "perturb", "angle", "rotate"):
            assert np.array_equal(d["aug_" + k], g[f"c{n}_d_{k}"][i]), (k, i)
    assert rs.randint(0, 1 << 30) == int(g[f"c{n}_probe"])


def _rotate_ok(got, want):
    """the rotation's criterion: np.dot's dgemm may sum in another order, so |delta| <= one float32 ulp of the row's largest
    coordinate magnitude, and >= 99.9 % of the elements bit-equal"""
    bound = A.ulp32(np.abs(want).max(axis=1, keepdims=True))
    return bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= bound).all() and (got == want).mean() >= 0.999)


@pytest.mark.parametrize("n", NS)
def test_restatement_reproduces_the_reference(g, n):
    """every stage of tests/augment_ref.py, fed the REFERENCE's input and draws, gives the reference's output"""
    for i in range(g[f"c{n}_norm"].shape[0]):
        c = {k: g[f"c{n}_{k}"][i] for k in ("norm", "drop", "scale", "shift", "pert", "rot", "height")}
        d = {k: g[f"c{n}_d_{k}"][i] for k in ("ratio", "u", "scale", "shift", "perturb", "rotate")}
        assert all(v.dtype == np.float32 for v in c.values()) and all(v.dtype == np.float64 for v in d.values())
        assert np.array_equal(A.dropout(c["norm"], d["u"] <= d["ratio"]), c["drop"])
        assert np.array_equal(A.scale(c["drop"], d["scale"]), c["scale"])
        assert np.array_equal(A.shift(c["scale"], d["shift"]), c["shift"])
        assert _rotate_ok(A.rotate(c["shift"], d["perturb"]), c["pert"])
        assert _rotate_ok(A.rotate(c["pert"], d["rotate"]), c["rot"])
        assert np.array_equal(A.height(c["rot"])[:, 3], c["height"])
        stages = [("dropout", d["u"] <= d["ratio"]), ("scale", d["scale"]), ("shift", d["shift"]), ("rotate", d["perturb"]),
                  ("rotate", d["rotate"])]
        assert _rotate_ok(A.chain(c["norm"], stages), c["rot"])


def test_jitter_restatement_is_the_float32_of_the_reference(g):
    x = g["c64_norm"][:2]
    for b in range(2):
        assert np.array_equal(A.jitter(x[b], g["jit_noise"][b]), g["jit_out"][b].astype(np.float32))
    assert g["jit_out"].dtype == np.float64 and np.abs(g["jit_noise"]).max() <= 0.05


def test_python_device_draws_are_in_range():
    """the Python statement of the counter function (what the GPU test compares the kernel with) keeps its own promises"""
    d = A.device_draws(12345, 2, 0x1234567887654321, 37)
    assert 0 <= d["ratio"] < 0.875 and 0.8 <= d["scale"] < 1.25 and np.abs(d["shift"]).max() <= 0.1
    assert np.abs(d["angles"]).max() <= 0.18 and np.abs(d["noise"]).max() <= 0.05 and 0 <= d["angle"] < 2 * np.pi
    for R in (d["perturb"], d["rotate"]):
        assert np.abs(R.T @ R - np.eye(3)).max() < 8 * np.finfo(np.float64).eps
    assert d["u"].shape == (37,) and d["noise"].shape == (37, 3) and d["mask"].dtype == np.uint8
    assert np.array_equal(A.device_draws(12345, 2, 0x1234567887654321, 64)["u"][:37], d["u"])      # the counter, not n, decides a row


def _cpu_set(m=9, n=64):
    r = np.random.default_rng(0)
    return PD.DeviceCloudSet(r.standard_normal((m, n, 3)).astype(np.float32), np.arange(m) % 5,
                             seg=r.integers(0, 4, (m, n)).astype(np.int32), device="cpu")


def test_loader_validation_and_plan():
    s = _cpu_set()
    with pytest.raises(ValueError, match="recipe"):
        PD.DeviceBatchLoader(s, 4, 32, "shapenet", True)                       # still not a recipe: the new one is "shapenet55"
    with pytest.raises(ValueError, match="unknown stage"):
        PD.DeviceBatchLoader(s, 4, 32, "modelnet", True, augment=("rotate", "flip"))
    with pytest.raises(ValueError, match="unknown stage"):
        PD.DeviceBatchLoader(s, 4, 32, "modelnet", True, augment=("height",))  # the height column is use_height, not a stage name
    with pytest.raises(ValueError, match="once"):
        PD.DeviceBatchLoader(s, 4, 32, "modelnet", True, augment=("jitter", "jitter"))
    with pytest.raises(ValueError, match="once"):
        PD.DeviceBatchLoader(s, 4, 32, "shapenet55", True, augment=("rotate",))      # ShapeNet's own chain already rotates
    PD.DeviceBatchLoader(s, 4, 32, "shapenet55", False, augment=("rotate",))
    with pytest.raises(ValueError, match="one row count"):
        PD.DeviceBatchLoader(PD.DeviceCloudSet(np.zeros((2, 64, 3), np.float32), [0, 1], lengths=[64, 50], device="cpu"), 2, 32,
                             "shapenet55", True)
    # augment=None: the launches of a batch are today's, for every old recipe and both splits
    today = {("modelnet", True): ("cloud_draws", "fps", "cloud_prep"), ("modelnet", False): ("cloud_draws", "fps", "cloud_prep"),
             ("scanobjectnn", True): ("cloud_draws", "cloud_prep"), ("scanobjectnn", False): ("cloud_prep",),
             ("shapenetpart", True): ("cloud_draws", "cloud_prep"), ("shapenetpart", False): ("cloud_draws", "cloud_prep")}
    for (recipe, train), want in today.items():
        for kw in ({}, {"augment": None}, {"augment": ()}):
            ld = PD.DeviceBatchLoader(s, 4, 32, recipe, train, **kw)
            assert ld.plan() == want and ld._aug_stages == (), (recipe, train, kw)
        assert PD.DeviceBatchLoader(s, 4, 32, recipe, train, use_height=True).plan() == want + ("cloud_height",)
        assert PD.DeviceBatchLoader(s, 4, 32, recipe, train, draws="numpy").plan() == tuple(x for x in want if x != "cloud_draws")
    # with augmentations: one draw launch and one augment launch more, and no separate height launch
    ld = PD.DeviceBatchLoader(s, 4, 32, "modelnet", True, augment=("rotate", "jitter"), use_height=True)
    assert ld.plan() == ("cloud_draws", "cloud_draws_aug", "fps", "cloud_prep", "cloud_augment") and ld._aug_stages == ("rotate", "jitter")
    ld = PD.DeviceBatchLoader(s, 4, 32, "shapenet55", True)
    assert ld.plan() == ("cloud_draws", "cloud_draws_aug", "fps", "cloud_prep", "cloud_augment")
    assert ld._aug_stages == ("dropout", "scale", "shift", "rotate_perturbation", "rotate")
    assert PD.DeviceBatchLoader(s, 4, 64, "shapenet55", True).plan() == ("cloud_draws", "cloud_draws_aug", "cloud_prep", "cloud_augment")
    assert PD.DeviceBatchLoader(s, 4, 32, "shapenet55", False).plan() == ("cloud_draws", "fps", "cloud_prep")
    assert PD.DeviceBatchLoader(s, 4, 32, "shapenet55", True, augment=("jitter",), use_height=True)._aug_stages[-1] == "jitter"


def test_ops_validation_needs_no_device():
    import torch
    from ppt_amd import ops
    pc = torch.zeros((2, 8, 3))
    s = torch.ones(2, dtype=torch.float64)
    with pytest.raises(ValueError, match="unknown stage"):
        ops.cloud_augment(pc, [("flip", s)])
    with pytest.raises(ValueError, match="last stage"):
        ops.cloud_augment(pc, [("height",), ("scale", s)])
    with pytest.raises(ValueError, match="last stage"):
        ops.cloud_augment(pc, [("height",)], height=True)
    with pytest.raises(ValueError, match="between 1 and 8"):
        ops.cloud_augment(pc, [("scale", s)] * 9)
    with pytest.raises(ValueError, match="between 1 and 8"):
        ops.cloud_augment(pc, [("scale", s)] * 8, height=True)
    with pytest.raises(ValueError, match="between 1 and 8"):
        ops.cloud_augment(pc, [])
    with pytest.raises(ValueError, match="parameter arrays"):
        ops.cloud_augment(pc, [("affine", s)])
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.cloud_augment(pc, [("scale", s)])                                  # a well-formed list, host tensors: no CPU path
    with pytest.raises(ValueError, match="unknown magnitude"):
        ops.cloud_draws_aug(torch.zeros(2, dtype=torch.int64), 8, 0, 0, jitter=True, sigma=0.1)
    with pytest.raises(ValueError, match="nothing asked for"):
        ops.cloud_draws_aug(torch.zeros(2, dtype=torch.int64), 8, 0, 0)
    with pytest.raises(ValueError, match="either rs="):
        PD.jitter_point_cloud(pc)
    with pytest.raises(ValueError, match="float32"):
        PD.rotate_point_cloud(pc.double(), seed=1)
    assert all(hasattr(PD, f) for f in ("rotate_point_cloud", "random_point_dropout", "random_scale_point_cloud", "shift_point_cloud",
                                        "jitter_point_cloud", "rotate_perturbation_point_cloud"))


def test_entry_points_validate_arguments_without_a_launch():
    """PPT_EINVAL / PPT_EUNSUPPORTED before any launch (no device is needed to get them); header, binding and library agree."""
    from ppt_amd import build, _lib
    build.build(verbose=False)
    L = _lib.lib()
    assert {"ppt_cloud_augment_f32", "ppt_cloud_draws_aug"} <= set(_lib._SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "ppt_hip.h")).read()
    assert "int ppt_cloud_augment_f32(" in hdr and "int ppt_cloud_draws_aug(" in hdr and L.ppt_abi_version() == 7
    for name, code in (("DROPOUT", 1), ("SCALE", 2), ("SHIFT", 3), ("ROTATE", 4), ("JITTER", 5), ("AFFINE", 6), ("HEIGHT", 7),
                       ("MAX_STAGES", 8), ("MAGNITUDES", 8)):
        assert f"#define PPT_AUG_{name} {code}\n" in hdr
    one, odd = 4096, 4100                                                      # non-null addresses; never dereferenced

    def stages(*items):
        arr = (_lib.AugStage * max(1, len(items)))()
        for k, (kind, a, b) in enumerate(items):
            arr[k].kind, arr[k].a, arr[k].b = kind, a, b
        return arr

    def aug(items, pc=one, B=2, n=64, out=one, count=None, arr=True):
        return L.ppt_cloud_augment_f32(pc, B, n, stages(*items) if arr else None, len(items) if count is None else count, out, None)
    sc = (2, one, None)
    for kw in (dict(pc=None), dict(out=None), dict(B=0), dict(n=0), dict(n=-5), dict(out=odd), dict(count=0), dict(count=9), dict(arr=False)):
        assert aug([sc], **kw) == -1, kw
    assert aug([sc] * 9) == -1                                                 # more than 8 stages
    assert aug([(0, one, None)]) == -1 and aug([(8, one, None)]) == -1         # an unknown stage
    assert aug([(7, None, None), sc]) == -1                                    # height anywhere but last
    assert aug([sc, (7, None, None), (7, None, None)]) == -1
    for kind in (1, 2, 3, 4, 5, 6):
        assert aug([(kind, None, one)]) == -1, kind                            # a stage without its parameters
    assert aug([(6, one, None)]) == -1
    assert aug([(2, odd, None)]) == -1 and aug([(6, one, odd)]) == -1          # f64 arrays are 8-byte aligned
    assert aug([sc], n=8193) == -3 and aug([sc, (7, None, None)], n=20000) == -3      # the LDS limit: unsupported, not invalid
    assert aug([sc], n=8193, out=odd) == -1                                    # an invalid call stays invalid beyond the limit

    okd = dict(index=one, B=2, n=64, seed=1, epoch=0, mag=None, ratio=None, mask=None, scale=one, shift=None, angles=None, perturb=None,
               angle=None, rotate=None, noise=None, stream=None)

    def draws(**kw):
        return L.ppt_cloud_draws_aug(*{**okd, **kw}.values())
    bad_mag = (ctypes.c_double * 8)(0.875, 0.8, float("nan"), 0.1, 0.06, 0.18, 0.01, 0.05)
    for bad in (dict(index=None), dict(B=0), dict(n=0), dict(scale=None), dict(ratio=one), dict(angles=one), dict(angle=one),
                dict(mag=bad_mag)):
        assert draws(**bad) == -1, bad
    assert draws(n=8193) == -3
