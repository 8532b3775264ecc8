"""GPU: the device-resident input pipeline (csrc/cloud_prep.hip, ppt_amd/data/device_loader.py) against what the reference's
dataset code produced (tests/golden/g_datapipe.npz, tests/golden/make_golden_datapipe.py) -- bit-exact, no tolerances -- and its
device draws against Philox4x32-10 restated in Python."""
import os
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import oracle as O
from ppt_amd import weights as W
from test_datapipe_cpu import KNOWN_ANSWERS, philox4x32_10

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
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


def six(pts):
    """the same clouds with three further columns (normals): only xyz may be read"""
    return np.ascontiguousarray(np.concatenate([pts, pts[..., ::-1] * np.float32(0.5)], axis=-1))


# ------------------------------------------------------------------ 1. the kernel, stage by stage
@pytest.mark.parametrize("cols", [3, 6])
def test_cloud_prep_stages_are_bit_exact(g, ops, cols):
    small = g["small"] if cols == 3 else six(g["small"])
    src, item = dev(small), dev(np.arange(4, dtype=np.int64))
    n = g["mn_train_idx"].shape[1]
    sel = dev(g["mn_train_idx"].astype(np.int64))
    scale, shift, perm = dev(g["mn_train_scale"]), dev(g["mn_train_shift"]), dev(g["mn_train_perm"])
    lengths = dev(np.full(4, small.shape[1], dtype=np.int32))
    gathered = np.take_along_axis(g["small"], g["mn_train_idx"].astype(np.int64)[:, :, None], axis=1)
    assert np.array_equal(host(ops.cloud_prep(src, item, n, sel=sel)), gathered)                                     # gather only
    assert np.array_equal(host(ops.cloud_prep(src, item, n)), g["small"][:, :n])                                      # rows 0 .. n-1
    assert np.array_equal(host(ops.cloud_prep(src, item, n, sel=sel, normalize=True, lengths=lengths)), g["mn_train_norm"])
    assert np.array_equal(host(ops.cloud_prep(src, item, n, sel=sel, normalize=True, scale=scale, shift=shift)), g["mn_train_trans"])
    assert np.array_equal(host(ops.cloud_prep(src, item, n, sel=sel, normalize=True, scale=scale, shift=shift, perm=perm,
                                              lengths=lengths)), g["mn_train_final"])
    # ScanObjectNN's train item: no selection, no normalisation
    so = ops.cloud_prep(src, item, n, scale=dev(g["so_train_scale"]), shift=dev(g["so_train_shift"]), perm=dev(g["so_train_perm"]))
    assert np.array_equal(host(so), g["so_train_final"])
    # items in another order, repeated: each output cloud comes from the cloud `item` names
    pick = np.array([2, 0, 2, 3, 1], dtype=np.int64)
    got = ops.cloud_prep(src, dev(pick), n, sel=dev(g["mn_train_idx"].astype(np.int64)[pick]), normalize=True)
    assert np.array_equal(host(got), g["mn_train_norm"][pick])
    # the 8192 -> 1024 cloud (96 KB of LDS)
    big = dev(g["big"] if cols == 3 else six(g["big"]))
    got = ops.cloud_prep(big, dev(np.zeros(1, np.int64)), g["mnbig_train_idx"].shape[1], sel=dev(g["mnbig_train_idx"].astype(np.int64)),
                         normalize=True, scale=dev(g["mnbig_train_scale"]), shift=dev(g["mnbig_train_shift"]),
                         perm=dev(g["mnbig_train_perm"]))
    assert np.array_equal(host(got), g["mnbig_train_final"])
    # n not a multiple of 4 (the narrow store path): the first 511 rows' normalisation, against the same arithmetic in numpy
    from ppt_amd.data import pc_normalize
    got = host(ops.cloud_prep(src, item, 511, normalize=True))
    assert all(np.array_equal(got[i], pc_normalize(g["small"][i, :511])) for i in range(4))


@pytest.mark.parametrize("cols", [3, 6])
def test_cloud_prep_part_seg_is_bit_exact(g, ops, cols):
    from ppt_amd.data import pc_normalize
    L = g["part_lengths"]
    pts = g["small"].copy()
    for i in range(4):
        pts[i, :L[i]] = pc_normalize(pts[i, :L[i]])                  # DeviceCloudSet does this once, on the host
    src = dev(pts if cols == 3 else six(pts))
    n = g["sp_sel"].shape[1]
    out, seg = ops.cloud_prep(src, dev(np.arange(4, dtype=np.int64)), n, sel=dev(g["sp_sel"].astype(np.int64)), lengths=dev(L),
                              seg_src=dev(g["seg"]))
    assert seg.dtype == torch.int64
    assert np.array_equal(host(out), g["sp_final"]) and np.array_equal(host(seg), g["sp_seg"].astype(np.int64))
    # with a permutation the labels follow their points
    perm = dev(g["mn_train_perm"])
    out2, seg2 = ops.cloud_prep(src, dev(np.arange(4, dtype=np.int64)), n, sel=dev(g["sp_sel"].astype(np.int64)), lengths=dev(L),
                                seg_src=dev(g["seg"]), perm=perm)
    p = g["mn_train_perm"].astype(np.int64)
    assert np.array_equal(host(out2), np.take_along_axis(g["sp_final"], p[:, :, None], axis=1))
    assert np.array_equal(host(seg2), np.take_along_axis(g["sp_seg"].astype(np.int64), p, axis=1))


# ------------------------------------------------------------------ 2. the loader in numpy-draw mode
def _sets(g):
    from ppt_amd.data import DeviceCloudSet
    labels = np.array([3, 9, 27, 11])
    return {"small": DeviceCloudSet(g["small"], labels), "small6": DeviceCloudSet(six(g["small"]), labels),
            "big": DeviceCloudSet(g["big"], [5]),
            "part": DeviceCloudSet([g["small"][i, :L] for i, L in enumerate(g["part_lengths"])], labels % 16,
                                   seg=[g["seg"][i, :L] for i, L in enumerate(g["part_lengths"])])}


@pytest.mark.parametrize("batch", [4, 3])
def test_loader_numpy_draws_reproduce_the_reference(g, batch):
    from ppt_amd.data import DeviceBatchLoader
    sets = _sets(g)
    seed = int(g["seed"])
    n = g["mn_train_final"].shape[1]

    def run(key, recipe, train, npoints=n, bs=batch):
        ld = DeviceBatchLoader(sets[key], bs, npoints, recipe, train, shuffle=False, seed=seed, draws="numpy")
        batches = list(ld)
        assert len(batches) == len(ld)
        return [torch.cat([b[k] for b in batches]) for k in range(len(batches[0]))]
    for key in ("small", "small6"):
        pc, target = run(key, "modelnet", True)
        assert pc.dtype == torch.float32 and target.dtype == torch.int64 and tuple(pc.shape) == (4, n, 3)
        assert np.array_equal(host(pc), g["mn_train_final"]) and host(target).tolist() == [3, 9, 27, 11]
        pc, _ = run(key, "modelnet", False)
        assert np.array_equal(host(pc), g["mn_test_final"])
        pc, _ = run(key, "scanobjectnn", True)
        assert np.array_equal(host(pc), g["so_train_final"])
        pc, _ = run(key, "scanobjectnn", False)
        assert np.array_equal(host(pc), g["small"][:, :n])
    pc, target = run("big", "modelnet", True, npoints=g["mnbig_train_final"].shape[1])
    assert np.array_equal(host(pc), g["mnbig_train_final"]) and host(target).tolist() == [5]
    for train in (True, False):
        pc, cls, seg = run("part", "shapenetpart", train)
        assert cls.dtype == torch.int32 and tuple(cls.shape) == (4, 1) and seg.dtype == torch.int64
        assert np.array_equal(host(pc), g["sp_final"]) and np.array_equal(host(seg), g["sp_seg"].astype(np.int64))
        assert host(cls).reshape(-1).tolist() == [3, 9, 11, 11]


def test_loader_fps_indices_match_the_reference_walk(g, ops):
    """The loader's FPS stage selects the reference's rows: the recorded indices, and oracle.dataset_farthest_point_sample (pinned to
    the reference function by tests/golden/make_golden.py) on further random sizes, duplicates included."""
    from ppt_amd.data import DeviceBatchLoader, DeviceCloudSet, numpy_draws, pc_normalize
    rng = np.random.default_rng(8)
    for m, rows, npoints, cols in ((3, 1500, 1024, 3), (5, 333, 70, 6), (2, 4096, 2048, 3)):
        clouds = rng.standard_normal((m, rows, cols)).astype(np.float32)
        clouds[:, rows // 2:rows // 2 + 5] = clouds[:, :1]            # duplicates
        ld = DeviceBatchLoader(DeviceCloudSet(clouds, np.arange(m)), 2, npoints, "modelnet", False, shuffle=False, seed=41, draws="numpy")
        got = torch.cat([b[0] for b in ld])
        rs = np.random.RandomState([41, 0, 0])
        for i in range(m):
            want_rows, _ = O.dataset_farthest_point_sample(clouds[i], npoints, numpy_draws(rs, "modelnet", False, rows, npoints)["start"])
            assert np.array_equal(host(got[i]), pc_normalize(want_rows[:, :3]))
    # the recorded indices themselves, through the same launch the loader makes
    idx, _ = ops.fps(dev(g["small"]), g["mn_train_idx"].shape[1], dev(g["mn_train_start"].astype(np.int64)))
    assert np.array_equal(host(idx), g["mn_train_idx"].astype(np.int64))


# ------------------------------------------------------------------ 3. device draws
def _i32(a):
    return np.asarray(a, dtype=np.uint32).view(np.int32)


def _bounded(idx, epoch, slot, block, key, rng):
    """Lemire's unbiased bounded integer over the words of Philox blocks, as csrc/cloud_prep.hip does it"""
    thresh = ((1 << 32) - rng) % rng
    for attempt in range(16):
        for w in philox4x32_10((idx, epoch, slot | (attempt << 8), block), key):
            if (w * rng) & 0xFFFFFFFF >= thresh:
                return (w * rng) >> 32
    raise AssertionError("unreachable")


def _u53(hi, lo):
    return float(((hi >> 5) << 26) | (lo >> 6)) * (1.0 / 9007199254740992.0)


def test_philox_known_answers_and_counters(ops):
    for ctr, key, want in KNOWN_ANSWERS:
        got = host(ops.philox4x32(dev(_i32([ctr])), key[0] | (key[1] << 32))).view(np.uint32)[0]
        assert tuple(int(x) for x in got) == want, (ctr, [hex(int(x)) for x in got])
    r = np.random.default_rng(0)
    ctrs = r.integers(0, 1 << 32, size=(3000, 4), dtype=np.uint64).astype(np.uint32)
    ctrs[:64, 0] = np.arange(64)                                     # and runs of neighbouring counters
    ctrs[:64, 1:] = ctrs[0, 1:]
    seed = 0x9E3779B97F4A7C15
    got = host(ops.philox4x32(dev(ctrs.view(np.int32)), seed)).view(np.uint32)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    want = np.array([philox4x32_10(c, key) for c in ctrs], dtype=np.uint32)
    assert np.array_equal(got, want)


def test_device_draws_are_the_documented_function_of_the_counter(ops):
    """start / scale / shift / perm / sel equal the Python restatement: counter (index, epoch, slot, block), key = seed."""
    seed, epoch, n = 0x1234567887654321, 3, 200
    key = (seed & 0xFFFFFFFF, seed >> 32)
    index = np.array([0, 7, 123456, 2 ** 31 + 5], dtype=np.int64)
    rows = np.array([8192, 1500, 2, 16384], dtype=np.int32)
    d = ops.cloud_draws(dev(index), n, seed, epoch, rows=dev(rows), start=True, affine=True, perm=True, sel=True)
    d = {k: host(v) for k, v in d.items()}
    for b, (ix, rw) in enumerate(zip(index.tolist(), rows.tolist())):
        ix &= 0xFFFFFFFF
        assert d["start"][b] == _bounded(ix, epoch, 0, 0, key, rw)
        for c in range(3):
            w = philox4x32_10((ix, epoch, 1, c), key)
            assert d["scale"][b, c] == 2.0 / 3.0 + (3.0 / 2.0 - 2.0 / 3.0) * _u53(w[0], w[1])
            assert d["shift"][b, c] == -0.2 + (0.2 - -0.2) * _u53(w[2], w[3])
        keys = np.array([philox4x32_10((ix, epoch, 2, j), key) for j in range((n + 3) // 4)], dtype=np.uint64).reshape(-1)[:n]
        assert np.array_equal(d["perm"][b], np.lexsort((np.arange(n), keys)))              # by key, ties by position
        assert d["sel"][b].tolist() == [_bounded(ix, epoch, 3, i, key, rw) for i in range(n)]
    # rows_all in place of a per-sample row count; only what is asked for is drawn
    d2 = ops.cloud_draws(dev(index[:2]), n, seed, epoch, rows_all=1500, start=True)
    assert sorted(d2) == ["start"] and host(d2["start"])[1] == d["start"][1]


def test_device_draws_ranges_and_distribution(ops):
    for n in (1, 5, 512, 1000, 1024, 8192):
        B = 6 if n > 1024 else 40
        d = ops.cloud_draws(dev(np.arange(B, dtype=np.int64) * 977), n, 11, 0, rows_all=777, start=True, affine=True, perm=True, sel=True)
        assert np.array_equal(np.sort(host(d["perm"]), axis=1), np.tile(np.arange(n, dtype=np.int32), (B, 1))), n
        assert d["perm"].dtype == torch.int32 and d["sel"].dtype == torch.int64 and d["scale"].dtype == torch.float64
        for k, lo, hi in (("start", 0, 777), ("sel", 0, 777), ("scale", 2 / 3, 3 / 2), ("shift", -0.2, 0.2)):
            v = host(d[k])
            assert v.min() >= lo and v.max() < hi, (k, n)
    # loose distribution checks: the mean of N draws within 5 standard errors of the distribution's mean (uniform on [a, b):
    # sd = (b - a) / sqrt(12); uniform integers on [0, r): sd = sqrt((r^2 - 1) / 12)) -- derived, not tuned
    B = 34000
    d = ops.cloud_draws(dev(np.arange(B, dtype=np.int64)), 4, 2024, 1, rows_all=1000, start=True, affine=True, perm=True, sel=True)
    N = 3 * B
    assert N >= 10 ** 5
    for k, a, b in (("scale", 2 / 3, 3 / 2), ("shift", -0.2, 0.2)):
        v = host(d[k]).reshape(-1)
        assert abs(v.mean() - (a + b) / 2) < 5 * (b - a) / np.sqrt(12 * N), k
    for k in ("start", "sel"):
        v = host(d[k]).reshape(-1).astype(np.float64)
        assert abs(v.mean() - 999 / 2) < 5 * np.sqrt((1000 ** 2 - 1) / 12 / v.size), k
    first = host(d["perm"])[:, 0].astype(np.float64)                   # the first element of a uniform permutation of 4
    assert abs(first.mean() - 1.5) < 5 * np.sqrt((4 ** 2 - 1) / 12 / B)


def _by_index(loader, epoch=0):
    loader.set_epoch(epoch)
    out = {}
    order = loader.indices()
    k = 0
    for batch in loader:
        for row in host(batch[0]):
            out.setdefault(int(order[k]), row)
            k += 1
    assert k == len(order)
    return out


@pytest.mark.parametrize("recipe", ["modelnet", "scanobjectnn", "shapenetpart"])
def test_device_draws_do_not_depend_on_batching(recipe):
    from ppt_amd.data import DeviceBatchLoader, DeviceCloudSet
    r = np.random.default_rng(2)
    m, rows, n = 70, 256, 64
    s = DeviceCloudSet(r.standard_normal((m, rows, 3)).astype(np.float32), np.arange(m) % 7,
                       seg=r.integers(0, 9, (m, rows)).astype(np.int32) if recipe == "shapenetpart" else None)

    def mk(bs, world=1, rank=0, seed=5):
        return DeviceBatchLoader(s, bs, n, recipe, True, seed=seed, world_size=world, rank=rank)
    a = _by_index(mk(8))
    assert sorted(a) == list(range(m))
    for other in (_by_index(mk(8)), _by_index(mk(32))):               # the same seed again; another batch size
        assert all(np.array_equal(a[i], other[i]) for i in range(m))
    halves = {**_by_index(mk(8, 2, 0)), **_by_index(mk(8, 2, 1))}     # two ranks
    assert sorted(halves) == list(range(m)) and all(np.array_equal(a[i], halves[i]) for i in range(m))
    nxt = _by_index(mk(8), epoch=1)
    assert not any(np.array_equal(a[i], nxt[i]) for i in range(m))    # another epoch, other draws
    other_seed = _by_index(mk(8, seed=6))
    assert not any(np.array_equal(a[i], other_seed[i]) for i in range(m))
    # two loaders, one seed: identical epochs, batch by batch
    for x, y in zip(mk(16), mk(16)):
        assert all(torch.equal(p, q) for p, q in zip(x, y))


# ------------------------------------------------------------------ 4. plumbing
def test_batches_carry_events_and_are_never_reused(g):
    from ppt_amd.data import DeviceBatchLoader, DeviceCloudSet
    n = g["mn_train_final"].shape[1]
    s = DeviceCloudSet(np.concatenate([g["small"], g["small"][::-1]] * 2), np.arange(16) % 4)          # four batches of four
    it = iter(DeviceBatchLoader(s, 4, n, "modelnet", True, shuffle=False, seed=int(g["seed"]), draws="numpy", ahead=2))
    first = next(it)
    assert all(isinstance(getattr(t, "_ppt_ready", None), torch.cuda.Event) for t in first)
    held = first[0]
    more = [next(it) for _ in range(3)]                               # three further batches produced while `held` is alive
    assert next(it, None) is None
    filler = [torch.empty_like(held).normal_() for _ in range(8)]     # and allocations that would land in a freed block
    torch.cuda.synchronize()
    assert np.array_equal(host(held), g["mn_train_final"])
    assert held.data_ptr() not in {b[0].data_ptr() for b in more} | {f.data_ptr() for f in filler}


def test_trainer_steps_from_the_loader():
    """A C2 Trainer (ModelNet40 class list, head_type 0, 32 x 1024 points) takes three steps from device-draw batches whose tensors
    it has not been told are ready: the ahead stage waits on the loader's event.  Finite loss each step."""
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
    assert not tr.inputs_ready
    pc, _ = W.synth_clouds(96, 2048, seed=5)
    s = DeviceCloudSet(pc, np.arange(96) % len(names))
    losses = []
    for pcb, target in DeviceBatchLoader(s, 32, 1024, "modelnet", True, seed=1):
        assert pcb._ppt_ready is not None and tuple(pcb.shape) == (32, 1024, 3)
        loss, _ = tr.step(pcb, target)
        losses.append(loss)
    tr.finish()
    torch.cuda.synchronize()
    assert len(losses) == 3 and all(np.isfinite(float(x.detach())) for x in losses), losses


def test_loader_rate_floor():
    """The loader alone (device draws, ModelNet recipe, 32 clouds 8192 -> 1024 per batch) against a floor that an accidental host
    synchronise or per-sample host work would break (RATE_FLOOR below, with the measured figures it comes from)."""
    from ppt_amd.data import DeviceBatchLoader, DeviceCloudSet
    pc, _ = W.synth_clouds(128, 8192, seed=3)
    s = DeviceCloudSet(pc, np.arange(128) % 40)
    ld = DeviceBatchLoader(s, 32, 1024, "modelnet", True, seed=0)
    rates = []
    for rep in range(4):
        ld.set_epoch(rep)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clouds = 0
        for _ in range(5):
            for pcb, _t in ld:
                clouds += pcb.shape[0]
        torch.cuda.synchronize()
        rates.append(clouds / (time.perf_counter() - t0))
    print("DATAPIPE loader-alone clouds/s per repeat (first = warm-up):", [round(r) for r in rates])
    assert min(rates[1:]) > RATE_FLOOR, rates


# First measured run on an MI355X, clouds/s per repeat: 30 866 (with the warm-up), 31 040, 31 068, 31 096 -- one batch is one 1.03 ms
# FPS walk.  The floor is half of the slowest of them; it is there to catch a host synchronise per batch, not to rank kernels.
RATE_FLOOR = 30866 / 2
