"""CPU: the device-resident input pipeline's host side (ppt_amd/data/device_loader.py) -- epoch order, length, the numpy draw
order, input validation, the C entry points' argument checks -- and the Philox reference the GPU tests compare the device with."""
import ctypes
import os

import numpy as np
import pytest
import torch

from ppt_amd import data as PD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Sized:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), from its constants."""
    c0, c1, c2, c3 = (int(x) for x in ctr)
    k0, k1 = (int(x) for x in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return (c0, c1, c2, c3)


KNOWN_ANSWERS = [      # Random123's kat_vectors, philox4x32 10 rounds
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_python_philox_matches_published_answers():
    for ctr, key, want in KNOWN_ANSWERS:
        assert philox4x32_10(ctr, key) == want


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("shuffle", [True, False])
def test_epoch_order_is_distributed_samplers(world, drop_last, shuffle):
    from torch.utils.data import DistributedSampler
    for n_items in (37, 5, 2):
        for rank in range(world):
            sm = DistributedSampler(_Sized(n_items), num_replicas=world, rank=rank, shuffle=shuffle, seed=7, drop_last=drop_last)
            for epoch in (0, 1):
                sm.set_epoch(epoch)
                got = PD.epoch_indices(n_items, epoch, shuffle, 7, drop_last, rank, world)
                assert got.dtype == np.int64 and got.tolist() == list(sm), (n_items, rank, epoch)
    if shuffle:
        assert PD.epoch_indices(37, 0, True, 7).tolist() != PD.epoch_indices(37, 1, True, 7).tolist()
        assert PD.epoch_indices(37, 1, True, 7).tolist() == PD.epoch_indices(37, 0, True, 8).tolist()      # seed + epoch


def _cpu_set(m=37, n=64, seg=False, lengths=None):
    r = np.random.default_rng(0)
    return PD.DeviceCloudSet(r.standard_normal((m, n, 3)).astype(np.float32), np.arange(m) % 5,
                             seg=r.integers(0, 4, (m, n)).astype(np.int32) if seg else None, lengths=lengths, device="cpu")


def test_len_and_loader_order():
    s = _cpu_set()
    assert len(s) == 37
    for world, drop_last, bs, want in ((1, False, 8, 5), (1, True, 8, 4), (2, False, 8, 3), (2, True, 8, 2), (3, True, 4, 3),
                                       (3, False, 4, 4)):
        ld = PD.DeviceBatchLoader(s, bs, 32, "scanobjectnn", True, drop_last=drop_last, seed=3, world_size=world, rank=world - 1)
        assert len(ld) == want, (world, drop_last, bs)
        ld.set_epoch(4)
        assert ld.indices().tolist() == PD.epoch_indices(37, 4, True, 3, drop_last, world - 1, world).tolist()
    with pytest.raises(RuntimeError, match="no CPU path"):
        next(iter(PD.DeviceBatchLoader(s, 8, 32, "scanobjectnn", True)))


def test_numpy_draw_order_and_generator_state():
    """numpy_draws consumes the RandomState exactly as the documented sequence does -- same values, same state afterwards."""
    n = 48
    for recipe, train, rows in (("modelnet", True, 200), ("modelnet", False, 200), ("modelnet", True, n), ("scanobjectnn", True, 200),
                                ("scanobjectnn", False, 200), ("shapenetpart", True, 131), ("shapenetpart", False, 131)):
        a, b = np.random.RandomState(99), np.random.RandomState(99)
        d = PD.numpy_draws(a, recipe, train, rows, n)
        want = {}
        if recipe == "shapenetpart":
            want["sel"] = b.choice(rows, n, replace=True)
        else:
            if recipe == "modelnet" and rows > n:
                want["start"] = b.randint(0, rows)
            if train:
                want["scale"] = b.uniform(2. / 3., 3. / 2., 3)
                want["shift"] = b.uniform(-0.2, 0.2, 3)
                want["perm"] = b.permutation(n)
        assert sorted(d) == sorted(want), (recipe, train, rows)
        for k in want:
            assert np.array_equal(d[k], want[k]), (recipe, k)
        assert a.randint(0, 1 << 30) == b.randint(0, 1 << 30)
    # permutation(n) is what np.random.shuffle does to the rows of a cloud, and leaves the generator where shuffle does
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    cloud = np.random.default_rng(1).standard_normal((n, 3)).astype(np.float32)
    shuffled = cloud.copy()
    a.shuffle(shuffled)
    assert np.array_equal(cloud[b.permutation(n)], shuffled) and a.randint(0, 1 << 30) == b.randint(0, 1 << 30)


def test_input_validation():
    r = np.random.default_rng(0)
    with pytest.raises(TypeError, match="float32 clouds only"):
        PD.DeviceCloudSet(r.standard_normal((2, 16, 3)), [0, 1], device="cpu")
    with pytest.raises(TypeError, match="float32 clouds only"):
        PD.DeviceCloudSet([r.standard_normal((16, 3))], [0], device="cpu")
    with pytest.raises(ValueError, match="at most 16384"):
        PD.DeviceCloudSet(np.zeros((1, 16385, 3), np.float32), [0], device="cpu")
    with pytest.raises(ValueError, match="labels"):
        PD.DeviceCloudSet(np.zeros((2, 16, 3), np.float32), [0], device="cpu")
    s = _cpu_set()
    with pytest.raises(ValueError, match="recipe"):
        PD.DeviceBatchLoader(s, 8, 32, "shapenet", True)
    with pytest.raises(ValueError, match="draws"):
        PD.DeviceBatchLoader(s, 8, 32, "modelnet", True, draws="torch")
    with pytest.raises(ValueError, match="npoints"):
        PD.DeviceBatchLoader(s, 8, 8193, "modelnet", True)
    with pytest.raises(ValueError, match="at least npoints"):
        PD.DeviceBatchLoader(s, 8, 65, "modelnet", True)
    with pytest.raises(ValueError, match="needs a DeviceCloudSet with seg"):
        PD.DeviceBatchLoader(s, 8, 32, "shapenetpart", True)
    with pytest.raises(ValueError, match="one row count"):
        PD.DeviceBatchLoader(_cpu_set(lengths=np.r_[np.full(36, 64), 50]), 8, 32, "modelnet", True)
    with pytest.raises(ValueError, match="rank"):
        PD.DeviceBatchLoader(s, 8, 32, "modelnet", True, rank=2, world_size=2)


def test_ragged_lists_are_padded_and_part_sets_normalised_once():
    r = np.random.default_rng(3)
    clouds = [r.standard_normal((n, 3)).astype(np.float32) + np.float32(2.0) for n in (40, 64, 51)]
    segs = [r.integers(0, 4, len(c)).astype(np.int32) for c in clouds]
    s = PD.DeviceCloudSet(clouds, [0, 1, 2], seg=segs, device="cpu")
    assert tuple(s.points.shape) == (3, 64, 3) and s.lengths.tolist() == [40, 64, 51] and s.lengths.dtype == torch.int32
    for i, c in enumerate(clouds):
        assert np.array_equal(s.points[i, :len(c)].numpy(), PD.pc_normalize(c))
        assert np.array_equal(s.seg[i, :len(c)].numpy(), segs[i])
    plain = PD.DeviceCloudSet(clouds, [0, 1, 2], device="cpu")                # no seg: stored as given
    assert np.array_equal(plain.points[0, :40].numpy(), clouds[0])


def test_entry_points_validate_arguments_without_a_launch():
    """PPT_EINVAL before any launch (no device is needed to get it), and header <-> binding agree on the two new entries."""
    from ppt_amd import build, _lib
    build.build(verbose=False)
    L = _lib.lib()
    assert {"ppt_cloud_prep_f32", "ppt_cloud_draws"} <= set(_lib._SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "ppt_hip.h")).read()
    assert "int ppt_cloud_prep_f32(" in hdr and "int ppt_cloud_draws(" in hdr
    assert L.ppt_abi_version() == 7
    one = ctypes.c_void_p(4096)                                                # a non-null, 16-byte aligned value; never dereferenced
    ok = dict(src=one, M=4, Nmax=2048, C=3, lengths=None, item=one, B=2, sel=None, n=512, normalize=1, translate=0, scale=None,
              shift=None, perm=None, seg_src=None, seg_out=None, out=one, stream=None)

    def prep(**kw):
        return L.ppt_cloud_prep_f32(*{**ok, **kw}.values())
    for bad in (dict(src=None), dict(item=None), dict(out=None), dict(M=0), dict(Nmax=0), dict(Nmax=16385), dict(C=2), dict(B=0),
                dict(n=0), dict(n=8193), dict(n=2049), dict(translate=1), dict(translate=1, scale=one), dict(seg_src=one),
                dict(seg_out=one), dict(out=ctypes.c_void_p(4100))):
        assert prep(**bad) == -1, bad
    okd = dict(index=one, B=2, rows=None, rows_all=2048, n=512, seed=1, epoch=0, start=one, scale=None, shift=None, perm=None, sel=None,
               raw_ctr=None, raw_count=0, raw_out=None, stream=None)

    def draws(**kw):
        return L.ppt_cloud_draws(*{**okd, **kw}.values())
    for bad in (dict(index=None), dict(B=0), dict(n=0), dict(n=8193), dict(start=None), dict(scale=one), dict(shift=one),
                dict(rows_all=0), dict(rows_all=16385), dict(raw_ctr=one), dict(raw_out=one), dict(raw_ctr=one, raw_out=one),
                dict(raw_ctr=one, raw_out=ctypes.c_void_p(4100), raw_count=1),
                dict(index=None, B=0, start=None)):
        assert draws(**bad) == -1, bad
