"""CPU: the host side of ragged clouds -- the four ppt_*_ragged_f32 entry points are declared, bound, exported and refuse bad
arguments before any launch; DeviceBatchLoader(ragged=) and the encoders' lengths= validation.  No device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ppt_amd.data as PD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = ("ppt_fps_ragged_f32", "ppt_knn_group_ragged_f32", "ppt_ball_query_ragged_f32", "ppt_ball_query_multi_ragged_f32")


def test_ragged_entry_points_are_declared_bound_and_exported():
    from ppt_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppt_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in RAGGED:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib._SIGNATURES and hasattr(L, name), name
        uniform = name.replace("_ragged", "")
        assert len(_lib._SIGNATURES[name][1]) == len(_lib._SIGNATURES[uniform][1]) + 1       # the old arguments + lengths
    assert _lib.lib().ppt_abi_version() == 7


def test_ragged_entry_points_refuse_bad_arguments_before_any_launch():
    """a null lengths, B <= 0 and Nmax over the entry point's limit are PPT_EINVAL (-1); the pointers are host dummies that a
    launch would fault on, so every return below happened in front of one"""
    from ppt_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    q = _lib.BallMulti()
    q.n, q.K[0], q.idx[0] = 1, 4, p.value
    calls = {
        "fps": (lambda B, N, ln: L.ppt_fps_ragged_f32(p, B, N, 4, p, ln, p, p, None), 16384),
        "knn": (lambda B, N, ln: L.ppt_knn_group_ragged_f32(p, p, B, N, 4, 4, ln, p, p, None, None), 8192),
        "ball": (lambda B, N, ln: L.ppt_ball_query_ragged_f32(p, p, B, N, 4, 0.04, 4, ln, p, None, None), 10240),
        "multi": (lambda B, N, ln: L.ppt_ball_query_multi_ragged_f32(p, p, B, N, 4, ln, ctypes.byref(q), None), 10240),
    }
    for name, (call, limit) in calls.items():
        assert call(2, 64, None) == -1, name
        assert call(0, 64, p) == -1 and call(-3, 64, p) == -1, name
        assert call(2, limit + 1, p) == -1 and call(2, 0, p) == -1, name


def _cpu_set(lengths, rows=None):
    r = np.random.default_rng(2)
    lengths = np.asarray(lengths, dtype=np.int32)
    pts = r.standard_normal((len(lengths), int(rows or lengths.max()), 3)).astype(np.float32)
    return PD.DeviceCloudSet(pts, np.arange(len(lengths)), lengths=lengths, device="cpu")


def test_loader_ragged_option():
    lens = [96, 64, 80, 33, 64, 96]
    s = _cpu_set(lens)
    for recipe in ("modelnet", "shapenet55"):
        with pytest.raises(ValueError, match="one row count.*ragged=True"):
            PD.DeviceBatchLoader(s, 4, 32, recipe, True)
        ld = PD.DeviceBatchLoader(s, 4, 32, recipe, False, ragged=True)
        uniform = PD.DeviceBatchLoader(_cpu_set([96] * 6), 4, 32, recipe, False)
        assert ld.plan() == uniform.plan() == ("cloud_draws", "fps", "cloud_prep")
        assert PD.DeviceBatchLoader(s, 4, 32, recipe, False, ragged=True, draws="numpy").plan() == ("fps", "cloud_prep")
        with pytest.raises(ValueError, match="at least npoints"):
            PD.DeviceBatchLoader(s, 4, 40, recipe, True, ragged=True)
    train = PD.DeviceBatchLoader(s, 4, 32, "modelnet", True, ragged=True)
    assert train.plan() == PD.DeviceBatchLoader(_cpu_set([96] * 6), 4, 32, "modelnet", True).plan()
    # a cloud of exactly npoints rows: taken as stored under "modelnet", refused under "shapenet55" (random_sample's permutation)
    exact = _cpu_set([96, 32, 80, 33])
    assert PD.DeviceBatchLoader(exact, 4, 32, "modelnet", True, ragged=True).plan() == train.plan()
    with pytest.raises(ValueError, match="exactly npoints"):
        PD.DeviceBatchLoader(exact, 4, 32, "shapenet55", True, ragged=True)
    # ragged=True on a uniform set is today's loader; the recipes without FPS never needed it
    assert PD.DeviceBatchLoader(_cpu_set([64] * 4), 4, 32, "modelnet", True, ragged=True).plan() == train.plan()
    assert PD.DeviceBatchLoader(s, 4, 32, "scanobjectnn", True, ragged=True).plan() == ("cloud_draws", "cloud_prep")


def test_numpy_draws_skip_the_start_of_an_unsampled_cloud():
    """a cloud of exactly npoints rows draws no randint, as the reference's dataset does not; its neighbours in the batch still do"""
    ld = PD.DeviceBatchLoader(_cpu_set([96, 32, 80]), 3, 32, "modelnet", False, ragged=True, draws="numpy")
    rs, want = np.random.RandomState(4), np.random.RandomState(4)
    per = [PD.numpy_draws(rs, "modelnet", False, n, 32) for n in (96, 32, 80)]
    assert "start" in per[0] and "start" not in per[1] and "start" in per[2]
    assert per[0]["start"] == want.randint(0, 96) and per[2]["start"] == want.randint(0, 80)
    assert ld._ragged and ld._exact and ld._fps_rows == 96


def test_lengths_validation_on_the_host():
    from ppt_amd import engine
    ok = engine.cloud_lengths([64, 33, 1], 3, 64, "cpu")
    assert ok.dtype == torch.int32 and ok.tolist() == [64, 33, 1]
    assert engine.cloud_lengths(np.array([40, 64], dtype=np.int64), 2, 64, "cpu", least=32).tolist() == [40, 64]
    for bad, kw in (([64, 65], {}), ([0, 64], {}), ([64, 31], dict(least=32)), ([64], {}), ([[64, 64]], {}), ([64.0, 32.0], {})):
        with pytest.raises(ValueError, match="lengths"):
            engine.cloud_lengths(bad, 2, 64, "cpu", **kw)


def test_encoders_validate_lengths_before_any_launch():
    from ppt_amd.models.pointbert.dvae import Group
    from ppt_amd.models.pointnet2.pointnet2 import Pointnet2_Msg, Pointnet2_Ssg
    pc = torch.zeros(2, 64, 3)
    with pytest.raises(ValueError, match="lengths"):
        Group(8, 32)(pc, lengths=[64, 31])                       # below group_size
    with pytest.raises(ValueError, match="lengths"):
        Group(8, 32)(pc, lengths=[64, 65])
    for cls in (Pointnet2_Msg, Pointnet2_Ssg):
        with pytest.raises(ValueError, match="lengths"):
            cls()(pc, lengths=[64, 0])
        with pytest.raises(ValueError, match="lengths"):
            cls()(pc, lengths=[64, 64, 64])


def test_encoders_without_a_ragged_form_refuse_lengths():
    from ppt_amd.models.pointmlp.pointMLP import pointMLP
    from ppt_amd.models.pointnext.pointnext import PointNEXT
    with pytest.raises(ValueError, match="lengths"):
        pointMLP()(torch.zeros(2, 64, 3), lengths=[64, 40])
    with pytest.raises(ValueError, match="lengths"):
        PointNEXT()(torch.zeros(2, 64, 4), lengths=[64, 40])
