#!/usr/bin/env python3
"""Generate tests/golden/g_datapipe.npz: what the UPSTREAM REFERENCE's dataset code (data/dataset_3d.py, imported through
tests/golden/ref_import.py) makes of seeded synthetic clouds, for the device-resident input pipeline
(ppt_amd/data/device_loader.py, csrc/cloud_prep.hip).  Build container only; only arrays are stored.

    python tests/golden/make_golden_datapipe.py

Per recipe and split the reference's own functions are run sample after sample on the global numpy generator seeded with
[SEED, 0, 0] -- the statements of ModelNet._get_item / __getitem__ (:291-315), ScanObjectNN.__getitem__ (:406-412) and
ShapeNetPart.__getitem__ (:750-755) -- and the outputs are stored.  While generating, the script asserts that
  * replaying the documented draw order (ppt_amd.data.numpy_draws) on a RandomState with the same seed reproduces every output and
    leaves the generator in the same state (the pin of the loader's draws="numpy" mode), and
  * the arithmetic csrc/cloud_prep.hip is written to (sequential float32 centroid sum, (x*x + y*y) + z*z, correctly rounded sqrt
    and division, float64 multiply-add rounded once) reproduces pc_normalize / translate_pointcloud bit for bit.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_import as R                     # noqa: E402
from ppt_amd import weights as W           # noqa: E402
from ppt_amd.data import numpy_draws       # noqa: E402
from oracle import oracle as O             # noqa: E402

SEED = 20240
SMALL_N, SMALL_M, BIG_N, BIG_M = 2048, 512, 8192, 1024
PART_LENGTHS = np.array([2048, 1500, 1801, 2048], dtype=np.int32)


def inputs():
    """4 clouds of 2048 rows (the last one resampled with replacement: duplicate points) and one of 8192, moved off the unit
    sphere so that normalising them does something."""
    a, _ = W.synth_clouds(3, SMALL_N, seed=SEED)
    d, _ = W.synth_clouds(1, SMALL_N, seed=SEED + 1, duplicates=True)
    small = np.concatenate([a, d], 0) * np.float32([1.7, 0.6, 1.1]) + np.float32([0.3, -0.2, 0.5])
    big, _ = W.synth_clouds(1, BIG_N, seed=SEED + 2)
    big = big * np.float32([0.8, 1.3, 2.1]) + np.float32([-0.4, 0.1, 0.25])
    seg = np.random.default_rng(SEED).integers(0, 50, size=(4, SMALL_N)).astype(np.int32)
    return small.astype(np.float32), big.astype(np.float32), seg


def normalize_as_kernel(p):
    """csrc/cloud_prep.hip's pc_normalize, one float32 operation at a time"""
    f = np.float32
    c = np.zeros(3, f)
    for row in p:
        c = (c + row).astype(f)
    c = (c / f(p.shape[0])).astype(f)
    q = (p - c).astype(f)
    r2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]).astype(f) + q[:, 2] * q[:, 2]).astype(f)
    m = np.sqrt(r2).max()
    return (q / m).astype(f)


def translate_as_kernel(p, scale, shift):
    return (p.astype(np.float64) * scale + shift).astype(np.float32)


def main():
    small, big, seg = inputs()
    with R.reference_context():
        import data.dataset_3d as D
    out = {"seed": np.int64(SEED), "small": small, "big": big, "seg": seg, "part_lengths": PART_LENGTHS}

    def modelnet(tag, clouds, npoints, train, keep_stages):
        np.random.seed([SEED, 0, 0])
        rs = np.random.RandomState([SEED, 0, 0])
        res = {k: [] for k in ("idx", "norm", "trans", "final", "start", "scale", "shift", "perm")}
        for pts in clouds:
            # ModelNet._get_item + __getitem__, data/dataset_3d.py:291-315
            points = D.farthest_point_sample(pts, npoints)
            points = points[:, 0:3]
            points[:, 0:3] = D.pc_normalize(points[:, 0:3])
            norm = points.copy()
            if train:
                trans = D.translate_pointcloud(points)
                final = trans.copy()
                np.random.shuffle(final)
            else:
                trans = final = points
            # the replay
            d = numpy_draws(rs, "modelnet", train, pts.shape[0], npoints)
            rows, idx = O.dataset_farthest_point_sample(pts, npoints, d["start"])
            assert np.array_equal(rows[:, :3], D_rows(pts, idx))
            n2 = normalize_as_kernel(pts[idx])
            assert np.array_equal(n2, norm), "kernel-order pc_normalize differs from the reference"
            if train:
                t2 = translate_as_kernel(n2, d["scale"], d["shift"])
                assert np.array_equal(t2, trans), "kernel-order translate differs from the reference"
                assert np.array_equal(t2[d["perm"]], final), "permutation(n) is not what np.random.shuffle did"
            res["idx"].append(idx.astype(np.int32)); res["norm"].append(norm); res["trans"].append(trans); res["final"].append(final)
            res["start"].append(d["start"])
            if train:
                res["scale"].append(d["scale"]); res["shift"].append(d["shift"]); res["perm"].append(d["perm"].astype(np.int32))
        assert np.random.randint(0, 1 << 30) == rs.randint(0, 1 << 30), "generator state differs after the replay"
        keep = ("idx", "final", "start") + (("scale", "shift", "perm") if train else ()) + (("norm", "trans") if keep_stages else ())
        for k in keep:
            out[f"{tag}_{k}"] = np.stack(res[k])

    def D_rows(pts, idx):
        return pts[idx][:, :3]

    def scanobjectnn(tag, clouds, npoints):
        np.random.seed([SEED, 0, 0])
        rs = np.random.RandomState([SEED, 0, 0])
        res = {k: [] for k in ("final", "scale", "shift", "perm")}
        for pts in clouds:
            pointcloud = pts[:npoints]                                   # ScanObjectNN.__getitem__, :407-412 (train)
            pointcloud = D.translate_pointcloud(pointcloud)
            np.random.shuffle(pointcloud)
            d = numpy_draws(rs, "scanobjectnn", True, pts.shape[0], npoints)
            assert np.array_equal(translate_as_kernel(pts[:npoints], d["scale"], d["shift"])[d["perm"]], pointcloud)
            res["final"].append(pointcloud); res["scale"].append(d["scale"]); res["shift"].append(d["shift"])
            res["perm"].append(d["perm"].astype(np.int32))
        assert np.random.randint(0, 1 << 30) == rs.randint(0, 1 << 30)
        for k in res:
            out[f"{tag}_{k}"] = np.stack(res[k])

    def shapenetpart(tag, clouds, segs, lengths, npoints):
        np.random.seed([SEED, 0, 0])
        rs = np.random.RandomState([SEED, 0, 0])
        res = {k: [] for k in ("final", "seg", "sel")}
        for pts, sg, L in zip(clouds, segs, lengths):
            point_set, s = pts[:L].copy(), sg[:L].copy()                 # ShapeNetPart.__getitem__, :750-755 (first access)
            point_set[:, 0:3] = D.pc_normalize(point_set[:, 0:3])
            choice = np.random.choice(len(s), npoints, replace=True)
            point_set = point_set[choice, :]
            s = s[choice]
            d = numpy_draws(rs, "shapenetpart", False, int(L), npoints)
            assert np.array_equal(d["sel"], choice)
            assert np.array_equal(normalize_as_kernel(pts[:L]), D.pc_normalize(pts[:L]))
            res["final"].append(point_set); res["seg"].append(s.astype(np.int32)); res["sel"].append(choice.astype(np.int32))
        assert np.random.randint(0, 1 << 30) == rs.randint(0, 1 << 30)
        for k in res:
            out[f"{tag}_{k}"] = np.stack(res[k])

    modelnet("mn_train", small, SMALL_M, True, keep_stages=True)
    modelnet("mn_test", small, SMALL_M, False, keep_stages=False)
    modelnet("mnbig_train", big, BIG_M, True, keep_stages=False)
    scanobjectnn("so_train", small, SMALL_M)                             # (the test split is small[:, :npoints] itself)
    shapenetpart("sp", small, seg, PART_LENGTHS, SMALL_M)                # (ShapeNetPart draws the same way in both splits)
    path = os.path.join(HERE, "g_datapipe.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
