#!/usr/bin/env python3
"""Generate tests/golden/g_augment.npz: what the UPSTREAM REFERENCE's augmentation functions and ShapeNet item (data/dataset_3d.py,
imported through tests/golden/ref_import.py) make of seeded synthetic clouds, for csrc/cloud_augment.hip, ppt_amd/data/augment.py and
the loader's "shapenet55" recipe.  Build container only; only arrays are stored.

    python tests/golden/make_golden_augment.py

The clouds are g_datapipe.npz's `small` (4 x 2048 rows, moved off the unit sphere by make_golden_datapipe.py), so the tests need no
second copy of them.  Stored:
  c{n}_*    ShapeNet.__getitem__ (:581-603) on the global numpy generator seeded with [SEED, 0, 0], sample after sample, for n = 3,
            64, 257 (4 samples each) and 512 (1 sample): FPS 2048 -> n, pc_norm, and the cloud after random_point_dropout,
            random_scale_point_cloud, shift_point_cloud, rotate_perturbation_point_cloud, rotate_point_cloud, the height column;
            every draw (`c{n}_d_*`); `c{n}_probe`, the generator's next randint(0, 2^30) after the last sample
  rs_*      the same item for clouds of exactly n = 64 rows: random_sample (:571-574) with its persistent permutation
  jit_*     jitter_point_cloud on two clouds (float64, as the reference returns it), generator seeded with [SEED, 1, 0]
  so_aug    ScanObjectNN's train item (:407-412, as make_golden_datapipe.py runs it) followed by rotate_point_cloud and
            jitter_point_cloud, per sample, on the generator seeded with [SEED, 0, 0]: what the loader's recipe "scanobjectnn" with
            augment=("rotate", "jitter") replays.  Sample 0's recipe output is g_datapipe.npz's; the later ones differ from it because
            the augmentations' draws now lie between the samples
  numpy     the numpy version string (the arithmetic is numpy >= 2's: a float32 array times an np.float64 scalar is a float64 product)
While generating, the script asserts that
  * replaying the documented draw order (ppt_amd.data.numpy_draws) on a RandomState with the same seed reproduces every draw and
    leaves the generator in the same state, and
  * the kernel-order restatement of every stage (tests/augment_ref.py) reproduces the reference's output from the reference's input:
    bit for bit for dropout, scale, shift, jitter and the height column; for the two rotations, whose np.dot runs a BLAS dgemm
    with its own summation, within one float32 ulp of the row's largest coordinate with at least 99.9 % of the elements bit-equal
    (the share actually found is printed).
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import ref_import as R                                     # noqa: E402
import augment_ref as A                                    # noqa: E402
from ppt_amd.data import numpy_draws, pc_normalize         # noqa: E402
from ppt_amd.data.augment import host_stage_draws          # noqa: E402
from oracle import oracle as O                             # noqa: E402

COUNTS = {3: 4, 64: 4, 257: 4, 512: 1}
ROTATE_STATS = {"elements": 0, "equal": 0}


def check_rotate(got, want, what):
    """the rotation's criterion (module text)"""
    bound = A.ulp32(np.abs(want).max(axis=1, keepdims=True))
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= bound).all(), what
    ROTATE_STATS["elements"] += want.size
    ROTATE_STATS["equal"] += int((got == want).sum())
    assert (got == want).mean() >= 0.999, (what, (got == want).mean())


def main():
    assert int(np.__version__.split(".")[0]) >= 2, "the fixture pins numpy >= 2 arithmetic (NEP 50 scalar promotion)"
    g = dict(np.load(os.path.join(HERE, "g_datapipe.npz")))
    seed, small = int(g["seed"]), g["small"]
    with R.reference_context():
        import data.dataset_3d as D
    out = {"numpy": np.array(np.__version__), "seed": np.int64(seed)}

    def item(data, use_height=True):
        """ShapeNet.__getitem__ from pc_norm on (:587-603); -> the cloud after every statement"""
        data = D.ShapeNet.pc_norm(None, data)
        res = {"norm": data.copy()}
        data = D.random_point_dropout(data[None, ...]); res["drop"] = data[0].copy()
        data = D.random_scale_point_cloud(data); res["scale"] = data[0].copy()
        data = D.shift_point_cloud(data); res["shift"] = data[0].copy()
        data = D.rotate_perturbation_point_cloud(data); res["pert"] = data[0].copy()
        data = D.rotate_point_cloud(data); res["rot"] = data[0].copy()
        data = data.squeeze()
        height_array = data[:, 1:2] - data[:, 1:2].min()
        res["height"] = np.concatenate((data, height_array), axis=1)[:, 3].copy()
        assert all(v.dtype == np.float32 for v in res.values())
        return res

    def replay(res, norm2, d):
        """the restatement, stage by stage, each from the REFERENCE's input"""
        assert np.array_equal(norm2, res["norm"]), "pc_normalize differs from ShapeNet.pc_norm"
        assert np.array_equal(A.dropout(res["norm"], d["aug_mask"]), res["drop"]), "dropout"
        assert np.array_equal(A.scale(res["drop"], d["aug_scale"]), res["scale"]), "scale"
        assert np.array_equal(A.shift(res["scale"], d["aug_shift"]), res["shift"]), "shift"
        check_rotate(A.rotate(res["shift"], d["aug_perturb"]), res["pert"], "rotate_perturbation")
        check_rotate(A.rotate(res["pert"], d["aug_rotate"]), res["rot"], "rotate")
        assert np.array_equal(A.height(res["rot"])[:, 3], res["height"]), "height"
        stages = [("dropout", d["aug_mask"]), ("scale", d["aug_scale"]), ("shift", d["aug_shift"]), ("rotate", d["aug_perturb"]),
                  ("rotate", d["aug_rotate"])]
        check_rotate(A.chain(res["norm"], stages), res["rot"], "the whole chain")

    draw_keys = ("ratio", "u", "scale", "shift", "angles", "perturb", "angle", "rotate")
    for n, count in COUNTS.items():
        np.random.seed([seed, 0, 0])
        rs = np.random.RandomState([seed, 0, 0])
        acc = {}
        for pts in small[:count]:
            res = item(D.farthest_point_sample(pts, n))
            d = numpy_draws(rs, "shapenet55", True, pts.shape[0], n)
            rows, idx = O.dataset_farthest_point_sample(pts, n, d["start"])
            replay(res, pc_normalize(rows[:, :3]), d)
            res["d_start"] = np.int64(d["start"])
            res.update({"d_" + k: np.asarray(d["aug_" + k]) for k in draw_keys})
            for k, v in res.items():
                acc.setdefault(k, []).append(v)
        probe = np.random.randint(0, 1 << 30)
        assert probe == rs.randint(0, 1 << 30), "generator state differs after the replay"
        out[f"c{n}_probe"] = np.int64(probe)
        for k, v in acc.items():
            out[f"c{n}_{k}"] = np.stack(v)

    # random_sample: clouds of exactly npoints rows, one persistent permutation (ShapeNet.permutation, :545)
    n = 64
    np.random.seed([seed, 0, 0])
    rs = np.random.RandomState([seed, 0, 0])
    ref_self, mine = SimpleNamespace(permutation=np.arange(n)), np.arange(n)
    sels, finals = [], []
    for pts in small[:, :n]:
        res = item(D.ShapeNet.random_sample(ref_self, pts, n))
        d = numpy_draws(rs, "shapenet55", True, n, n, permutation=mine)
        assert np.array_equal(mine, ref_self.permutation) and np.array_equal(d["sel"], mine)
        replay(res, pc_normalize(pts[d["sel"]]), d)
        sels.append(d["sel"].astype(np.int32)); finals.append(res["rot"])
    assert np.random.randint(0, 1 << 30) == rs.randint(0, 1 << 30)
    out["rs_sel"], out["rs_final"] = np.stack(sels), np.stack(finals)

    # jitter (float64 out of the reference)
    x = out["c64_norm"][:2].copy()
    np.random.seed([seed, 1, 0])
    rs = np.random.RandomState([seed, 1, 0])
    jit = D.jitter_point_cloud(x)
    noise = host_stage_draws(rs, "jitter", 2, 64)["noise"]
    assert jit.dtype == np.float64 and np.array_equal(noise + x, jit) and np.random.randint(0, 1 << 30) == rs.randint(0, 1 << 30)
    assert all(np.array_equal(A.jitter(x[b], noise[b]), jit[b].astype(np.float32)) for b in range(2))
    out["jit_noise"], out["jit_out"] = noise, jit

    # recipe "scanobjectnn" + augment=("rotate", "jitter"): the recipe's draws, then the two functions on its output, per sample
    np.random.seed([seed, 0, 0])
    rs = np.random.RandomState([seed, 0, 0])
    m = g["so_train_final"].shape[1]
    finals = []
    for i in range(4):
        pointcloud = D.translate_pointcloud(small[i][:m])                # ScanObjectNN.__getitem__, :407-412 (train)
        np.random.shuffle(pointcloud)
        if i == 0:                                                       # (later samples see a generator the augmentations advanced)
            assert np.array_equal(pointcloud, g["so_train_final"][0])
        pc = pointcloud[None].copy()
        rot = D.rotate_point_cloud(pc)
        fin = D.jitter_point_cloud(rot)
        d = numpy_draws(rs, "scanobjectnn", True, small.shape[1], m, augment=("rotate", "jitter"))
        assert np.array_equal(A.affine(small[i][:m], d["scale"], d["shift"])[d["perm"]], pc[0])
        check_rotate(A.rotate(pc[0], d["aug_rotate"]), rot[0], "so rotate")
        assert np.array_equal(A.jitter(rot[0], d["aug_noise"]), fin[0].astype(np.float32))
        finals.append(fin[0].astype(np.float32))
    assert np.random.randint(0, 1 << 30) == rs.randint(0, 1 << 30)
    out["so_aug_final"] = np.stack(finals)

    path = os.path.join(HERE, "g_augment.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays; rotation elements bit-equal to np.dot:",
          f"{ROTATE_STATS['equal']}/{ROTATE_STATS['elements']}")


if __name__ == "__main__":
    main()
