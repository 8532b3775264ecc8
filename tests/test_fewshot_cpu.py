"""CPU: the few-shot selection against the reference's recorded draws (tests/golden/g_fewshot.npz, written by
tests/golden/make_golden_fewshot.py), the payload of save_recog_feats, and the host-side argument checks of the nearest-rows
entry points."""
import os
import random

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g_fewshot.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("seed", [0, 3])
@pytest.mark.parametrize("shots", [1, 4, 9])
def test_selection_equals_the_reference(golden, seed, shots):
    """sample where a class has enough items, choices where it falls short (9 shots: four of the seven classes)"""
    from ppt_amd.data.fewshot import fewshot_indices
    got = fewshot_indices(golden["labels"], shots, seed=seed)
    assert got.dtype == np.int64 and got.shape == (7 * shots,)
    assert np.array_equal(got, golden[f"seed{seed}_shots{shots}"])
    # classes in order of first appearance, `shots` of each
    lab = golden["labels"]
    first = list(dict.fromkeys(lab.tolist()))
    assert lab[got].tolist() == [c for c in first for _ in range(shots)]


@pytest.mark.parametrize("seed", [0, 3])
def test_selection_without_repeat(golden, seed):
    from ppt_amd.data.fewshot import fewshot_indices
    got = fewshot_indices(golden["labels"], 9, seed=seed, repeat=False)
    assert np.array_equal(got, golden[f"seed{seed}_shots9_norepeat"])
    assert len(got) < 7 * 9


def test_selection_of_everything_and_from_the_global_stream(golden):
    from ppt_amd.data.fewshot import fewshot_indices
    lab = golden["labels"]
    assert np.array_equal(fewshot_indices(lab, -1), golden["all"])
    assert np.array_equal(fewshot_indices(lab, 0, seed=5), np.arange(50))
    state = random.getstate()
    try:
        random.seed(11)
        got = np.concatenate([fewshot_indices(lab, 4), fewshot_indices(lab, 2)])
    finally:
        random.setstate(state)
    assert np.array_equal(got, golden["global_seed11_shots4_then_2"])
    # a seeded call leaves the global stream alone
    random.seed(11)
    a = random.random()
    random.seed(11)
    fewshot_indices(lab, 4, seed=0)
    assert random.random() == a
    random.setstate(state)


def test_save_recog_feats_payload(tmp_path):
    """the reference's keys and dtypes (save_recog_feats.py:75-78); the float64 values are the fp32 logits exactly"""
    from ppt_amd import analysis
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(5, 3, generator=g) * 7.3
    labels = torch.tensor([2, 0, 1, 1, 2], dtype=torch.int32)
    names = ["chair", "bed", "table", "table", "chair"]
    path = tmp_path / "feats.pt"
    analysis.save_recog_feats(path, logits, labels, names)
    got = torch.load(path, weights_only=False)
    assert set(got) == {"test_feats", "test_labels", "test_names"}
    want = np.array(logits.tolist())                    # what the reference builds: a float64 array from Python floats
    assert got["test_feats"].dtype == np.float64 == want.dtype and got["test_feats"].shape == (5, 3)
    assert np.array_equal(got["test_feats"], want)
    assert np.array_equal(got["test_feats"].astype(np.float32), logits.numpy())
    assert got["test_labels"].dtype == np.int64 == np.array(labels.tolist()).dtype
    assert got["test_labels"].tolist() == labels.tolist()
    assert got["test_names"].dtype == np.array(names).dtype and got["test_names"].tolist() == names
    with pytest.raises(ValueError):
        analysis.save_recog_feats(path, logits, labels, names[:4])


def test_nearest_rows_argument_validation_without_gpu():
    """NULL pointers and non-positive sizes: PPT_EINVAL before any launch; unsupported shapes: workspace size 0"""
    from ppt_amd import _lib, ops
    L = _lib.lib()
    assert L.ppt_nearest_rows_f32(None, 1, None, 4, 1, 4, 1, None, None, None, 0, None) == -1
    assert L.ppt_nearest_rows_workspace_bytes(32, 49408, 512, 10) == 386 * 32 * 10 * 8
    assert L.ppt_nearest_rows_workspace_bytes(64, 2000, 512, 5) > 0            # Q D = 32768: the limit
    assert L.ppt_nearest_rows_workspace_bytes(1, 70, 4, 64) > 0
    assert L.ppt_nearest_rows_workspace_bytes(4, 100, 6, 3) == 0               # D % 4 != 0
    assert L.ppt_nearest_rows_workspace_bytes(4, 100, 8, 65) == 0              # k > 64
    assert L.ppt_nearest_rows_workspace_bytes(4, 10, 8, 11) == 0               # k > V
    assert L.ppt_nearest_rows_workspace_bytes(65, 2000, 512, 5) == 0           # Q D > 32768
    assert L.ppt_nearest_rows_workspace_bytes(0, 100, 8, 3) == 0
    assert ops.nearest_rows_workspace_bytes(32, 49408, 512, 10) == 386 * 32 * 10 * 8
    # pointers that are never dereferenced on the host: sizes and shapes are judged first
    buf = (_lib.c_float * 64)()
    p = _lib.ctypes.cast(buf, _lib.c_void_p)
    assert L.ppt_nearest_rows_f32(p, 0, p, 4, 1, 4, 1, p, p, p, 1 << 20, None) == -1         # Q = 0
    assert L.ppt_nearest_rows_f32(p, 1, p, 2, 1, 4, 1, p, p, p, 1 << 20, None) == -1         # ld < D
    assert L.ppt_nearest_rows_f32(p, 1, p, 8, 4, 6, 1, p, p, p, 1 << 20, None) == -3         # D % 4 != 0
    assert L.ppt_nearest_rows_f32(p, 1, p, 8, 4, 8, 5, p, p, p, 1 << 20, None) == -3         # k > V
    assert L.ppt_nearest_rows_f32(p, 1, p, 8, 4, 8, 2, p, p, p, 8, None) == -1               # workspace too small (or misaligned)


def test_nearest_rows_has_no_cpu_path():
    from ppt_amd import analysis, ops
    q, table = torch.zeros(2, 8), torch.zeros(16, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.nearest_rows(q, table, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        analysis.nearest_tokens(q, table, 3)
    with pytest.raises(ValueError):
        analysis.nearest_tokens(torch.zeros(2, 2, 8), table, 3)
