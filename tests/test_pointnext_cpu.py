"""CPU: the PointNeXt-S surface (factory, module tree, weight spec, use_height) and the restatement the GPU tests are measured
against (tests/pointnext_ref.py) held to the reference outputs of tests/golden/g_pointnext.npz."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pointnext_ref as P
from ppt_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("eval_n1024", "eval_n200", "train", "train_b3")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g_pointnext.npz")))


def case_inputs(g, tag):
    """-> (pc4 [B,N,4] float32 array, train, drop masks | None) of a golden case."""
    if tag == "eval_n1024":
        return P.cloud_height(W.synth_clouds(2, 1024, seed=101)[0]), False, None
    if tag == "eval_n200":
        return g["pc_n200"], False, None
    if tag == "train_b3":                                  # 3 x 12 = 36 rows in the GroupAll stage: a ragged 32-row BatchNorm partial
        return g["pc_n200"], True, (g["drop1"][:3], g["drop2"][:3])
    return g["pc_train"], True, (g["drop1"], g["drop2"])


@pytest.mark.parametrize("tag", CASES)
def test_fp32_restatement_equals_the_reference(g, tag):
    """Separates the fixture from the restatement's bugs: in fp32 it reproduces the reference within 4 x the reference's own distance
    from the fp64 restatement (outputs, and for the train case every updated running statistic)."""
    sd = W.synth_state_dict(W.pointnext_spec(prefix=""), seed=0)
    pc, train, masks = case_inputs(g, tag)
    out, stats, idx = P.forward(sd, pc, train, masks, dtype=torch.float32)
    ref, bound = g[tag], 4 * float(g["ref_err_" + tag])
    err = np.abs(out.numpy() - ref).max() / np.abs(ref).max()
    print(f"pointnext restatement {tag}: err / max|ref| {err:.3g} (bound {bound:.3g})")
    assert err <= bound
    if train:
        assert len(stats) == 2 * 12
        for k, v in stats.items():
            r = g[f"stat.{tag}.{k}"]
            assert np.abs(v.numpy() - r).max() / np.abs(r).max() <= bound, k
    if tag == "eval_n200":
        for i, (ci, ni) in enumerate(idx):
            assert np.array_equal(ci, g[f"fps{i}"]) and np.array_equal(ni, g[f"ball{i}"])
        assert 1 not in idx[0][1][2, 0] and idx[0][0][2, 0] == 0          # the boundary point is outside its centre's ball


def test_factory_names_shapes_and_frozen_set(g):
    import models.ULIP_models as models
    a = SimpleNamespace(classnames=models.dataset_classnames("modelnet40"), template_init='', class_name_position='middle',
                        num_learnable_prompt_tokens=32, gpu=0, task='cls', head_type=0, evaluate_3d=False, ulip2=False,
                        synthetic_weights=True)
    m = models.ULIP_PN_NEXT(a)
    enc = m.point_encoder.state_dict()
    assert list(enc.keys()) == [str(k) for k in g["keys"]]
    assert [str(tuple(v.shape)) for v in enc.values()] == [str(s) for s in g["shapes"]]
    assert list(enc.keys()) == [k for k, _ in W.pointnext_spec(prefix="")]
    spec = dict(W.ulip_spec(256, True) + W.pointnext_spec())
    sd = m.state_dict()
    assert set(sd) == set(spec) and all(tuple(sd[k].shape) == tuple(v) for k, v in spec.items())
    assert set(W.ulip_pn_next_state_dict(seed=0)) == set(spec) - {"token_embedding.weight"}
    assert [n for n, p in m.named_parameters() if p.requires_grad] == ["prompt_learner.learnable_tokens"]
    assert m.pc_projection.shape[0] == 256


def test_encoder_has_the_yaml_parameter_count():
    from models.pointnext.pointnext import PointNEXT
    assert sum(p.numel() for p in PointNEXT().parameters()) == 1363264


def test_three_channel_input_raises_and_names_use_height():
    from ppt_amd.models.pointnext.pointnext import PointNEXT
    with pytest.raises(ValueError, match="use_height"):
        PointNEXT()(torch.zeros(2, 64, 3))


def test_use_height_on_the_host_is_the_numpy_expression():
    """DeviceBatchLoader has no CPU path: what runs here is the host branch of the helper it calls, `device_loader.add_height`, which
    this test alone reaches.  The loader itself with use_height=True is covered on the device
    (tests/test_pointnext_gpu.py::test_loader_use_height_adds_the_column_to_the_finished_cloud)."""
    from ppt_amd.data.device_loader import add_height
    pc, _ = W.synth_clouds(3, 77, seed=5)
    pc[1, 9, 1] = pc[1, :, 1].min()                       # the minimum occurs twice
    want = np.stack([np.concatenate((c, c[:, 1:2] - c[:, 1:2].min()), axis=1) for c in pc])      # dataset_3d.py:311-314 per cloud
    got = add_height(torch.from_numpy(pc))
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want) and np.array_equal(P.cloud_height(pc), want)
