"""CPU: the host side of ragged part segmentation -- lengths validation (engine.cloud_lengths with total_rows), finalize_partseg
on ragged batch sizes, the float64 reference helper against tests/decoder_ref.py, and the paths that still refuse lengths."""
import numpy as np
import pytest
import torch

import decoder_ref as D
import partseg_ragged_ref as R
import validate_ref as V


def test_lengths_validation():
    from ppt_amd import engine
    cpu = torch.device("cpu")
    L, rows = engine.cloud_lengths([700, 513, 300], 3, 704, cpu, least=32, total_rows=None)
    assert L.dtype == torch.int32 and L.tolist() == [700, 513, 300] and rows == 1513
    assert engine.cloud_lengths(np.array([700, 513, 300]), 3, 704, cpu, least=32).tolist() == [700, 513, 300]     # no total asked: as before
    assert engine.cloud_lengths([700, 513, 300], 3, 704, cpu, total_rows=1513)[1] == 1513
    for bad in ([700, 513], [700, 513, 705], [700, 513, 31], [700.0, 513.0, 300.0]):
        with pytest.raises(ValueError, match="lengths"):
            engine.cloud_lengths(bad, 3, 704, cpu, least=32, total_rows=None)
    with pytest.raises(ValueError, match="total_rows"):
        engine.cloud_lengths([700, 513, 300], 3, 704, cpu, least=32, total_rows=1512)


def test_device_lengths_of_the_wrong_dtype_or_shape_are_refused():
    """the device-tensor branch looks at dtype and shape only; a meta tensor stands in for one (is_cuda is what selects the branch)"""
    from ppt_amd import engine

    class FakeCuda(torch.Tensor):
        is_cuda = True
    for t in (torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)):
        with pytest.raises(ValueError, match="int32"):
            engine.cloud_lengths(t.as_subclass(FakeCuda), 3, 704, torch.device("cpu"), total_rows=None)
    with pytest.raises(ValueError, match="total_rows"):
        engine.cloud_lengths(torch.zeros(3, dtype=torch.int32).as_subclass(FakeCuda), 3, 704, torch.device("cpu"), least=32, total_rows=95)


def _records(sizes, seed):
    """records of clouds with the given point counts (one category each, random labels and predictions)"""
    c2p = V.category2part()
    g = torch.Generator().manual_seed(seed)
    cats = list(c2p.values())
    recs = []
    for i, n in enumerate(sizes):
        parts = cats[(3 * i + seed) % len(cats)]
        labels = torch.tensor(parts)[torch.randint(0, len(parts), (1, n), generator=g)]
        recs.append(V.partseg_records(torch.randn(1, n, 50, generator=g) * 3, labels, c2p, 0.2))
    return torch.cat(recs).numpy(), c2p


def test_finalize_partseg_with_ragged_batches():
    """two ragged batches (B, Nmax, R) against the same clouds listed one per batch at their own length: the per-cloud IoU figures
    are the same bits; acc and loss are the batch-weighted means with R as the batch's point count"""
    from ppt_amd import evaluate
    sizes = [700, 513, 300, 704, 65, 1]
    rec, c2p = _records(sizes, seed=2)
    got = evaluate.finalize_partseg(rec, [(4, 704, sum(sizes[:4])), (2, 704, sum(sizes[4:]))], c2p)
    lone = evaluate.finalize_partseg(rec, [(1, n) for n in sizes], c2p)
    assert got["n"] == lone["n"] == 6 and got["category_counts"] == lone["category_counts"]
    assert V.same_bits(got["mean_inst_iou"], lone["mean_inst_iou"]) and V.same_bits(got["mean_class_iou"], lone["mean_class_iou"])
    assert V.same_bits(list(got["category_ious"].values()), list(lone["category_ious"].values()))
    correct = rec[:, 2].astype(np.int64)
    loss = rec[:, 4].copy().view(np.float32).astype(np.float64)
    acc = ((torch.tensor(int(correct[:4].sum())) / sum(sizes[:4])).item() * 4 + (torch.tensor(int(correct[4:].sum())) / sum(sizes[4:])).item() * 2) / 6
    want_loss = (loss[:4].sum() / sum(sizes[:4]) * 4 + loss[4:].sum() / sum(sizes[4:]) * 2) / 6
    assert got["acc"] == acc and abs(got["loss"] - want_loss) <= 1e-12 * want_loss
    # a uniform batch listed with R = B * N is the uniform batch
    rec_u, _ = _records([64, 64, 64], seed=5)
    a, b = evaluate.finalize_partseg(rec_u, [(3, 64)], c2p), evaluate.finalize_partseg(rec_u, [(3, 64, 192)], c2p)
    assert a["acc"] == b["acc"] and a["loss"] == b["loss"]


@pytest.mark.parametrize("training", [True, False])
def test_the_float64_helper_equals_decoder_ref_on_a_uniform_case(training):
    """partseg_ragged_ref's packed feature propagation, fed a uniform batch, against decoder_ref.fp_exact (same inputs; the helper
    finds its own 3 neighbours with cdist in float64, decoder_ref takes the case's).  The case carries its distances ROUNDED TO
    FP32 (decoder_ref.knn), the helper keeps them in float64: a relative 2^-24 = 6e-8 per distance, twice that per normalised
    weight, carried through two conv + BatchNorm layers whose gains are O(1) -- bound 1e-6 of the output's scale (everything else
    on both sides is float64, 1e-15)."""
    c = D.BY_ID["fp-m640"]
    inp = D.inputs(c)
    sd = {}
    for j, lay in enumerate(inp["layers"]):
        sd.update({f"p.mlp_convs.{j}.weight": lay.W, f"p.mlp_convs.{j}.bias": lay.b, f"p.mlp_bns.{j}.weight": lay.gamma,
                   f"p.mlp_bns.{j}.bias": lay.beta, f"p.mlp_bns.{j}.running_mean": lay.rm, f"p.mlp_bns.{j}.running_var": lay.rv})
    idx, w = R.three_nn_f64(inp["xyz1"][0], inp["xyz2"][0])
    assert torch.equal(idx, inp["idx"][0])
    got = R.fp_exact_rows(sd, "p.", inp["xyz1"], inp["xyz2"], inp["p1"], inp["p2"], training)
    want = D.fp_exact(inp, training)[0]["out"].detach()
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-6 * want.abs().max().item()


def test_trainer_and_forward_loss_still_refuse_lengths():
    """the messages are raised before anything touches a device"""
    from ppt_amd.models import ULIP_models as M
    from ppt_amd.train import Trainer
    import inspect
    src = inspect.getsource(M.ULIP_WITH_IMAGE.forward_loss)
    assert "forward_loss takes no lengths" in src
    m = M.ULIP_WITH_IMAGE.__new__(M.ULIP_WITH_IMAGE)
    with pytest.raises(ValueError, match="lengths"):
        M.ULIP_WITH_IMAGE.forward_loss(m, torch.zeros(2, 64, 3), torch.zeros(2, dtype=torch.long), 0.2, lengths=[64, 40])
    tr = Trainer.__new__(Trainer)
    with pytest.raises(ValueError, match="lengths"):
        Trainer.step(tr, torch.zeros(2, 64, 3), torch.zeros(2, dtype=torch.long), lengths=[64, 40])
