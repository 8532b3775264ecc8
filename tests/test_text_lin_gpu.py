"""GPU: the 16-bit form of the text-lin kernel (csrc/text_lin.hip, ops.text_lin16): the four linears of the text tower's
attention half on the mixed mode's 16-bit operands, rows stationary and the weight streamed.

Bounds.  A product of two f16 (11 + 11 significand bits) or two bf16 values is exact in fp32, so the only error of an fp32 result is
the fp32 accumulation (norm-relative < 1e-5 against fp64 here); a 16-bit result is that value rounded once, so it is within one unit
in the last place of the format of the fp64 value.  Against ops.gemm on the same operands: the tile GEMM multiplies on 32x32x16
MFMAs, this kernel on 16x16x32 ones, so the fp32 sums are formed in another order and are not bit-identical -- fp32 results agree to
the accumulation bound, 16-bit results to one unit in the last place (a rounding boundary between the two sums)."""
from types import SimpleNamespace

import pytest
import torch

from ppt_amd import weights as W

pytestmark = pytest.mark.gpu

CASES = [(817, 1536, 512, "bias"), (817, 512, 512, "bias+residual"), (817, 512, 512, "plain"), (817, 512, 1536, "chunks"),
         (37, 512, 512, "plain"), (1480, 1536, 512, "bias")]
EPS16 = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}           # one unit in the last place, relative to the value


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ppt_amd import ops as _ops
    return _ops


def _operands(M, N, K, epi, dt):
    g = torch.Generator().manual_seed(M + N + K + (1 if dt == torch.bfloat16 else 0))
    a = torch.randn(M, K, generator=g)
    a[:, ::41] *= 8.0
    a = a.to(dt)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dt)
    b = 0.1 * torch.randn(N, generator=g) if "bias" in epi else None
    r = torch.randn(M, N, generator=g) if "residual" in epi else None
    return a, w, b, r


def _rel(x, y):
    return ((x - y).norm() / y.norm()).item()


def _within_ulp(got, want, dt):
    """every element of the 16-bit `got` is within one unit in the last place of the fp64 `want` (plus an fp32-accumulation floor)"""
    err = (got.double().cpu() - want).abs()
    return bool((err <= EPS16[dt] * want.abs() + 1e-5 * want.abs().max()).all())


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("M,N,K,epi", CASES)
def test_text_lin16_matches_fp64_and_the_tile_gemm(ops, M, N, K, epi, dt):
    a, w, b, r = _operands(M, N, K, epi, dt)
    want = a.double() @ w.double().t() + (b.double() if b is not None else 0) + (r.double() if r is not None else 0)
    ad, wd = a.cuda(), w.cuda()
    bd, rd = (b.cuda() if b is not None else None), (r.cuda() if r is not None else None)
    wt = ops.text_lin_retile16(wd)
    assert wt.numel() == N * K * 2
    if epi == "chunks":                                   # the K = 1536 input gradient: three fp32 partial products
        got = ops.text_lin16(ad, wt)
        assert got.shape == (K // 512, M, N) and got.dtype == torch.float32
        assert _rel(got.double().sum(0).cpu(), want) < 1e-5
        ref = ops.gemm_splitk(ad, wd, K // 512)
        for c in range(K // 512):
            assert _rel(got[c].double(), ref[c].double()) < 1e-5
    elif epi == "bias+residual":                          # out_proj: fp32 through a strided out=
        big = torch.zeros((M, N + 64), dtype=torch.float32, device="cuda")
        got = ops.text_lin16(ad, wt, bias=bd, residual=rd, out=big[:, :N])
        assert got.data_ptr() == big.data_ptr() and float(big[:, N:].abs().max()) == 0.0
        assert _rel(got.double().cpu(), want) < 1e-5
        ref = torch.empty((M, N), dtype=torch.float32, device="cuda")
        ops.gemm(ad, wd, out=ref, bias=bd, residual=rd)
        assert _rel(got.double(), ref.double()) < 1e-5
    else:                                                 # in_proj (bias) / out_proj's input gradient (plain): 16-bit out
        got = ops.text_lin16(ad, wt, bias=bd)
        assert got.shape == (M, N) and got.dtype == dt
        assert torch.isfinite(got).all()
        assert _within_ulp(got, want, dt)
        ref = ops.gemm(ad, wd, out_dtype=dt, bias=bd)
        diff = (got.float() - ref.float()).abs()
        assert bool((diff <= EPS16[dt] * ref.float().abs() + 1e-5 * float(ref.float().abs().max())).all())
        assert _rel(got.double(), ref.double()) < EPS16[dt]
    # bit-reproducible run to run
    again = ops.text_lin16(ad, wt, bias=bd, residual=rd, out=torch.empty_like(got)) if epi == "bias+residual" else ops.text_lin16(ad, wt, bias=bd)
    assert torch.equal(again, got)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("M,N,K,epi", [c for c in CASES if c[3] in ("bias", "plain")])
def test_text_lin16_overflow_is_inf_not_saturated(ops, M, N, K, epi, dt):
    """a product beyond the 16-bit format's range leaves as +-inf, as ops.gemm's rounding makes it (ppt_amd/health.py reads an inf
    in the half activations as overflow): never a saturated finite value"""
    a, w, b, _ = _operands(M, N, K, epi, dt)
    huge = 1.0e4 if dt == torch.float16 else 1.0e38           # x 8 ones: beyond 65 504 / beyond fp32 itself
    a[M - 1] = 0.0
    a[M - 1, :8] = huge
    w[0] = 1.0
    w[1] = -1.0
    ad, wd = a.cuda(), w.cuda()
    bd = b.cuda() if b is not None else None
    got = ops.text_lin16(ad, ops.text_lin_retile16(wd), bias=bd)
    assert got[M - 1, 0].item() == float("inf") and got[M - 1, 1].item() == float("-inf")
    fin = got[torch.isfinite(got)].float().abs()
    assert float(fin.max()) <= torch.finfo(dt).max
    ref = ops.gemm(ad, wd, out_dtype=dt, bias=bd)
    assert torch.equal(torch.isinf(got), torch.isinf(ref)) and torch.equal(got[torch.isinf(got)], ref[torch.isinf(ref)])


def test_text_lin16_rejects_what_it_does_not_support(ops):
    a = torch.zeros((64, 512), dtype=torch.float16, device="cuda")
    wt = ops.text_lin_retile16(torch.zeros((512, 512), dtype=torch.float16, device="cuda"))
    with pytest.raises(Exception):
        ops.text_lin16(a.to(torch.bfloat16), wt)            # operand dtype other than the copy's
    with pytest.raises(Exception):
        ops.text_lin_retile16(torch.zeros((512, 384), dtype=torch.float16, device="cuda"))   # K not a multiple of 512


def _c2_model(precision):
    from ppt_amd.models import ULIP_models as M
    args = SimpleNamespace(classnames=M.dataset_classnames("modelnet40"), template_init='', class_name_position='middle',
                           num_learnable_prompt_tokens=32, gpu=0, task='cls', head_type=0, evaluate_3d=False, ulip2=False,
                           synthetic_weights=True)
    m = M.ULIP_PointBERT(args)
    m.load_state_dict(W.ulip_pointbert_state_dict(seed=0), strict=False)
    m.prompt_learner.embedding = W.synth_prompt_embedding_from_tokens(m.tokenized_prompts, seed=0)
    m.cuda().set_precision(precision)
    m.overlap_text_tower = False
    return m


def test_mixed16_train_step_text_lin16_on_and_off():
    """the mixed16 C2-shaped step (head 0, ModelNet40 prompts: 817 prefix-shared rows) with the attention half's linears on the
    text-lin kernel (PPT_TEXT_LIN_SPLIT, default) and on the tile GEMMs: text features, loss and the token gradient within the bounds
    of test_text_tower_fused_paths_match_the_unfused_tower; the kernel actually runs in the first and not in the second."""
    from ppt_amd import engine, ops
    from ppt_amd.train import Trainer
    pc, start = W.synth_clouds(4, 1024, seed=77)
    labels = torch.tensor([1, 7, 30, 12]).cuda()
    res, calls = {}, {}
    saved, real = engine.TEXT_LIN_SPLIT, ops.text_lin16
    count = [0]

    def counted(*a, **k):
        count[0] += 1
        return real(*a, **k)
    try:
        ops.text_lin16 = counted
        for on in (False, True):
            engine.TEXT_LIN_SPLIT = on
            count[0] = 0
            m = _c2_model(torch.bfloat16)
            m.train()
            m.point_encoder.fps_start = torch.from_numpy(start).cuda()
            m.point_encoder.drop_path_factors = torch.ones(12, 2, 4)
            tr = Trainer(m, lr=3e-3, distributed=False)
            te = m._text_raw().detach().float().cpu()
            loss, _ = tr.step(torch.from_numpy(pc).cuda(), labels)
            tr.finish()
            torch.cuda.synchronize()
            calls[on] = count[0]
            res[on] = (te, loss.item(), m.prompt_learner.learnable_tokens.grad.detach().cpu().clone())
    finally:
        engine.TEXT_LIN_SPLIT = saved
        ops.text_lin16 = real
    assert calls[False] == 0 and calls[True] >= 4 * 12, calls
    a, b = res[False], res[True]
    assert ((a[0] - b[0]).norm() / a[0].norm()).item() < 5e-3
    assert abs(a[1] - b[1]) < 2e-2 * abs(a[1])
    assert ((a[2] - b[2]).norm() / a[2].norm()).item() < 8e-2
    cos = (a[2].flatten() @ b[2].flatten() / (a[2].norm() * b[2].norm())).item()
    assert cos > 0.995, cos
