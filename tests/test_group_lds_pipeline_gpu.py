"""The request ring of csrc/group_lds.h (mini-PointNet conv3 and conv4) at its ends.

A persistent workgroup of that kernel keeps DIST groups of LDS-DMA requests in flight in a ring of DIST + 1 LDS images (conv3: 3
ahead in 4 slots, conv4: 2 ahead in 3), waits for them with counted vmcnt waits and clamps the prefetch index at the last group.  A
ring goes wrong at its ends, so these cases make workgroups take FEW and UNEQUAL numbers of groups:

  * under ops.persistent_occupancy(10), the smallest share the setter accepts, the grid is max(8, 10 % of the CUs) workgroups
    (`GRID_MIN`; 25 on the 256 CUs of an MI355X).  Group counts 1, 2, 7, 8, 9, 16, 17, 24, 25, 33, 41: fewer groups than
    workgroups, exactly as many, one more, and up to two per workgroup where the grid is 25 (up to six where it is 8).
  * counts stated in units of that grid, k * GRID_MIN + d: every workgroup takes k groups and the first d one more (d < 0: the
    last -d one fewer) -- 1 to 7 groups per workgroup, neighbours differing by one: ring prologue alone (fewer groups than
    slots), steady state, the wrap of both rings (more groups than slots) and the drain, whatever the CU count.
  * at the default occupancy (one workgroup per CU): 300 groups and 2 * CUs + 1.

Every form: conv3 with statistics + store, store only, statistics only, conv4; both 16-bit formats.  y3 and tok must be
torch.equal to the ops.gemm references tests/test_kernels_gpu.py uses (group_add + col_stats; A_AFFINE_RELU + pool_max), the
partials within that file's 1e-4 / 1e-3 of the reference's and bit-equal between the statistics pass and the storing pass.  Every
output is allocated with sentinel-filled guard rows behind it, which must stay untouched, and the same input under different
occupancies (different grids, other groups per workgroup) gives the same bits."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4                                   # guard rows behind every output
SENT16, SENT32 = -1234.0, 12345.0           # what they hold (exact in both 16-bit formats' range, never a result of these inputs)
MIN_SHARE = 10                              # the smallest percentage ppt_set_persistent_occupancy accepts

FIXED = (1, 2, 7, 8, 9, 16, 17, 24, 25, 33, 41)
IN_GRIDS = ((1, 1), (2, -1), (3, 1), (4, 0), (6, 1))      # (k, d): k * GRID_MIN + d groups
FORMATS = (torch.float16, torch.bfloat16)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ppt_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _grid_min(cus):
    return max(8, cus * MIN_SHARE // 100)


_CASES = {}


def _case(ops, T, groups):
    """operands of `groups` groups and the ops.gemm references, computed once per (format, count) and never written again"""
    key = (T, groups)
    if key not in _CASES:
        g = torch.Generator(device="cuda").manual_seed(1000 + groups)
        M = 32 * groups
        c = {"groups": groups, "T": T}
        c["A3"] = torch.randn(M, 256, device="cuda", generator=g).to(T)
        c["w3"] = (torch.randn(512, 256, device="cuda", generator=g) / 16).to(T)
        c["gt"] = torch.randn(groups, 512, device="cuda", generator=g)
        c["st_ref"] = (torch.empty((groups, 512), device="cuda"), torch.empty((groups, 512), device="cuda"))
        c["y_ref"] = ops.gemm(c["A3"], c["w3"], out_dtype=T, group_add=c["gt"], group_rows=32, col_stats=c["st_ref"])
        c["A4"] = torch.randn(M, 512, device="cuda", generator=g).to(T)
        c["sc"] = 1.0 + 0.2 * torch.randn(512, device="cuda", generator=g)
        c["sh"] = 0.2 * torch.randn(512, device="cuda", generator=g)
        c["w4"] = (torch.randn(256, 512, device="cuda", generator=g) / 512 ** 0.5).to(T)
        c["b4"] = torch.randn(256, device="cuda", generator=g) * 0.1
        c["tok_ref"] = torch.empty((groups, 256), dtype=T, device="cuda")
        ops.gemm(c["A4"], c["w4"], a_mode=ops.A_AFFINE_RELU, a_scale=c["sc"], a_shift=c["sh"], bias=c["b4"], pool_max=c["tok_ref"],
                 want_out=False)
        _CASES[key] = c
    return _CASES[key]


def _guarded(rows, cols, dtype):
    """[rows + GUARD, cols] filled with the sentinel -> (the whole buffer, its first `rows` rows)"""
    buf = torch.full((rows + GUARD, cols), SENT32 if dtype == torch.float32 else SENT16, dtype=dtype, device="cuda")
    return buf, buf[:rows]


def _guards_untouched(*bufs):
    for buf in bufs:
        tail = buf[-GUARD:]
        assert torch.equal(tail, torch.full_like(tail, SENT32 if buf.dtype == torch.float32 else SENT16)), "rows behind an output were written"


def _conv3(ops, c, stats, store):
    """one launch of ppt_mini_pointnet_conv3_half into guarded outputs -> (y3 or None, part_sum or None, part_m2 or None)"""
    groups, T = c["groups"], c["T"]
    bufs, y, ps, pm = [], None, None, None
    if store:
        b, y = _guarded(32 * groups, 512, T)
        bufs.append(b)
    if stats:
        b, ps = _guarded(groups, 512, torch.float32)
        bufs.append(b)
        b, pm = _guarded(groups, 512, torch.float32)
        bufs.append(b)
    ops._lib.check(ops._lib.lib().ppt_mini_pointnet_conv3_half(ops._p(c["A3"]), 32 * groups, 256, ops._p(c["w3"]), ops._p(c["gt"]), 512, ops._p(y),
                                                               ops._p(ps), ops._p(pm), ops.dtype_code(T), ops._stream()),
                   "ppt_mini_pointnet_conv3_half")
    _guards_untouched(*bufs)
    return y, ps, pm


def _conv4(ops, c):
    """one launch of ppt_mini_pointnet_conv4_half into a guarded output -> tok"""
    groups, T = c["groups"], c["T"]
    buf, tok = _guarded(groups, 256, T)
    ops._lib.check(ops._lib.lib().ppt_mini_pointnet_conv4_half(ops._p(c["A4"]), 32 * groups, 512, ops._p(c["sc"]), ops._p(c["sh"]), ops._p(c["w4"]),
                                                               ops._p(c["b4"]), 256, ops._p(tok), ops.dtype_code(T), ops._stream()),
                   "ppt_mini_pointnet_conv4_half")
    _guards_untouched(buf)
    return tok


def _all_forms(ops, c):
    """every instantiation on one case -> {name: tensor}"""
    y, ps, pm = _conv3(ops, c, stats=True, store=True)
    y_eval, _, _ = _conv3(ops, c, stats=False, store=True)
    _, ps_only, pm_only = _conv3(ops, c, stats=True, store=False)
    return {"y": y, "ps": ps, "pm": pm, "y_eval": y_eval, "ps_only": ps_only, "pm_only": pm_only, "tok": _conv4(ops, c)}


def _check(ops, T, groups, share):
    c = _case(ops, T, groups)
    with ops.persistent_occupancy(share) if share < 100 else contextlib.nullcontext():
        out = _all_forms(ops, c)
    assert torch.equal(out["y"], c["y_ref"]), "conv3, statistics + store: y3"
    assert torch.equal(out["y_eval"], c["y_ref"]), "conv3, store only: y3"
    assert torch.equal(out["tok"], c["tok_ref"]), "conv4: tok"
    rs, rm = c["st_ref"]
    assert (out["ps"] - rs).abs().max().item() < 1e-4 * max(1.0, rs.abs().max().item())
    assert (out["pm"] - rm).abs().max().item() < 1e-3 * max(1.0, rm.abs().max().item())
    assert torch.equal(out["ps_only"], out["ps"]) and torch.equal(out["pm_only"], out["pm"]), "statistics pass vs storing pass"
    return out


@pytest.mark.parametrize("T", FORMATS, ids=lambda t: str(t).split(".")[-1])
@pytest.mark.parametrize("groups", FIXED)
def test_few_groups_on_the_smallest_grid(ops, T, groups):
    """the smallest grid the occupancy setter gives; from fewer groups than workgroups to a few per workgroup"""
    _check(ops, T, groups, MIN_SHARE)


@pytest.mark.parametrize("T", FORMATS, ids=lambda t: str(t).split(".")[-1])
@pytest.mark.parametrize("k,d", IN_GRIDS, ids=lambda v: str(v))
def test_unequal_shares_of_the_smallest_grid(ops, cus, T, k, d):
    """k * GRID_MIN + d groups: every workgroup takes k groups or one more / one fewer -- 1 to 7 groups per workgroup"""
    _check(ops, T, k * _grid_min(cus) + d, MIN_SHARE)


@pytest.mark.parametrize("T", FORMATS, ids=lambda t: str(t).split(".")[-1])
@pytest.mark.parametrize("which", ["300", "2xgrid+1"])
def test_default_occupancy(ops, cus, T, which):
    """one workgroup per CU: 300 groups (one or two per workgroup) and 2 * CUs + 1 (two, and one workgroup three)"""
    _check(ops, T, 300 if which == "300" else 2 * cus + 1, 100)


@pytest.mark.parametrize("T", FORMATS, ids=lambda t: str(t).split(".")[-1])
@pytest.mark.parametrize("which", ["41", "6xgridmin+1", "2xgrid+1"])
def test_results_do_not_depend_on_the_grid(ops, cus, T, which):
    """the same input under three occupancies -- three grids, other groups per workgroup, other ring positions: the same bits"""
    groups = {"41": 41, "6xgridmin+1": 6 * _grid_min(cus) + 1, "2xgrid+1": 2 * cus + 1}[which]
    outs = [_check(ops, T, groups, share) for share in (MIN_SHARE, 30, 100)]
    for other in outs[1:]:
        for name, t in outs[0].items():
            assert torch.equal(t, other[name]), name
