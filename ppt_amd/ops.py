"""Thin torch-tensor wrappers over the C ABI of libppt_hip.so (include/ppt_hip.h).

PyTorch is plumbing here: it owns device memory (caching allocator) and the stream; every
operation below is ONE call into a hand-written gfx950 kernel.  Tensors must be CUDA(HIP),
contiguous, of the stated dtype; wrappers allocate outputs and raise RuntimeError on any error
code.  There is no CPU path.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_NONE, ACT_QUICKGELU, ACT_RELU, A_AFFINE_RELU, A_CONV1, A_PLAIN,
                   PPT_BF16, PPT_F16, PPT_F32, GemmParams, RowGemmParams)
from . import _lib as _libmod  # noqa: F401

_DT = {torch.float32: PPT_F32, torch.bfloat16: PPT_BF16, torch.float16: PPT_F16}
_TORCH_DT = {PPT_F32: torch.float32, PPT_BF16: torch.bfloat16, PPT_F16: torch.float16}
HALF = (torch.bfloat16, torch.float16)        # the two 16-bit operand formats (same MFMA rate)


class KernelProfiler:
    """Optional per-launch timing with HIP events recorded on the launch stream (used by bench.py for
    the live roofline numbers).  Off by default: `ops.profiler = KernelProfiler()` turns it on."""

    def __init__(self):
        self.records = []          # (name, start_event, end_event, algorithmic work)
        self.kernels = []          # the kernel behind each record (a finer name than the family in `name`)
        self.executed = []         # FLOPs / bytes the launch really performs (differs from the model's where work is shared
                                   # -- the broadcast half of conv3 evaluated once per group -- or recomputed)

    def begin(self, name, work, kernel=None, executed=None):
        """work: the MODEL's algorithmic FLOPs (or bytes) of the layer(s) the launch stands for;
        executed: what the launch itself computes (default: the same)."""
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        self._cur = (name, ev, work, kernel or name, work if executed is None else executed)

    def end(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        name, st, work, kernel, executed = self._cur
        self.records.append((name, st, ev, work))
        self.kernels.append(kernel)
        self.executed.append(executed)

    def by_kernel(self):
        """-> {kernel: dict(family, launches, ms, work, executed)} (call after a device synchronise)."""
        out = {}
        for (name, st, en, work), kernel, ex in zip(self.records, self.kernels, self.executed):
            d = out.setdefault(kernel, dict(family=name, launches=0, ms=0.0, work=0.0, executed=0.0))
            d["launches"] += 1
            d["ms"] += st.elapsed_time(en)
            d["work"] += work
            d["executed"] += ex
        return out

    def summary(self):
        """-> {name: dict(launches, ms, work, executed)} (call after a device synchronise)."""
        out = {}
        for (name, st, en, work), ex in zip(self.records, self.executed):
            d = out.setdefault(name, dict(launches=0, ms=0.0, work=0.0, executed=0.0))
            d["launches"] += 1
            d["ms"] += st.elapsed_time(en)
            d["work"] += work
            d["executed"] += ex
        return out


profiler = None


def dtype_code(t):
    return _DT[t.dtype if isinstance(t, torch.Tensor) else t]


_raw_stream = torch._C._cuda_getCurrentRawStream      # current HIP stream handle without building a Stream object


def _stream():
    return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _chk(t, dtype=None, name="tensor"):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a CUDA/HIP tensor (ppt_amd has no CPU path)")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"{name}: expected {dtype}, got {t.dtype}")


def aligned16(t):
    """t, or a copy of it at a 16-byte aligned address: ppt_gemm refuses statistics / pooling launches whose bias or group_add is
    not (struct ppt_gemm_params), and a state-dict tensor can be a view at any element of a flat buffer"""
    return t if t is None or t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


# ---------------------------------------------------------------------------------------------
def _chk_lengths(lengths, B):
    """lengths of the ragged index kernels: [B] int32 on the device (cloud b = rows 0 .. lengths[b]-1 of its [Nmax, 3] slab)."""
    _chk(lengths, torch.int32, "lengths")
    if tuple(lengths.shape) != (B,):
        raise RuntimeError(f"lengths: expected shape ({B},), got {tuple(lengths.shape)}")


def fps(xyz, M, start, lengths=None):
    """H1.  xyz [B,N,3] f32, start [B] i64 -> (idx [B,M] i64, center [B,M,3] f32).  lengths [B] i32 (device): cloud b is its first
    lengths[b] rows, N is the row stride (ppt_fps_ragged_f32); each cloud's picks are those of that cloud alone."""
    _chk(xyz, torch.float32, "xyz"); _chk(start, torch.int64, "start")
    B, N, _ = xyz.shape
    idx = torch.empty((B, M), dtype=torch.int64, device=xyz.device)
    ctr = torch.empty((B, M, 3), dtype=torch.float32, device=xyz.device)
    if profiler is not None:
        profiler.begin("fps", float(B) * (12 * N + 8 * M))          # algorithmic HBM bytes
    if lengths is None:
        _lib.check(_lib.lib().ppt_fps_f32(_p(xyz), B, N, M, _p(start), _p(idx), _p(ctr), _stream()), "ppt_fps_f32")
    else:
        _chk_lengths(lengths, B)
        _lib.check(_lib.lib().ppt_fps_ragged_f32(_p(xyz), B, N, M, _p(start), _p(lengths), _p(idx), _p(ctr), _stream()),
                   "ppt_fps_ragged_f32")
    if profiler is not None:
        profiler.end()
    return idx, ctr


def cloud_offsets(lengths):
    """lengths [B] i32 (device) -> offsets [B+1] i32: the exclusive prefix sum, cloud b owning packed rows offsets[b] ..
    offsets[b+1]-1 (the layout of every *_packed function below; include/ppt_hip.h)."""
    _chk(lengths, torch.int32, "lengths")
    off = torch.zeros(lengths.numel() + 1, dtype=torch.int32, device=lengths.device)
    off[1:] = torch.cumsum(lengths, 0, dtype=torch.int32)
    return off


def _chk_offsets(offsets, B):
    _chk(offsets, torch.int32, "offsets")
    if tuple(offsets.shape) != (B + 1,):
        raise RuntimeError(f"offsets: expected shape ({B + 1},), got {tuple(offsets.shape)}")


def knn_group(xyz, center, k, want_idx=True, want_nbhd=True, want_dist=False, lengths=None, query_lengths=None,
              query_offsets=None, total_rows=None):
    """H2.  xyz [B,N,3], center [B,G,3] -> (nbr_idx [B,G,k] i64, neighborhood [B,G,k,3] f32[, dist [B,G,k] f32]).
    lengths [B] i32 (device): per-cloud row counts, every one >= k (ppt_knn_group_ragged_f32).
    query_lengths [B] i32 (device): cloud b has query_lengths[b] centres, rows 0 .. of its [G,3] slab; the outputs are then PACKED
    rows, [R,k] / [R,k,3] / [R,k] with R = total_rows = sum(query_lengths) and query_offsets [B+1] i32 their prefix sum (computed
    here when None) -- ppt_knn_group_packed_f32; cloud b's rows are those of knn_group on that cloud's queries alone."""
    _chk(xyz, torch.float32, "xyz"); _chk(center, torch.float32, "center")
    B, N, _ = xyz.shape
    G = center.shape[1]
    if query_lengths is not None:
        _chk_lengths(query_lengths, B)
        if lengths is not None:
            _chk_lengths(lengths, B)
        if query_offsets is None:
            query_offsets = cloud_offsets(query_lengths)
        _chk_offsets(query_offsets, B)
        R = int(total_rows)
        idx = torch.empty((R, k), dtype=torch.int64, device=xyz.device) if want_idx else None
        nb = torch.empty((R, k, 3), dtype=torch.float32, device=xyz.device) if want_nbhd else None
        nd = torch.empty((R, k), dtype=torch.float32, device=xyz.device) if want_dist else None
        if profiler is not None:
            profiler.begin("knn_group_packed", float(B) * 12 * N + float(R) * (12 + 8 * k + 12 * k))
        _lib.check(_lib.lib().ppt_knn_group_packed_f32(_p(xyz), _p(center), B, N, G, k, _p(lengths), _p(query_lengths),
                                                       _p(query_offsets), R, _p(idx), _p(nb), _p(nd), _stream()),
                   "ppt_knn_group_packed_f32")
        if profiler is not None:
            profiler.end()
        return (idx, nb, nd) if want_dist else (idx, nb)
    idx = torch.empty((B, G, k), dtype=torch.int64, device=xyz.device) if want_idx else None
    nb = torch.empty((B, G, k, 3), dtype=torch.float32, device=xyz.device) if want_nbhd else None
    if profiler is not None:
        profiler.begin("knn_group", float(B) * (12 * N + 12 * G + 8 * G * k + 12 * G * k))
    nd = torch.empty((B, G, k), dtype=torch.float32, device=xyz.device) if want_dist else None
    if lengths is None:
        _lib.check(_lib.lib().ppt_knn_group_f32(_p(xyz), _p(center), B, N, G, k, _p(idx), _p(nb), _p(nd), _stream()),
                   "ppt_knn_group_f32")
    else:
        _chk_lengths(lengths, B)
        _lib.check(_lib.lib().ppt_knn_group_ragged_f32(_p(xyz), _p(center), B, N, G, k, _p(lengths), _p(idx), _p(nb), _p(nd),
                                                       _stream()), "ppt_knn_group_ragged_f32")
    if profiler is not None:
        profiler.end()
    return (idx, nb, nd) if want_dist else (idx, nb)


def ball_query_multi(xyz, center, queries, want_grouped=False, lengths=None):
    """queries = [(radius, K), ...] (1..3) around the same centres, one pass over the cloud (ppt_ball_query_multi_f32)
    -> [(idx [B,S,K] i64, grouped_xyz [B,S,K,3] | None), ...]; same results as ball_query per pair.  lengths: as ball_query."""
    _chk(xyz, torch.float32, "xyz"); _chk(center, torch.float32, "center")
    import numpy as np
    B, N, _ = xyz.shape
    S = center.shape[1]
    q = _lib.BallMulti()
    q.n = len(queries)
    outs, bytes_ = [], 12 * N + 12 * S
    for j, (r, K) in enumerate(queries):
        idx = torch.empty((B, S, K), dtype=torch.int64, device=xyz.device)
        g = torch.empty((B, S, K, 3), dtype=torch.float32, device=xyz.device) if want_grouped else None
        q.r2[j], q.K[j] = float(np.float32(r * r)), K
        q.idx[j], q.gxyz[j] = idx.data_ptr(), (g.data_ptr() if g is not None else None)
        outs.append((idx, g))
        bytes_ += 8 * S * K + (12 * S * K if want_grouped else 0)
    if profiler is not None:
        profiler.begin("ball_query", float(B) * bytes_)
    if lengths is None:
        _lib.check(_lib.lib().ppt_ball_query_multi_f32(_p(xyz), _p(center), B, N, S, ctypes.byref(q), _stream()), "ppt_ball_query_multi_f32")
    else:
        _chk_lengths(lengths, B)
        _lib.check(_lib.lib().ppt_ball_query_multi_ragged_f32(_p(xyz), _p(center), B, N, S, _p(lengths), ctypes.byref(q), _stream()),
                   "ppt_ball_query_multi_ragged_f32")
    if profiler is not None:
        profiler.end()
    return outs


def square_distance(src, dst):
    """dvae.py:130-149: src [B,S,3], dst [B,N,3] f32 -> [B,S,N] f32 with the reference's rounding sequence."""
    _chk(src, torch.float32, "src"); _chk(dst, torch.float32, "dst")
    B, S, _ = src.shape
    N = dst.shape[1]
    out = torch.empty((B, S, N), dtype=torch.float32, device=src.device)
    _lib.check(_lib.lib().ppt_square_distance_f32(_p(src), _p(dst), B, S, N, _p(out), _stream()), "ppt_square_distance_f32")
    return out


def ball_query(xyz, center, radius, K, want_grouped=False, lengths=None):
    """H7.  -> idx [B,S,K] i64 (query_ball_point semantics) [, grouped_xyz [B,S,K,3] = xyz[idx] - center].  lengths [B] i32
    (device): per-cloud row counts; an empty ball is filled with the cloud's own length (ppt_ball_query_ragged_f32)."""
    _chk(xyz, torch.float32, "xyz"); _chk(center, torch.float32, "center")
    B, N, _ = xyz.shape
    S = center.shape[1]
    idx = torch.empty((B, S, K), dtype=torch.int64, device=xyz.device)
    import numpy as np
    r2 = float(np.float32(radius * radius))
    g = torch.empty((B, S, K, 3), dtype=torch.float32, device=xyz.device) if want_grouped else None
    if profiler is not None:                    # algorithmic HBM bytes per SA branch: cloud + centres + indices (+ grouped xyz)
        profiler.begin("ball_query", float(B) * (12 * N + 12 * S + 8 * S * K + (12 * S * K if want_grouped else 0)))
    if lengths is None:
        _lib.check(_lib.lib().ppt_ball_query_f32(_p(xyz), _p(center), B, N, S, r2, K, _p(idx), _p(g), _stream()),
                   "ppt_ball_query_f32")
    else:
        _chk_lengths(lengths, B)
        _lib.check(_lib.lib().ppt_ball_query_ragged_f32(_p(xyz), _p(center), B, N, S, r2, K, _p(lengths), _p(idx), _p(g), _stream()),
                   "ppt_ball_query_ragged_f32")
    if profiler is not None:
        profiler.end()
    return (idx, g) if want_grouped else idx


# ---------------------------------------------------------------------------------------------
# split16 (ppt_gemm_params.split16): the powers of two the A / B operand values are multiplied by before they are split into
# hi + lo halves.  A: activations and S-scaled gradients (ppt_amd/gradscale.py) -- typical magnitude 1e-3 .. 1e2, left where they
# are; B: weights (typically 0.01 .. 0.1, |w| < 4 095 required) -- x 16 puts them where half keeps all of hi + lo's 22 bits.
SPLIT16_POW2 = (int(os.environ.get("PPT_SPLIT16_A_POW2", "0")), int(os.environ.get("PPT_SPLIT16_B_POW2", "4")))
# Process-wide on purpose (not thread-local): a node's backward runs on autograd's device thread.  The last model that fetched its
# WeightCache decides -- a model's backward follows its forward in every loop of the reference (main_cls.py:194-198).
_SPLIT16 = False
ATTN_SPLIT16 = os.environ.get("PPT_ATTN_SPLIT16", "1") != "0"      # 0: the split16 mode keeps the fp32 VALU attention forward


def set_split16(on, pow2=None):
    """fp32-operand ops.gemm calls that do not say `split=` themselves use the split16 products from now on (True) or the fp32
    MFMA (False).  pow2: the (A, B) pre-scales of the model that says so (ULIP_WITH_IMAGE.split_pow2: its weight range decides B's,
    _fit_split16_range) -- every model re-asserts its OWN pair with the flag whenever it fetches its WeightCache, so one model's
    fit no longer changes another's."""
    global _SPLIT16, SPLIT16_POW2
    _SPLIT16 = bool(on)
    if on and pow2 is not None:
        SPLIT16_POW2 = (int(pow2[0]), int(pow2[1]))


_SPLIT_OVERFLOW = {}


def split16_overflow_counter(device=None):
    """The device word (uint32, one per GPU, process-wide, never re-allocated: captured hipGraphs keep its address) to which every
    split16 GEMM wave that SATURATED a finite operand beyond IEEE half's range adds 1 (ppt_gemm_params.split_overflow).  A counter,
    not a flag: readers compare with the value they saw last (health.Monitor), nothing ever clears it, so a read on one stream
    cannot race with an add from another."""
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    if dev not in _SPLIT_OVERFLOW:
        _SPLIT_OVERFLOW[dev] = torch.zeros((1,), dtype=torch.int32, device=torch.device("cuda", dev))
    return _SPLIT_OVERFLOW[dev]


def split16_enabled():
    return _SPLIT16


def gemm(A, B, *, out=None, out_dtype=None, M=None, bias=None, act=ACT_NONE, dact_pre=None,
         group_add=None, group_rows=0, row_scale=None, row_scale_rows=0, residual=None,
         residual2=None, out2=None, out2_pre=False, col_stats=None, pool_max=None, pool_min=None, pool_rows=0,
         batch=1, strideA=0, strideB=0, strideC=0,
         a_mode=A_PLAIN, a_scale=None, a_shift=None, pts=None, w1=None, b1=None, want_out=True, algo_k=None, core=None, split=None):
    """C[M,N] = epilogue(prologue(A)[M,K] @ B[N,K]^T) -- see struct ppt_gemm_params.
    A [M,K] (or None with a_mode=A_CONV1 and pts [M,3]); B [N,K]; 2-D, last-dim contiguous
    (row stride may exceed K).  Returns out (or None when want_out=False).
    split (fp32 operands only): True / (a_pow2, b_pow2) multiplies hi + lo half pairs on the 16-bit matrix pipe (split16,
    ppt_gemm_params.split16); False: the fp32 MFMA; None: what set_split16() last said (a model in the "split16" precision mode
    says it whenever it fetches its WeightCache, in forward and in backward)."""
    p = GemmParams()
    N, K = B.shape
    if a_mode == A_CONV1:
        M = pts.shape[0]
        dev = pts.device
    else:
        M = A.shape[0] if M is None else M
        dev = A.device
        assert A.shape[1] == K and A.stride(1) == 1 and A.dtype == B.dtype
        p.A, p.lda = _p(A), A.stride(0)
    assert B.stride(1) == 1
    p.B, p.ldb = _p(B), B.stride(0)
    p.M, p.N, p.K = M, N, K
    p.dtype = dtype_code(B)
    if out is None and want_out:
        out = torch.empty((M, N), dtype=out_dtype or B.dtype, device=dev)
    if out is not None:
        assert out.stride(1) == 1
        p.C, p.ldc, p.c_dtype = _p(out), out.stride(0), dtype_code(out)
    p.a_mode = a_mode
    p.a_scale, p.a_shift, p.pts, p.w1, p.b1 = _p(a_scale), _p(a_shift), _p(pts), _p(w1), _p(b1)
    p.bias = _p(bias)
    p.group_add, p.group_rows = _p(group_add), group_rows
    p.act = act
    if dact_pre is not None:
        assert dact_pre.dtype == B.dtype and dact_pre.stride(1) == 1
        p.dact_pre, p.ld_dact = _p(dact_pre), dact_pre.stride(0)
    p.row_scale, p.row_scale_rows = _p(row_scale), row_scale_rows
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.stride(-1) == 1
        p.residual, p.ld_res = _p(residual), residual.stride(-2)
    if residual2 is not None:
        assert residual2.dtype == torch.float32 and residual2.stride(-1) == 1
        p.residual2, p.ld_res2 = _p(residual2), residual2.stride(-2)
    if out2 is not None:
        p.C2, p.ldc2, p.c2_dtype, p.c2_pre = _p(out2), out2.stride(-2), dtype_code(out2), int(out2_pre)
    if col_stats is not None:
        p.col_sum, p.col_sqsum = _p(col_stats[0]), _p(col_stats[1])
    if pool_max is not None:
        p.pool_max, p.pool_dtype, p.pool_rows = _p(pool_max), dtype_code(pool_max), pool_rows
        p.pool_min = _p(pool_min)
    p.batch, p.strideA, p.strideB, p.strideC = batch, strideA, strideB, strideC
    if split is None:
        split = _SPLIT16
    if split and p.dtype == PPT_F32:
        p.split16 = 2 if core == "tiles" else 1          # ("tiles": keep the launch off the 256 x 128 split kernel -- A/B, tests)
        p.split_a_pow2, p.split_b_pow2 = split if isinstance(split, tuple) else SPLIT16_POW2
        if not torch.cuda.is_current_stream_capturing() or dev.index in _SPLIT_OVERFLOW:
            p.split_overflow = _p(split16_overflow_counter(dev))      # (first use outside a capture: the word is allocated there)
    if profiler is not None:
        kk = K if algo_k is None else algo_k
        # ("bf16" names the 16-bit MFMA family of the roofline table: bf16 and fp16 operands run at the same rate)
        profiler.begin("gemm_" + ("bf16" if p.dtype != PPT_F32 else "f32"), 2.0 * M * N * kk * max(1, batch),
                       "ppt_gemm " + ({PPT_BF16: "bf16", PPT_F16: "f16"}.get(p.dtype, "f32")) + (" (A-prologue)" if a_mode != A_PLAIN else ""),
                       executed=2.0 * M * N * K * max(1, batch))
    if core == "256":                  # the 256-row macro-tile core, explicitly (tests / tools; ppt_gemm picks it by itself)
        _lib.check(_lib.lib().ppt_gemm256(ctypes.byref(p), _stream()), "ppt_gemm256")
    else:
        _lib.check(_lib.lib().ppt_gemm(ctypes.byref(p), _stream()), "ppt_gemm")
    if profiler is not None:
        profiler.end()
    if probe is not None:
        _probe("gemm", out); _probe("gemm (second output)", out2)
    return out


class wave_priority:
    """with ops.wave_priority(1): every launch made inside raises its waves' issue priority (ppt_set_wave_priority; the
    kernels of the prompt chain take it as an argument, so a hipGraph captured inside keeps it)."""

    def __init__(self, prio):
        self.prio = int(bool(prio))

    def __enter__(self):
        self.old = _lib.lib().ppt_get_wave_priority()
        _lib.lib().ppt_set_wave_priority(self.prio)

    def __exit__(self, *exc):
        _lib.lib().ppt_set_wave_priority(self.old)


def cross_entropy_rows(logits, labels, smoothing, ignore_index=-100):
    """(loss 0-d, dlogits [R,C], scale 0-d) of nn.CrossEntropyLoss(label_smoothing=smoothing) with mean reduction
    (ppt_cross_entropy_rows).  Rows whose label == ignore_index (outside [0, C)) are ignored as ATen ignores them; any other label
    outside [0, C) makes the loss NaN (ATen: device assert).  dlogits is scaled by 1 / R and `scale` = R / counted rows (1.0 when
    none is ignored) completes it."""
    assert not (0 <= ignore_index < logits.shape[1]), "ignore_index inside [0, C) is not covered by ppt_cross_entropy_rows"
    _chk(logits, torch.float32, "logits"); _chk(labels, torch.int64, "labels")
    R, C = logits.shape
    out = torch.empty((2,), dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    partial = torch.empty((2 * ((R + 127) // 128),), dtype=torch.float32, device=logits.device)
    _lib.check(_lib.lib().ppt_cross_entropy_rows(_p(logits), _p(labels), float(smoothing), R, C, int(ignore_index), _p(out), _p(dlogits),
                                                 _p(partial), _stream()), "ppt_cross_entropy_rows")
    return out[0], dlogits, out[1]


class persistent_occupancy:
    """with ops.persistent_occupancy(60): the persistent point-tower kernels launched inside size their grids for 60 % of the
    CUs (ppt_set_persistent_occupancy) -- room for the prompt chain on the other stream."""

    def __init__(self, percent):
        self.percent = int(percent)

    def __enter__(self):
        self.old = _lib.lib().ppt_get_persistent_occupancy()
        _lib.lib().ppt_set_persistent_occupancy(self.percent)

    def __exit__(self, *exc):
        _lib.lib().ppt_set_persistent_occupancy(self.old)


def get_persistent_occupancy():
    return _lib.lib().ppt_get_persistent_occupancy()


def rows_matmul(a, w_kn, alpha=1.0):
    """out [M,N] = alpha * a [M,K] @ w_kn [K,N], fp32, for a few rows (ppt_rows_matmul_f32) -- None when the shape is not covered."""
    _chk(a, torch.float32, "a"); _chk(w_kn, torch.float32, "w_kn")
    M, K = a.shape
    N = w_kn.shape[1]
    if K > 1536 or K % 32 or w_kn.shape[0] != K:
        return None
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    if profiler is not None:
        profiler.begin("gemm_f32", 2.0 * M * N * K, "ppt_rows_matmul_f32")
    _lib.check(_lib.lib().ppt_rows_matmul_f32(_p(a), _p(w_kn), M, K, N, float(alpha), _p(out), _stream()), "ppt_rows_matmul_f32")
    if profiler is not None:
        profiler.end()
    return out


# Which schedule of the fused frozen-block kernel runs (supported switch): 3 = csrc/mlp_fused3.hip (round 6: 256-unit
# slabs, GELU under fc2's MFMAs, residual kept in the accumulators), 2 = csrc/mlp_fused.hip (rounds 2-5).  The fragment-ordered
# weight copies differ, so vit_mlp_retile tags what it returns and vit_mlp follows the tag.
VIT_MLP_VARIANT = int(os.environ.get("PPT_VIT_MLP", "3"))


def vit_mlp_retile(w1, w2, variant=None):
    """(w1 [1536,384], w2 [384,1536]) 16-bit -> the fragment-ordered copies the fused kernel reads (ppt_vit_mlp_retile for
    variant 2, ppt_vit_mlp3_retile for variant 3; default VIT_MLP_VARIANT)."""
    assert w1.dtype in HALF and w2.dtype == w1.dtype
    _chk(w1, w1.dtype, "w1"); _chk(w2, w1.dtype, "w2")
    assert tuple(w1.shape) == (1536, 384) and tuple(w2.shape) == (384, 1536)
    variant = VIT_MLP_VARIANT if variant is None else int(variant)
    w1t, w2t = torch.empty_like(w1), torch.empty_like(w2)
    fn = _lib.lib().ppt_vit_mlp3_retile if variant == 3 else _lib.lib().ppt_vit_mlp_retile
    _lib.check(fn(_p(w1), _p(w2), _p(w1t), _p(w2t), _stream()), "ppt_vit_mlp_retile")
    w1t.ppt_variant = w2t.ppt_variant = variant          # (a plain attribute, like the copy event of data/prefetch.py)
    return w1t, w2t


def lnlin_retile(w):
    """w [N, 384] 16-bit (N a multiple of 384) -> the fragment-ordered copy ppt_lnlin reads."""
    assert w.dtype in HALF and w.dim() == 2 and w.shape[1] == 384 and w.shape[0] % 384 == 0
    _chk(w, w.dtype, "w")
    wt = torch.empty_like(w)
    _lib.check(_lib.lib().ppt_lnlin_retile(_p(w), _p(wt), w.shape[0], _stream()), "ppt_lnlin_retile")
    return wt


def lnlin(x, wt, ln, *, bias=None, ln_eps=1e-5, out=None):
    """LayerNorm(x [M, 384] f32; ln = (weight, bias)) @ W^T (+ bias) -> [M, N] in the weight's 16-bit dtype (csrc/lnlin.hip: rows
    stationary, weight streamed; wt = lnlin_retile(W))."""
    _chk(x, torch.float32, "x")
    M, K = x.shape
    N = wt.shape[0]
    assert K == 384 and wt.dtype in HALF
    out = torch.empty((M, N), dtype=wt.dtype, device=x.device) if out is None else out
    p = _lib.LnLinParams()
    p.x, p.W, p.C, p.ln_w, p.ln_b, p.ln_eps, p.bias = _p(x), _p(wt), _p(out), _p(ln[0]), _p(ln[1]), float(ln_eps), _p(bias)
    p.M, p.N, p.K, p.dtype = M, N, K, dtype_code(wt)
    if profiler is not None:
        profiler.begin("gemm_bf16", 2.0 * M * N * K, "ppt_lnlin (LayerNorm prologue)")
    _lib.check(_lib.lib().ppt_lnlin(ctypes.byref(p), _stream()), "ppt_lnlin")
    if profiler is not None:
        profiler.end()
    return out


def text_mlp_retile(w1, w2, b_pow2=None):
    """(w1 [2048, 512], w2 [512, 2048]) row-major -> the fragment-ordered copies ppt_text_mlp_pair reads (csrc/text_mlp.hip).  Forward:
    (c_fc.weight, c_proj.weight); backward: (c_proj.weight^T, c_fc.weight^T) -- the same shapes.  16-bit weights: copies of the same
    dtype; fp32 weights: the split16 form's hi + lo half copies (uint8 [4 MB] each), multiplied by 2^b_pow2 (default: the current
    SPLIT16_POW2's B scale) -- the copies remember the scale they were made with (`.ppt_b_pow2`)."""
    assert w1.dtype in HALF + (torch.float32,) and w2.dtype == w1.dtype and tuple(w1.shape) == (2048, 512) and tuple(w2.shape) == (512, 2048)
    _chk(w1, w1.dtype, "w1"); _chk(w2, w1.dtype, "w2")
    if w1.dtype != torch.float32:
        w1t, w2t = torch.empty_like(w1), torch.empty_like(w2)
        _lib.check(_lib.lib().ppt_text_mlp_retile(_p(w1), _p(w2), _p(w1t), _p(w2t), _stream()), "ppt_text_mlp_retile")
        return w1t, w2t
    b = SPLIT16_POW2[1] if b_pow2 is None else int(b_pow2)
    w1t = torch.empty((2048 * 512 * 4,), dtype=torch.uint8, device=w1.device)
    w2t = torch.empty((2048 * 512 * 4,), dtype=torch.uint8, device=w1.device)
    _lib.check(_lib.lib().ppt_text_mlp_retile_split(_p(w1), _p(w2), _p(w1t), _p(w2t), b, _stream()), "ppt_text_mlp_retile_split")
    w1t.ppt_b_pow2 = w2t.ppt_b_pow2 = b
    return w1t, w2t


text_mlp_retile_split = text_mlp_retile       # (the split16 form's earlier names: the form follows the operands)


def text_lin_retile_split(w, b_pow2=None):
    """w [N, K] fp32 row-major (N a multiple of 256, K of 512) -> the fragment-ordered hi + lo half copy text_lin_split reads (uint8,
    N * K * 4 bytes), multiplied by 2^b_pow2 (default: the current SPLIT16_POW2's B scale); remembers (N, K, b_pow2)."""
    assert w.dtype == torch.float32 and w.dim() == 2
    _chk(w, torch.float32, "w")
    N, K = w.shape
    b = SPLIT16_POW2[1] if b_pow2 is None else int(b_pow2)
    wt = torch.empty((N * K * 4,), dtype=torch.uint8, device=w.device)
    _lib.check(_lib.lib().ppt_text_lin_retile_split(_p(w), _p(wt), N, K, b, _stream()), "ppt_text_lin_retile_split")
    wt.ppt_shape, wt.ppt_b_pow2 = (N, K), b
    return wt


def text_lin_split(a, wt, *, bias=None, residual=None, out=None, a_pow2=None):
    """a [M, K] fp32 @ W^T (+ bias) (+ residual) on split16 products, rows stationary (csrc/text_lin.hip; wt =
    text_lin_retile_split(W)) -> out [M, N] fp32; K > 512: the K / 512 partial products [K / 512, M, N] (no bias / residual)."""
    N, K = wt.ppt_shape
    M = a.shape[0]
    assert a.dtype == torch.float32 and a.dim() == 2 and a.shape[1] == K and a.stride(1) == 1
    kc = K // 512
    if kc > 1:
        assert bias is None and residual is None and out is None
        out = torch.empty((kc, M, N), dtype=torch.float32, device=a.device)
    elif out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    p = _lib.TextLinParams()
    p.A, p.lda, p.W, p.bias = _p(a), a.stride(0), _p(wt), _p(bias)
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.stride(-1) == 1
        p.residual, p.ld_res = _p(residual), residual.stride(-2)
    p.C, p.ldc = _p(out), (N if kc > 1 else out.stride(0))
    p.M, p.N, p.K = M, N, K
    p.split_a_pow2 = SPLIT16_POW2[0] if a_pow2 is None else int(a_pow2)
    p.split_b_pow2 = int(wt.ppt_b_pow2)
    if not torch.cuda.is_current_stream_capturing() or a.device.index in _SPLIT_OVERFLOW:
        p.split_overflow = _p(split16_overflow_counter(a.device))
    if profiler is not None:
        profiler.begin("gemm_f32", 2.0 * M * N * K, "ppt_text_lin_split")
    _lib.check(_lib.lib().ppt_text_lin_split(ctypes.byref(p), _stream()), "ppt_text_lin_split")
    if profiler is not None:
        profiler.end()
    return out


def text_lin_retile16(w):
    """w [N, K] 16-bit row-major (N a multiple of 256, K of 512) -> the fragment-ordered copy text_lin16 reads (uint8, N * K * 2
    bytes, the same values); remembers (N, K, dtype)."""
    assert w.dtype in HALF and w.dim() == 2
    _chk(w, w.dtype, "w")
    N, K = w.shape
    wt = torch.empty((N * K * 2,), dtype=torch.uint8, device=w.device)
    _lib.check(_lib.lib().ppt_text_lin_retile16(_p(w), _p(wt), N, K, _stream()), "ppt_text_lin_retile16")
    wt.ppt_shape, wt.ppt_dtype = (N, K), w.dtype
    return wt


def text_lin16(a, wt, *, bias=None, residual=None, out=None, out_dtype=None):
    """a [M, K] 16-bit @ W^T (+ bias) (+ residual), rows stationary (csrc/text_lin.hip; wt = text_lin_retile16(W), W in a's
    dtype) -> out [M, N] in out_dtype (a's dtype by default, or fp32; out= may be a strided view); K > 512: the K / 512 fp32 partial
    products [K / 512, M, N] (no bias / residual).  16-bit results are rounded as gemm rounds them."""
    N, K = wt.ppt_shape
    M = a.shape[0]
    assert a.dtype == wt.ppt_dtype and a.dim() == 2 and a.shape[1] == K and a.stride(1) == 1
    kc = K // 512
    if kc > 1:
        assert bias is None and residual is None and out is None and out_dtype in (None, torch.float32)
        out = torch.empty((kc, M, N), dtype=torch.float32, device=a.device)
    elif out is None:
        out = torch.empty((M, N), dtype=out_dtype or a.dtype, device=a.device)
    assert out.dtype in (torch.float32, a.dtype) and out.stride(-1) == 1
    p = _lib.TextLin16Params()
    p.A, p.lda, p.W, p.bias = _p(a), a.stride(0), _p(wt), _p(bias)
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.stride(-1) == 1
        p.residual, p.ld_res = _p(residual), residual.stride(-2)
    p.C, p.ldc = _p(out), (N if kc > 1 else out.stride(0))
    p.M, p.N, p.K, p.dtype, p.c_dtype = M, N, K, _DT[a.dtype], _DT[out.dtype]
    if profiler is not None:
        profiler.begin("gemm_bf16", 2.0 * M * N * K, "ppt_text_lin16")
    _lib.check(_lib.lib().ppt_text_lin16(ctypes.byref(p), _stream()), "ppt_text_lin16")
    if profiler is not None:
        profiler.end()
    return out


def text_mlp_pair(a, w1t, w2t, *, bias=None, pre=None, backward=False, a_pow2=None, ln=None, ln_eps=1e-5, save_stats=False):
    """The MLP half of a CLIP text layer in one launch (csrc/text_mlp.hip) -> the eight slices' partial products [8, M, 512] f32.
    forward: QuickGELU(a w1^T + bias) w2^T, `pre` (optional, [M, 2048]) receives the pre-activation; backward=True:
    ((a w1^T) * QuickGELU'(pre)) w2^T with w1 / w2 the transposed weights' tiled copies.  The caller's LayerNorm sums the slices
    (layernorm_fwd_sum / layernorm_bwd_sum).  The operand form follows the tiled weights (text_mlp_retile): 16-bit copies -> `a` and
    `pre` in their dtype; the split16 copies (uint8) -> `a` and `pre` fp32, every product on hi + lo half pairs with `a` multiplied by
    2^a_pow2 (default: the current SPLIT16_POW2's A scale).
    ln = (weight, bias) (forward only): `a` is the FP32 residual stream and the LayerNorm in front of the branch (ln_2) is applied while
    the rows are staged; save_stats -> also returns (mean, rstd) [M] for the LayerNorm backward: (parts, mean, rstd)."""
    M = a.shape[0]
    split = w1t.dtype == torch.uint8
    t = torch.float32 if split else w1t.dtype
    assert a.dim() == 2 and a.shape[1] == 512 and a.stride(1) == 1 and (split or t in HALF) and w2t.dtype == w1t.dtype
    assert a.dtype == (torch.float32 if ln is not None else t) and not (ln is not None and backward)
    parts = torch.empty((8, M, 512), dtype=torch.float32, device=a.device)
    p = _lib.TextMlpParams()
    p.A, p.lda, p.W1, p.W2, p.b1, p.pre, p.parts = _p(a), a.stride(0), _p(w1t), _p(w2t), _p(bias), _p(pre), _p(parts)
    p.M, p.D, p.hidden, p.mode, p.dtype = M, 512, 2048, int(bool(backward)), (PPT_F32 if split else dtype_code(w1t))
    if split:
        p.split_a_pow2 = SPLIT16_POW2[0] if a_pow2 is None else int(a_pow2)
        p.split_b_pow2 = int(w1t.ppt_b_pow2)
        if not torch.cuda.is_current_stream_capturing() or a.device.index in _SPLIT_OVERFLOW:
            p.split_overflow = _p(split16_overflow_counter(a.device))
    mean = rstd = None
    if ln is not None:
        _chk(ln[0], torch.float32, "ln weight"); _chk(ln[1], torch.float32, "ln bias")
        if save_stats:
            mean = torch.empty((M,), dtype=torch.float32, device=a.device)
            rstd = torch.empty((M,), dtype=torch.float32, device=a.device)
        p.ln_w, p.ln_b, p.ln_eps, p.ln_mean, p.ln_rstd = _p(ln[0]), _p(ln[1]), float(ln_eps), _p(mean), _p(rstd)
    if pre is not None:
        assert pre.dtype == t and tuple(pre.shape) == (M, 2048) and pre.is_contiguous()
    direction = "backward" if backward else "forward"
    if profiler is not None:
        profiler.begin("gemm_f32" if split else "gemm_bf16", 4.0 * M * 512 * 2048, f"ppt_text_mlp_pair {'split16 ' if split else ''}({direction})")
    _lib.check(_lib.lib().ppt_text_mlp_pair(ctypes.byref(p), _stream()), "ppt_text_mlp_pair (split16)" if split else "ppt_text_mlp_pair")
    if profiler is not None:
        profiler.end()
    return (parts, mean, rstd) if ln is not None else parts


text_mlp_pair_split = text_mlp_pair


def vit_proj_retile(wp):
    """attn.proj.weight [384,384] (16-bit) -> the fragment-ordered copy the fused proj prologue of ppt_vit_mlp_bf16 reads."""
    assert wp.dtype in HALF and tuple(wp.shape) == (384, 384)
    _chk(wp, wp.dtype, "wp")
    wpt = torch.empty_like(wp)
    _lib.check(_lib.lib().ppt_vit_proj_retile(_p(wp), _p(wpt), _stream()), "ppt_vit_proj_retile")
    return wpt


def vit_mlp(x, w1, b1, w2, b2, ln, *, out=None, ln_eps=1e-5, row_scale=None, row_scale_rows=0, residual2=None, workgroups=0, proj=None):
    """ppt_vit_mlp_bf16 (csrc/mlp_fused.hip): out = x + row_scale * (GELU(LN(x) w1^T + b1) w2^T + b2) (+ residual2), x [M,384]
    f32, w1 / w2: the fragment-ordered bf16 weights of vit_mlp_retile; out defaults to x (in place).
    proj = (a [M,384] 16-bit, wp_tiled (vit_proj_retile), bias | None, row_scale1 | None, rows): the attention branch's tail in
    front -- x <- x + row_scale1 * (a wp^T + bias) first (written to out), then the MLP branch on that."""
    assert w1.dtype in HALF and w2.dtype == w1.dtype
    _chk(x, torch.float32, "x"); _chk(w1, w1.dtype, "w1"); _chk(w2, w1.dtype, "w2")
    M, D = x.shape
    out = x if out is None else out
    p = _lib.VitMlpParams()
    p.dtype = dtype_code(w1)
    p.x, p.out, p.W1, p.W2, p.ln_w, p.ln_b, p.ln_eps = _p(x), _p(out), _p(w1), _p(w2), _p(ln[0]), _p(ln[1]), ln_eps
    p.b1, p.b2, p.row_scale, p.row_scale_rows, p.residual2 = _p(b1), _p(b2), _p(row_scale), row_scale_rows, _p(residual2)
    p.M, p.D, p.hidden, p.workgroups = M, D, w1.shape[0], workgroups
    flops = 4.0 * M * D * w1.shape[0]
    if proj is not None:
        a, wpt, pb, rs1, rs1_rows = proj
        assert a.dtype == w1.dtype and wpt.dtype == w1.dtype and tuple(a.shape) == (M, D)
        _chk(a, a.dtype, "proj a"); _chk(wpt, a.dtype, "proj w")
        p.proj_a, p.proj_W, p.proj_b, p.proj_row_scale, p.proj_row_scale_rows = _p(a), _p(wpt), _p(pb), _p(rs1), int(rs1_rows)
        flops += 2.0 * M * D * D
    if profiler is not None:
        profiler.begin("gemm_bf16", flops, "ppt_vit_mlp_bf16 (" + ("proj + residual + " if proj is not None else "") + "LN + fc1 + GELU + fc2 + residual)")
    variant = getattr(w1, "ppt_variant", 2)                  # (the order the weights were re-tiled in decides the kernel)
    assert getattr(w2, "ppt_variant", 2) == variant
    if variant == 3:
        _lib.check(_lib.lib().ppt_vit_mlp3_bf16(ctypes.byref(p), _stream()), "ppt_vit_mlp3_bf16")
    else:
        _lib.check(_lib.lib().ppt_vit_mlp_bf16(ctypes.byref(p), _stream()), "ppt_vit_mlp_bf16")
    if profiler is not None:
        profiler.end()
    return out


ROWGEMM_K = (384, 512)


def rowgemm(A, W, *, ln=None, ln_eps=1e-5, ln_stats=None, bias=None, act=ACT_NONE, out=None, out2=None, residual=None, residual2=None,
            row_scale=None, row_scale_rows=0, walkers=0):
    """ppt_rowgemm_bf16 (csrc/rowgemm.hip): C = epilogue(prologue(A) @ W^T) with W [N,K] bf16 held in registers.
    A: bf16 [M,K], or -- with ln = (gamma, beta) -- the f32 residual stream, LayerNorm applied while the rows are staged.
    residual given: the f32 form out = residual + row_scale[m // row_scale_rows] * (acc + bias) + residual2 (out may be
    residual itself); else out (bf16) = act(acc + bias) and out2 (bf16, optional) receives the pre-activation."""
    M, K = A.shape
    N = W.shape[0]
    T = W.dtype
    assert W.shape[1] == K and T in HALF and W.is_contiguous() and A.is_contiguous()
    assert A.dtype == (torch.float32 if ln is not None else T)
    p = RowGemmParams()
    p.A, p.W, p.M, p.N, p.K = _p(A), _p(W), M, N, K
    p.dtype = dtype_code(W)
    if ln is not None:
        p.a_ln, p.ln_w, p.ln_b, p.ln_eps = 1, _p(ln[0]), _p(ln[1]), ln_eps
        if ln_stats is not None:                     # (mean [M], rstd [M]) f32: what ppt_layernorm_bwd needs
            p.ln_mean, p.ln_rstd = _p(ln_stats[0]), _p(ln_stats[1])
    p.bias, p.act = _p(bias), act
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.is_contiguous() and residual.shape == (M, N)
        if out is None:
            out = torch.empty((M, N), dtype=torch.float32, device=A.device)
        assert out.dtype == torch.float32 and out.is_contiguous()
        p.residual_form, p.residual, p.residual2 = 1, _p(residual), _p(residual2)
        p.row_scale, p.row_scale_rows = _p(row_scale), row_scale_rows
    else:
        if out is None:
            out = torch.empty((M, N), dtype=T, device=A.device)
        assert out.dtype == T and out.is_contiguous()
        if out2 is not None:
            assert out2.dtype == T and out2.is_contiguous()
            p.C2 = _p(out2)
    p.C, p.walkers = _p(out), walkers
    if profiler is not None:
        profiler.begin("gemm_bf16", 2.0 * M * N * K, "ppt_rowgemm_bf16" + (" (LayerNorm prologue)" if ln is not None else
                                                                            " (residual form)" if residual is not None else ""))
    _lib.check(_lib.lib().ppt_rowgemm_bf16(ctypes.byref(p), _stream()), "ppt_rowgemm_bf16")
    if profiler is not None:
        profiler.end()
    if probe is not None:
        _probe("rowgemm", out); _probe("rowgemm (second output)", out2)
    return out


def layernorm_fwd(x, w, b, y_dtype, add=None, add_rows=0, write_xs=None, save_stats=False, eps=1e-5):
    """y = LN(x (+ add)); x f32 [..., D].  write_xs: f32 tensor receiving x+add (may be x itself).
    Returns (y, mean, rstd)."""
    _chk(x, torch.float32, "x")
    D = x.shape[-1]
    M = x.numel() // D
    y = torch.empty(x.shape, dtype=y_dtype, device=x.device)
    mean = torch.empty((M,), dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty((M,), dtype=torch.float32, device=x.device) if save_stats else None
    _lib.check(_lib.lib().ppt_layernorm_fwd(_p(x), _p(add), add_rows, _p(write_xs), _p(w), _p(b), _p(y),
                                            dtype_code(y), _p(mean), _p(rstd), M, D, eps, _stream()),
               "ppt_layernorm_fwd")
    if probe is not None:
        _probe("layernorm", y)
    return y, mean, rstd


def layernorm_fwd_sum(x, bias, parts, w, b, y_dtype, write_xs, save_stats=False, eps=1e-5):
    """y = LN(x + bias + parts[0] + ... + parts[S-1]) -- the consumer of a split-K linear (ppt_layernorm_fwd_sum): x f32 [M, D],
    parts f32 [S, M, D] (the S partial products, ops.gemm_splitk), bias [D] or None; write_xs receives the summed rows.
    Returns (y, mean, rstd)."""
    _chk(x, torch.float32, "x"); _chk(parts, torch.float32, "parts"); _chk(write_xs, torch.float32, "write_xs")
    D = x.shape[-1]
    M = x.numel() // D
    S = parts.shape[0]
    assert parts.numel() == S * M * D
    y = torch.empty(x.shape, dtype=y_dtype, device=x.device)
    mean = torch.empty((M,), dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty((M,), dtype=torch.float32, device=x.device) if save_stats else None
    _lib.check(_lib.lib().ppt_layernorm_fwd_sum(_p(x), _p(bias), _p(parts), S, _p(write_xs), _p(w), _p(b), _p(y), dtype_code(y),
                                                _p(mean), _p(rstd), M, D, eps, _stream()), "ppt_layernorm_fwd_sum")
    if probe is not None:
        _probe("layernorm", y)
    return y, mean, rstd


def layernorm_bwd_sum(dy_parts, xs, w, mean, rstd, dx, accumulate=True, copy_dtype=None):
    """layernorm_bwd's input-gradient form with dy = dy_parts[0] + ... + dy_parts[S-1] ([S, M, D] f32) -> (dx, dx_copy)."""
    _chk(dy_parts, torch.float32, "dy_parts"); _chk(xs, torch.float32, "xs")
    D = xs.shape[-1]
    M = xs.numel() // D
    S = dy_parts.shape[0]
    assert dy_parts.numel() == S * M * D
    cp = torch.empty(xs.shape, dtype=copy_dtype, device=xs.device) if copy_dtype is not None else None
    _lib.check(_lib.lib().ppt_layernorm_bwd_sum(_p(dy_parts), S, _p(xs), _p(w), _p(mean), _p(rstd), _p(dx), int(accumulate), _p(cp),
                                                dtype_code(cp) if cp is not None else 0, M, D, _stream()), "ppt_layernorm_bwd_sum")
    return dx, cp


def gemm_splitk(A, B, S):
    """The S partial products of A [M, K] @ B [N, K]^T over K slices of K / S as fp32 slices [S, M, N] (one batched ppt_gemm launch,
    plain epilogue): for skinny problems (the prompt chain: 817 rows) whose K loop is what takes the time.  K / S must be a multiple
    of 64 elements (the 64 x 64 LDS-DMA tile loop's slab)."""
    M, K = A.shape
    N = B.shape[0]
    Ks = K // S
    assert Ks * S == K and Ks % 64 == 0 and A.stride(1) == 1 and B.stride(1) == 1
    part = torch.empty((S, M, N), dtype=torch.float32, device=A.device)
    gemm(A[:, :Ks], B[:, :Ks], out=part.view(S * M, N), M=M, batch=S, strideA=Ks, strideB=Ks, strideC=M * N)
    return part


def layernorm_bwd(dy, xs, w, mean, rstd, dx=None, accumulate=False, want_wgrad=False, partial_rows=None,
                  copy_dtype=None):
    """-> (dx, dw, db[, dx_copy]).  dx f32; accumulate=True adds into the given dx; copy_dtype: also
    return the final dx converted to that dtype (operand of the next GEMM)."""
    _chk(dy, torch.float32, "dy"); _chk(xs, torch.float32, "xs")
    D = xs.shape[-1]
    M = xs.numel() // D
    if dx is None:
        dx = torch.empty_like(xs)
        accumulate = False
    dwp = dbp = None
    if partial_rows is None:
        # one wave per partial row walks M / partial_rows rows: enough waves to fill the chip (256 partial rows left the
        # 32 832-row LayerNorm backwards of C3 on 64 workgroups, 0.4 ms each), at most ~16 rows per wave
        partial_rows = max(256, min(4096, (M + 15) // 16))
    if want_wgrad:
        dwp = torch.empty((partial_rows, D), dtype=torch.float32, device=xs.device)
        dbp = torch.empty((partial_rows, D), dtype=torch.float32, device=xs.device)
    cp = torch.empty(xs.shape, dtype=copy_dtype, device=xs.device) if copy_dtype is not None else None
    _lib.check(_lib.lib().ppt_layernorm_bwd(_p(dy), _p(xs), _p(w), _p(mean), _p(rstd), _p(dx), int(accumulate),
                                            _p(cp), dtype_code(cp) if cp is not None else 0,
                                            _p(dwp), _p(dbp), partial_rows, M, D, _stream()), "ppt_layernorm_bwd")
    dw, db = (reduce_rows(dwp), reduce_rows(dbp)) if want_wgrad else (None, None)
    return (dx, dw, db, cp) if copy_dtype is not None else (dx, dw, db)


def _attn_split16(qkv):
    """split16 mode: fp32 q / k / v with every product from hi + lo half pairs on the matrix pipe"""
    return qkv.dtype == torch.float32 and _SPLIT16 and ATTN_SPLIT16


def _attn_pairs(n_seq, T, P, causal):
    """(query, key) pairs per head of n_seq sequences of T positions whose first P (causal only) are stored and computed once"""
    return n_seq * (T * T - P * P) + P * P if causal else 2 * n_seq * T * T


def _attention_fwd(qkv, n_seq, T, P, H, scale, causal, want_lse):
    """plain (P == 0: rows = n_seq * T, lse [n_seq, H, T]) or prefix-shared (P > 0, causal: lse [rows, H]) forward"""
    _chk(qkv, None, "qkv")
    rows = prefix_rows(n_seq, T, P)
    assert not P or qkv.shape[0] == rows
    out = torch.empty((rows, H * 64), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((rows, H) if P else (n_seq, H, T), dtype=torch.float32, device=qkv.device) if want_lse else None
    if profiler is not None:
        profiler.begin("attention_fwd", 2.0 * _attn_pairs(n_seq, T, P, causal) * H * 64)
    L = _lib.lib()
    if _attn_split16(qkv):
        _lib.check(L.ppt_attention_fwd_split16(_p(qkv), _p(out), _p(lse), n_seq, T, P, H, 64, scale, int(causal), _stream()),
                   "ppt_attention_fwd_split16")
    elif P:
        _lib.check(L.ppt_attention_prefix_fwd(_p(qkv), _p(out), _p(lse), n_seq, T, P, H, 64, scale, dtype_code(qkv), _stream()),
                   "ppt_attention_prefix_fwd")
    else:
        _lib.check(L.ppt_attention_fwd(_p(qkv), _p(out), _p(lse), n_seq, T, H, 64, scale, int(causal), dtype_code(qkv), _stream()),
                   "ppt_attention_fwd")
    if profiler is not None:
        profiler.end()
    if probe is not None:
        _probe("attention", out)
    return out, lse


def _attention_bwd(qkv, out, dout, lse, n_seq, T, P, H, scale, causal):
    _chk(qkv, None, "qkv"); _chk(out, qkv.dtype, "out"); _chk(dout, qkv.dtype, "dout")
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((prefix_rows(n_seq, T, P), H) if P else (n_seq, H, T), dtype=torch.float32, device=qkv.device)
    L = _lib.lib()
    ws = torch.empty((L.ppt_attention_prefix_workspace_bytes(n_seq, P, H, 64) // 4,), dtype=torch.float32, device=qkv.device) if P else None
    if profiler is not None:
        profiler.begin("attention_bwd", 5.0 * _attn_pairs(n_seq, T, P, causal) * H * 64)
    if _attn_split16(qkv):
        _lib.check(L.ppt_attention_bwd_split16(_p(qkv), _p(out), _p(dout), _p(lse), _p(delta), _p(dqkv), _p(ws), n_seq, T, P, H, 64,
                                               scale, int(causal), _stream()), "ppt_attention_bwd_split16")
    elif P:
        _lib.check(L.ppt_attention_prefix_bwd(_p(qkv), _p(out), _p(dout), _p(lse), _p(delta), _p(dqkv), _p(ws), n_seq, T, P, H, 64,
                                              scale, dtype_code(qkv), _stream()), "ppt_attention_prefix_bwd")
    else:
        _lib.check(L.ppt_attention_bwd(_p(qkv), _p(out), _p(dout), _p(lse), _p(delta), _p(dqkv), n_seq, T, H, 64,
                                       scale, int(causal), dtype_code(qkv), _stream()), "ppt_attention_bwd")
    if profiler is not None:
        profiler.end()
    return dqkv


def attention_fwd(qkv, Bt, T, H, scale, causal, want_lse=True):
    """qkv [Bt*T, 3*H*64] -> out [Bt*T, H*64], lse [Bt,H,T] f32."""
    return _attention_fwd(qkv, Bt, T, 0, H, scale, causal, want_lse)


def attention_bwd(qkv, out, dout, lse, Bt, T, H, scale, causal):
    return _attention_bwd(qkv, out, dout, lse, Bt, T, 0, H, scale, causal)


def prefix_rows(C, T, P):
    """rows of the prefix-shared layout (include/ppt_hip.h, ppt_attention_prefix_fwd): P shared + C * (T - P)."""
    return P + C * (T - P)


def attention_prefix_fwd(qkv, C, T, P, H, scale, want_lse=True):
    """causal attention over C prompts of T positions sharing their first P: qkv [P + C(T-P), 3*H*64] ->
    (out [rows, H*64], lse [rows, H] f32)."""
    return _attention_fwd(qkv, C, T, P, H, scale, True, want_lse)


def attention_prefix_bwd(qkv, out, dout, lse, C, T, P, H, scale):
    return _attention_bwd(qkv, out, dout, lse, C, T, P, H, scale, True)


def conv1_stats(pts, w1, b1):
    """partial (sum, sumsq) of y = w1.p + b1 over points [M,3] -> ([P,C], [P,C])."""
    _chk(pts, torch.float32, "pts")
    M = pts.shape[0]
    C = w1.shape[0]
    P = _lib.lib().ppt_conv1_stats_max_partials(M)
    ps = torch.empty((P, C), dtype=torch.float32, device=pts.device)
    pq = torch.empty((P, C), dtype=torch.float32, device=pts.device)
    n = ctypes.c_int(0)
    _lib.check(_lib.lib().ppt_conv1_stats(_p(pts), M, _p(w1), _p(b1), C, _p(ps), _p(pq), ctypes.byref(n), _stream()),
               "ppt_conv1_stats")
    return ps, pq, _lib.lib().ppt_conv1_stats_rows_per_partial()


def bn_finalize(gamma, beta, train, partials=None, rows_per_partial=0, count=0, running_mean=None, running_var=None,
                num_batches_tracked=None, eps=1e-5, momentum=0.1, update_running=True, want_moments=False):
    """-> (scale, shift) f32 [C] (+ (mean, rstd) with want_moments); updates the running buffers in place when train."""
    C = gamma.shape[0]
    mean = torch.empty((C,), dtype=torch.float32, device=gamma.device) if want_moments else None
    rstd = torch.empty((C,), dtype=torch.float32, device=gamma.device) if want_moments else None
    scale = torch.empty((C,), dtype=torch.float32, device=gamma.device)
    shift = torch.empty((C,), dtype=torch.float32, device=gamma.device)
    ps, pq = partials if partials is not None else (None, None)
    upd = train and update_running
    P = 0 if ps is None else ps.shape[0]
    wbytes = _lib.lib().ppt_bn_finalize_workspace_bytes(P, C) if train else 0
    ws = torch.empty((wbytes // 8,), dtype=torch.float64, device=gamma.device) if wbytes else None
    _lib.check(_lib.lib().ppt_bn_finalize_ws(_p(ps), _p(pq), P, rows_per_partial, count, C, _p(gamma),
                                             _p(beta), eps, int(train), momentum,
                                             _p(running_mean) if (upd or not train) else None,
                                             _p(running_var) if (upd or not train) else None,
                                             _p(num_batches_tracked) if upd else None, _p(scale), _p(shift), _p(mean), _p(rstd),
                                             _p(ws), wbytes, _stream()),
               "ppt_bn_finalize_ws")
    return (scale, shift, mean, rstd) if want_moments else (scale, shift)


def rows_stats(x):
    """x [M,C] f32 -> ((sum, M2) partials [P,C], rows per partial) for bn_finalize."""
    _chk(x, torch.float32, "x")
    M, C = x.shape
    rpp = _lib.lib().ppt_rows_stats_rows_per_partial()
    P = (M + rpp - 1) // rpp
    ps = torch.empty((P, C), dtype=torch.float32, device=x.device)
    pq = torch.empty_like(ps)
    _lib.check(_lib.lib().ppt_rows_stats_f32(_p(x), M, C, _p(ps), _p(pq), _stream()), "ppt_rows_stats_f32")
    return (ps, pq), rpp


def bn_rows_backward(dy, x, scale, shift, mean, rstd, relu, batch_stats, want_dx=True, want_bf16=False, half_dtype=torch.bfloat16):
    """BatchNorm1d(+ReLU) backward over rows: -> (dx [M,C] f32 | None, d gamma [C], d beta [C][, dx in half_dtype (bf16 | f16)])."""
    _chk(dy, torch.float32, "dy"); _chk(x, torch.float32, "x")
    M, C = x.shape
    rpp = _lib.lib().ppt_rows_stats_rows_per_partial()
    P = (M + rpp - 1) // rpp
    pg = torch.empty((P, C), dtype=torch.float32, device=x.device)
    pgx = torch.empty_like(pg)
    _lib.check(_lib.lib().ppt_bn_rows_bwd_reduce(_p(dy), _p(x), _p(scale), _p(shift), _p(mean), _p(rstd), int(relu), M, C,
                                                 _p(pg), _p(pgx), _stream()), "ppt_bn_rows_bwd_reduce")
    sg, sgx = reduce_rows(pg), reduce_rows(pgx)
    dx = torch.empty_like(x) if want_dx else None
    dxb = torch.empty(x.shape, dtype=half_dtype, device=x.device) if want_bf16 else None
    _lib.check(_lib.lib().ppt_bn_rows_bwd_apply(_p(dy), _p(x), _p(scale), _p(shift), _p(mean), _p(rstd), _p(sg), _p(sgx),
                                                int(relu), int(batch_stats), M, C, _p(dx), _p(dxb), _DT[half_dtype], _stream()),
               "ppt_bn_rows_bwd_apply")
    return (dx, sgx, sg, dxb) if want_bf16 else (dx, sgx, sg)


def three_nn_interp(points1, points2, idx, dist, out_dtype, mult):
    """ppt_three_nn_interp_fwd: rows [B*N, ld] = [points1 | sum_j w_j points2[idx_j] | 0], ld = D1 + D2 rounded up to `mult`
    (the K alignment of the GEMM that reads them), in out_dtype; -> (rows, normalised weights [B,N,3] f32)."""
    _chk(points2, torch.float32, "points2"); _chk(idx, torch.int64, "idx"); _chk(dist, torch.float32, "dist")
    _chk(points1, torch.float32, "points1")
    B, N, _ = idx.shape
    S, D2 = points2.shape[1], points2.shape[2]
    D1 = 0 if points1 is None else points1.shape[2]
    ld = (D1 + D2 + mult - 1) // mult * mult
    rows = torch.empty((B * N, ld), dtype=out_dtype, device=points2.device)
    w = torch.empty((B, N, 3), dtype=torch.float32, device=points2.device)
    _lib.check(_lib.lib().ppt_three_nn_interp_fwd(_p(points1), D1, _p(points2), D2, _p(idx), _p(dist), B, N, S, _p(rows),
                                                  dtype_code(rows), ld, _p(w), _stream()), "ppt_three_nn_interp_fwd")
    return rows, w


def scatter_rows_bwd(idx, weight, d_rows, col_off, rows_div, S, C):
    """ppt_scatter_rows_bwd: idx [B,E] i64 (E entries per cloud), weight [B,E] f32 | None, d_rows [B * E / rows_div, ld] f32
    -> d_src [B,S,C] f32 = sum of the (weighted) gradient rows of the entries that gathered source s, ascending entry order."""
    _chk(idx, torch.int64, "idx"); _chk(weight, torch.float32, "weight"); _chk(d_rows, torch.float32, "d_rows")
    B = idx.shape[0]
    E = idx.numel() // B
    out = torch.empty((B, S, C), dtype=torch.float32, device=d_rows.device)
    _lib.check(_lib.lib().ppt_scatter_rows_bwd(_p(idx), _p(weight), _p(d_rows), d_rows.shape[1], col_off, B, E, rows_div, S, C,
                                               _p(out), _stream()), "ppt_scatter_rows_bwd")
    return out


def three_nn_interp_packed(cloud_cols, points1, points2, idx, dist, offsets, out_dtype, mult):
    """ppt_three_nn_interp_packed_fwd: three_nn_interp on the R packed rows of a ragged batch.  idx / dist [R,3] (knn_group with
    query_lengths), points2 [B,S,D2], offsets [B+1] i32; the points1 columns are [cloud_cols[b] | points1[b, n]] with cloud_cols
    [B,Dc] | None one row per cloud and points1 [B,Nmax,Dp] | None a PADDED slab -- neither is ever packed.
    -> (rows [R, ld] in out_dtype, normalised weights [R,3] f32)."""
    _chk(points2, torch.float32, "points2"); _chk(idx, torch.int64, "idx"); _chk(dist, torch.float32, "dist")
    _chk(points1, torch.float32, "points1"); _chk(cloud_cols, torch.float32, "cloud_cols")
    R = idx.shape[0]
    B, S, D2 = points2.shape
    _chk_offsets(offsets, B)
    assert tuple(idx.shape) == (R, 3) and tuple(dist.shape) == (R, 3)
    Dc = 0 if cloud_cols is None else cloud_cols.shape[1]
    Dp = 0 if points1 is None else points1.shape[2]
    assert cloud_cols is None or cloud_cols.shape[0] == B
    assert points1 is None or points1.shape[0] == B
    assert points1 is not None or cloud_cols is None, "the slab gives the row stride: cloud_cols alone is not supported"
    Nmax = points1.shape[1] if points1 is not None else R
    ld = (Dc + Dp + D2 + mult - 1) // mult * mult
    rows = torch.empty((R, ld), dtype=out_dtype, device=points2.device)
    w = torch.empty((R, 3), dtype=torch.float32, device=points2.device)
    if profiler is not None:
        profiler.begin("three_nn_interp_packed", float(R) * (36 + 12 * D2 + ld * rows.element_size() + 12))
    _lib.check(_lib.lib().ppt_three_nn_interp_packed_fwd(_p(cloud_cols), Dc, _p(points1), Dp, _p(points2), D2, _p(idx), _p(dist),
                                                         _p(offsets), B, Nmax, R, S, _p(rows), dtype_code(rows), ld, _p(w),
                                                         _stream()), "ppt_three_nn_interp_packed_fwd")
    if profiler is not None:
        profiler.end()
    return rows, w


def scatter_rows_packed_bwd(idx, weight, d_rows, col_off, rows_div, offsets, S, C):
    """ppt_scatter_rows_packed_bwd: scatter_rows_bwd for packed rows.  idx [R * rows_div] i64 (rows_div entries per packed row),
    weight like it | None, d_rows [R, ld] f32, offsets [B+1] i32 -> d_src [B,S,C] f32; cloud b's sources take the entries of its
    own rows only, in ascending order."""
    _chk(idx, torch.int64, "idx"); _chk(weight, torch.float32, "weight"); _chk(d_rows, torch.float32, "d_rows")
    B = offsets.numel() - 1
    _chk_offsets(offsets, B)
    R = d_rows.shape[0]
    assert idx.numel() == R * rows_div and (weight is None or weight.numel() == R * rows_div)
    out = torch.empty((B, S, C), dtype=torch.float32, device=d_rows.device)
    _lib.check(_lib.lib().ppt_scatter_rows_packed_bwd(_p(idx), _p(weight), _p(d_rows), d_rows.shape[1], col_off, _p(offsets), B, R,
                                                      rows_div, S, C, _p(out), _stream()), "ppt_scatter_rows_packed_bwd")
    return out


def pack_rows(padded, offsets, total_rows):
    """padded [B, Nmax, ...] -> packed [R, ...]: cloud b's first offsets[b+1] - offsets[b] rows, in order; nothing behind them is
    read (ppt_pack_rows; any dtype).  The backward of unpack_rows."""
    assert padded.is_contiguous() and padded.dim() >= 2
    B, Nmax = padded.shape[:2]
    _chk_offsets(offsets, B)
    R = int(total_rows)
    out = torch.empty((R,) + tuple(padded.shape[2:]), dtype=padded.dtype, device=padded.device)
    row_bytes = out[0].numel() * out.element_size()
    if profiler is not None:
        profiler.begin("pack_rows", 2.0 * R * row_bytes)
    _lib.check(_lib.lib().ppt_pack_rows(_p(padded), _p(out), _p(offsets), B, Nmax, R, row_bytes, _stream()), "ppt_pack_rows")
    if profiler is not None:
        profiler.end()
    return out


def unpack_rows(packed, offsets, Nmax):
    """packed [R, ...] -> padded [B, Nmax, ...] with ZERO rows behind every cloud's end (ppt_unpack_rows; any dtype).  The
    backward of pack_rows."""
    assert packed.is_contiguous() and packed.dim() >= 1
    B = offsets.numel() - 1
    _chk_offsets(offsets, B)
    R = packed.shape[0]
    out = torch.empty((B, int(Nmax)) + tuple(packed.shape[1:]), dtype=packed.dtype, device=packed.device)
    row_bytes = packed[0].numel() * packed.element_size()
    if profiler is not None:
        profiler.begin("unpack_rows", float(R + B * int(Nmax)) * row_bytes)
    _lib.check(_lib.lib().ppt_unpack_rows(_p(packed), _p(out), _p(offsets), B, int(Nmax), R, row_bytes, _stream()), "ppt_unpack_rows")
    if profiler is not None:
        profiler.end()
    return out


def sum_groups(x, k):
    """x [G*k, C] f32 -> [G, C]: sums of each k consecutive rows."""
    _chk(x, torch.float32, "x")
    C = x.shape[-1]
    G = x.numel() // (k * C)
    out = torch.empty((G, C), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().ppt_sum_groups(_p(x), G, k, C, _p(out), _stream()), "ppt_sum_groups")
    return out


def gather_add(P, Q, idx, Nsrc, y_dtype, want_stats=True):
    """y[b,s,k,:] = P[b*Nsrc + idx[b,s,k], :] + Q[b*S + s, :] -> (y [B*S*K, C], (psum, pm2) | None)."""
    _chk(P, torch.float32, "P"); _chk(Q, torch.float32, "Q"); _chk(idx, torch.int64, "idx")
    B, S, K = idx.shape
    C = P.shape[1]
    M = B * S * K
    y = torch.empty((M, C), dtype=y_dtype, device=P.device)
    ps = pm = None
    if want_stats:
        ps = torch.empty(((M + 31) // 32, C), dtype=torch.float32, device=P.device)
        pm = torch.empty_like(ps)
    _lib.check(_lib.lib().ppt_gather_add(_p(P), dtype_code(P), _p(Q), _p(idx), B, Nsrc, S, K, C, _p(y), dtype_code(y),
                                         _p(ps), _p(pm), _stream()), "ppt_gather_add")
    return y, ((ps, pm) if want_stats else None)


def pool_finish(pmax, pmin, fold, scale, shift, out):
    """out[g, :C] = relu(scale * (scale >= 0 ? max : min) + shift) folded over `fold` pooled rows; out is a 2-D
    view (row stride free) -- e.g. a column slice of the concatenated MSG feature matrix."""
    G = pmax.shape[0] // fold
    C = pmax.shape[1]
    assert out.shape[0] == G and out.shape[1] == C and out.stride(1) == 1
    _lib.check(_lib.lib().ppt_pool_finish(_p(pmax), _p(pmin), dtype_code(pmax), G, fold, C, _p(scale), _p(shift), _p(out),
                                          dtype_code(out), out.stride(0), _stream()), "ppt_pool_finish")
    return out


def bn_act_rows(x, scale, shift, y_dtype, mask=None):
    _chk(x, torch.float32, "x")
    M, C = x.shape
    y = torch.empty((M, C), dtype=y_dtype, device=x.device)
    _lib.check(_lib.lib().ppt_bn_act_rows(_p(x), M, C, _p(scale), _p(shift), _p(mask), _p(y), dtype_code(y), _stream()),
               "ppt_bn_act_rows")
    return y


def ball_query_lt(xyz, center, radius, K, want_grouped=False):
    """The ball query of PointNeXt's compiled extension (ppt_ball_query_lt_f32): first K indices in ascending order with the
    direct-form fp32 distance (dx*dx + dy*dy) + dz*dz < float32(radius) * float32(radius), padded with the first hit, all 0 when
    nothing hits.  xyz [B,N,3], center [B,S,3] -> idx [B,S,K] i64 [, grouped_xyz [B,S,K,3] = xyz[idx] - center]."""
    _chk(xyz, torch.float32, "xyz"); _chk(center, torch.float32, "center")
    import numpy as np
    B, N, _ = xyz.shape
    S = center.shape[1]
    idx = torch.empty((B, S, K), dtype=torch.int64, device=xyz.device)
    g = torch.empty((B, S, K, 3), dtype=torch.float32, device=xyz.device) if want_grouped else None
    r2 = float(np.float32(radius) * np.float32(radius))
    if profiler is not None:
        profiler.begin("ball_query", float(B) * (12 * N + 12 * S + 8 * S * K + (12 * S * K if want_grouped else 0)))
    _lib.check(_lib.lib().ppt_ball_query_lt_f32(_p(xyz), _p(center), B, N, S, r2, K, _p(idx), _p(g), _stream()),
               "ppt_ball_query_lt_f32")
    if profiler is not None:
        profiler.end()
    return (idx, g) if want_grouped else idx


def pool_res_finish(pmax, pmin, fold, scale, shift, identity, out_dtype):
    """out[g] = relu((scale * (scale >= 0 ? max : min) + shift) + identity[g]) folded over `fold` pooled rows (ppt_pool_res_finish):
    pmax / pmin [G * fold, C] f32, identity [G, C] f32 | None -> [G, C] in out_dtype."""
    _chk(pmax, torch.float32, "pmax"); _chk(pmin, torch.float32, "pmin"); _chk(identity, torch.float32, "identity")
    _chk(scale, torch.float32, "scale"); _chk(shift, torch.float32, "shift")
    C = pmax.shape[1]
    G = pmax.shape[0] // fold
    assert pmax.shape[0] == G * fold and pmin.shape == pmax.shape and (identity is None or tuple(identity.shape) == (G, C))
    out = torch.empty((G, C), dtype=out_dtype, device=pmax.device)
    _lib.check(_lib.lib().ppt_pool_res_finish(_p(pmax), _p(pmin), G, fold, C, _p(scale), _p(shift), _p(identity), _p(out),
                                              dtype_code(out), _stream()), "ppt_pool_res_finish")
    return out


def cloud_height(pc):
    """data/dataset_3d.py:311-314 (use_height): pc [B,N,3] f32 -> [B,N,4] f32, column 3 = y - min over the cloud of y."""
    _chk(pc, torch.float32, "pc")
    B, N, C = pc.shape
    assert C == 3
    out = torch.empty((B, N, 4), dtype=torch.float32, device=pc.device)
    _lib.check(_lib.lib().ppt_cloud_height_f32(_p(pc), B, N, _p(out), _stream()), "ppt_cloud_height_f32")
    return out


def gn_lrelu_max_forward(y, gamma, beta, groups, eps, slope):
    """y [B,Q,K,C] f32 -> (out [B,Q,C], arg [B,Q,C] i32, mean [B,G], rstd [B,G]): GroupNorm(groups) + LeakyReLU(slope) +
    max over K (DGCNN_Propagation, pointbert/pointnet2_utils.py:371-467)."""
    _chk(y, torch.float32, "y")
    B, Q, K, C = y.shape
    L = _lib.lib()
    nch = L.ppt_gn_stats_chunks(Q * K)
    part = torch.empty((B, nch, groups, 2), dtype=torch.float64, device=y.device)
    _lib.check(L.ppt_gn_stats(_p(y), B, Q * K, C, groups, _p(part), _stream()), "ppt_gn_stats")
    n = float(Q * K * (C // groups))
    mean = torch.empty((B, groups), dtype=torch.float32, device=y.device)
    rstd = torch.empty((B, groups), dtype=torch.float32, device=y.device)
    _lib.check(L.ppt_gn_finish(_p(part), B, nch, groups, n, float(eps), 0, _p(mean), _p(rstd), _stream()), "ppt_gn_finish")   # biased, as nn.GroupNorm
    out = torch.empty((B, Q, C), dtype=torch.float32, device=y.device)
    arg = torch.empty((B, Q, C), dtype=torch.int32, device=y.device)
    _lib.check(L.ppt_gn_lrelu_max(_p(y), _p(mean), _p(rstd), _p(gamma), _p(beta), B, Q, K, C, groups, slope, _p(out), _p(arg),
                                  _stream()), "ppt_gn_lrelu_max")
    return out, arg, mean, rstd


def gn_lrelu_max_backward(y, dout, out, arg, mean, rstd, gamma, groups, slope):
    """-> (dy [B,Q,K,C], dgamma [C], dbeta [C])."""
    _chk(y, torch.float32, "y"); _chk(dout, torch.float32, "dout")
    B, Q, K, C = y.shape
    L = _lib.lib()
    nch = L.ppt_gn_bwd_chunks(Q)
    psum = torch.empty((B, nch, groups, 2), dtype=torch.float64, device=y.device)
    pgb = torch.empty((B, nch, C, 2), dtype=torch.float32, device=y.device)
    _lib.check(L.ppt_gn_bwd_sums(_p(y), _p(dout), _p(out), _p(arg), _p(mean), _p(rstd), _p(gamma), B, Q, K, C, groups, slope,
                                 _p(psum), _p(pgb), _stream()), "ppt_gn_bwd_sums")
    n = float(Q * K * (C // groups))
    s12n = torch.empty((B, groups, 2), dtype=torch.float32, device=y.device)
    _lib.check(L.ppt_gn_finish(_p(psum), B, nch, groups, n, 0.0, 1, _p(s12n), None, _stream()), "ppt_gn_finish")
    gb = reduce_rows(pgb.view(B * nch, 2 * C))                        # [2C] interleaved (dgamma, dbeta)
    dy = torch.empty_like(y)
    _lib.check(L.ppt_gn_bwd_apply(_p(y), _p(dout), _p(out), _p(arg), _p(mean), _p(rstd), _p(gamma), _p(s12n), B, Q, K, C, groups,
                                  slope, _p(dy), _stream()), "ppt_gn_bwd_apply")
    gb = gb.view(C, 2)
    return dy, gb[:, 0].contiguous(), gb[:, 1].contiguous()


def mini_pointnet_conv12(pts, w1, b1, a_scale, a_shift, w2, bias2):
    """pts [M,3] f32 -> (y2 [M,256] bf16, gmax [M/32,256] bf16): conv1 + folded BN + ReLU + conv2 + bias and the max over
    each group of 32 rows, one kernel (ppt_mini_pointnet_conv12_bf16).  w2 [256,128] bf16."""
    assert w2.dtype in HALF
    _chk(pts, torch.float32, "pts"); _chk(w2, w2.dtype, "w2")
    M = pts.shape[0]
    N, C1 = w2.shape
    y2 = torch.empty((M, N), dtype=w2.dtype, device=pts.device)
    gmax = torch.empty((M // 32, N), dtype=w2.dtype, device=pts.device)
    if profiler is not None:
        profiler.begin("gemm_bf16", 2.0 * M * N * C1, "ppt_mini_pointnet_conv12_bf16")
    _lib.check(_lib.lib().ppt_mini_pointnet_conv12_half(_p(pts), M, _p(w1), _p(b1), _p(a_scale), _p(a_shift), C1, _p(w2), _p(bias2),
                                                        N, _p(y2), _p(gmax), dtype_code(w2), _stream()), "ppt_mini_pointnet_conv12_half")
    if profiler is not None:
        profiler.end()
    if probe is not None:
        _probe("mini-PointNet conv2 output (pre-BN)", y2)
    return y2, gmax


def mini_pointnet_conv3(A, w, gterm, col_stats=None, store=True):
    """A [M,256] bf16, w [512,256] bf16, gterm [M/32,512] f32 -> y [M,512] bf16 = A @ w^T + gterm[group] (+ BatchNorm partials
    into col_stats) -- ppt_mini_pointnet_conv3_bf16.  The FLOPs are accounted at the 512-wide conv this is the local half of.
    store=False: the statistics pass alone (y is not written; returns None)."""
    assert w.dtype in HALF
    _chk(A, w.dtype, "A"); _chk(w, w.dtype, "w"); _chk(gterm, torch.float32, "gterm")
    M, K = A.shape
    N = w.shape[0]
    assert store or col_stats is not None
    y = torch.empty((M, N), dtype=w.dtype, device=A.device) if store else None
    ps, pm = col_stats if col_stats is not None else (None, None)
    if profiler is not None:
        # model: the 512-wide Conv1d on cat(global, local) (dvae.py:194); executed: the local half (the global half is one row
        # per group, a separate small GEMM booked with algo_k = 0 / its own executed FLOPs)
        profiler.begin("gemm_bf16", 2.0 * M * N * 2 * K, "ppt_mini_pointnet_conv3_bf16", executed=2.0 * M * N * K)
    _lib.check(_lib.lib().ppt_mini_pointnet_conv3_half(_p(A), M, K, _p(w), _p(gterm), N, _p(y), _p(ps), _p(pm), dtype_code(w), _stream()),
               "ppt_mini_pointnet_conv3_half")
    if profiler is not None:
        profiler.end()
    if probe is not None:
        _probe("mini-PointNet conv3 output (pre-BN)", y)
    return y


def mpn34_retile(w4):
    """W4 [256,512] 16-bit -> the fragment order csrc/mpn34.hip streams (ppt_mpn34_retile)."""
    assert w4.dtype in HALF and tuple(w4.shape) == (256, 512)
    _chk(w4, w4.dtype, "w4")
    out = torch.empty_like(w4)
    _lib.check(_lib.lib().ppt_mpn34_retile(_p(w4), _p(out), _stream()), "ppt_mpn34_retile")
    return out


def mini_pointnet_conv34(y2, w3s, gs, w4_tiled, bias4):
    """tok [M/32,256] = max over each group of 32 rows of relu(y2 @ w3s^T + gs[group]) @ w4^T + bias4, the [M,512] intermediate
    never leaving the chip (ppt_mini_pointnet_conv34_half).  y2 [M,256], w3s [512,256] (BatchNorm scale folded in), w4_tiled from
    mpn34_retile, all one 16-bit format; gs [M/32,512] f32."""
    T = w3s.dtype
    assert T in HALF and tuple(w3s.shape) == (512, 256) and w4_tiled.dtype == T and w4_tiled.numel() == 256 * 512
    _chk(y2, T, "y2"); _chk(w3s, T, "w3s"); _chk(w4_tiled, T, "w4_tiled"); _chk(gs, torch.float32, "gs")
    M = y2.shape[0]
    assert y2.shape[1] == 256 and tuple(gs.shape) == (M // 32, 512) and M % 32 == 0
    tok = torch.empty((M // 32, 256), dtype=T, device=y2.device)
    if profiler is not None:
        # model: the 512-wide conv3 on cat(global, local) + conv4; executed: the local half of conv3 (17 k-steps) + conv4
        profiler.begin("gemm_bf16", 2.0 * M * 512 * 512 + 2.0 * M * 256 * 512, "ppt_mini_pointnet_conv34_half",
                       executed=2.0 * M * 512 * 272 + 2.0 * M * 256 * 512)
    _lib.check(_lib.lib().ppt_mini_pointnet_conv34_half(_p(y2), M, _p(w3s), _p(gs), _p(w4_tiled), _p(bias4), _p(tok), dtype_code(T), _stream()),
               "ppt_mini_pointnet_conv34_half")
    if profiler is not None:
        profiler.end()
    if probe is not None:
        _probe("mini-PointNet tokens", tok)
    return tok


def mini_pointnet_conv4(A, a_scale, a_shift, w, bias):
    """A [M,512] bf16 -> tok [M/32,256] bf16 = max over each group of 32 rows of relu(a_scale*A + a_shift) @ w^T + bias
    (ppt_mini_pointnet_conv4_bf16)."""
    assert w.dtype in HALF
    _chk(A, w.dtype, "A"); _chk(w, w.dtype, "w")
    M, K = A.shape
    N = w.shape[0]
    tok = torch.empty((M // 32, N), dtype=w.dtype, device=A.device)
    if profiler is not None:
        profiler.begin("gemm_bf16", 2.0 * M * N * K, "ppt_mini_pointnet_conv4_bf16")
    _lib.check(_lib.lib().ppt_mini_pointnet_conv4_half(_p(A), M, K, _p(a_scale), _p(a_shift), _p(w), _p(bias), N, _p(tok), dtype_code(w),
                                                       _stream()), "ppt_mini_pointnet_conv4_half")
    if profiler is not None:
        profiler.end()
    if probe is not None:
        _probe("mini-PointNet tokens", tok)
    return tok


CONV12_STATS_SHAPES = {(32, 32), (64, 64), (64, 96), (64, 128), (128, 128)}      # (C1, N) ppt_conv12_stats_bf16 is built for


def conv12_stats(pts, w1, b1, a_scale, a_shift, w2, bias2):
    """pts [M,3] f32 -> (y2 [M,N] bf16, (part_sum, part_m2) [M/32, N]): conv1 + folded BN + ReLU + conv2 (+ bias) with the
    BatchNorm partials of the output, one barrier-free kernel (ppt_conv12_stats_bf16).  w2 [N,C1] bf16."""
    _chk(pts, torch.float32, "pts"); _chk(w2, torch.bfloat16, "w2")
    M = pts.shape[0]
    N, C1 = w2.shape
    y2 = torch.empty((M, N), dtype=torch.bfloat16, device=pts.device)
    ps = torch.empty((M // 32, N), dtype=torch.float32, device=pts.device)
    pm = torch.empty_like(ps)
    if profiler is not None:
        profiler.begin("gemm_bf16", 2.0 * M * N * C1, "ppt_conv12_stats_bf16")
    _lib.check(_lib.lib().ppt_conv12_stats_bf16(_p(pts), M, _p(w1), _p(b1), _p(a_scale), _p(a_shift), C1, _p(w2), _p(bias2), N,
                                                _p(y2), _p(ps), _p(pm), _stream()), "ppt_conv12_stats_bf16")
    if profiler is not None:
        profiler.end()
    return y2, (ps, pm)


AFFINE_CONV_POOL_SHAPES = {(32, 64, 16), (64, 128, 32), (96, 128, 64), (128, 256, 64)}     # (K, N, pool_rows)


def affine_conv_pool(A, a_scale, a_shift, w, bias, pool_rows, pmax, pmin, col_stats):
    """relu(a_scale * A + a_shift) @ w^T + bias, not written: BatchNorm partials into col_stats = (sum, M2) [M/32, N] and the
    max / min over every pool_rows rows into pmax / pmin (ppt_affine_conv_pool_bf16)."""
    _chk(A, torch.bfloat16, "A"); _chk(w, torch.bfloat16, "w")
    M, K = A.shape
    N = w.shape[0]
    if profiler is not None:
        profiler.begin("gemm_bf16", 2.0 * M * N * K, "ppt_affine_conv_pool_bf16")
    _lib.check(_lib.lib().ppt_affine_conv_pool_bf16(_p(A), A.stride(0), M, K, _p(a_scale), _p(a_shift), _p(w), _p(bias), N, pool_rows,
                                                    _p(pmax), _p(pmin), _p(col_stats[0]), _p(col_stats[1]), _stream()),
               "ppt_affine_conv_pool_bf16")
    if profiler is not None:
        profiler.end()


def group_anchor_stats(x, idx, anchor, Nsrc):
    """x [B*Nsrc, D] (f32 | bf16), idx [B,S,K], anchor [B,S] -> [B,S,2] f32: (sum, sum of squares) of x[idx] - x[anchor] per
    group (the statistic behind LocalGrouper's per-cloud std, pointMLP.py:170-175)."""
    _chk(x, None, "x"); _chk(idx, torch.int64, "idx"); _chk(anchor, torch.int64, "anchor")
    B, S, K = idx.shape
    out = torch.empty((B, S, 2), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().ppt_group_anchor_stats(_p(x), dtype_code(x), _p(idx), _p(anchor), B, Nsrc, S, K, x.shape[1], _p(out),
                                                 _stream()), "ppt_group_anchor_stats")
    return out


def pointmlp_cloud_rstd(stats, n):
    """stats [B,S,2] f32 (group_anchor_stats) -> r [B] f32 = 1 / (unbiased std over the cloud's n values + 1e-5), fp64 inside
    (pointMLP.py:174-175)."""
    _chk(stats, torch.float32, "stats")
    B, S, _ = stats.shape
    r = torch.empty((B,), dtype=torch.float32, device=stats.device)
    _lib.check(_lib.lib().ppt_pointmlp_cloud_rstd(_p(stats), B, S, float(n), _p(r), _stream()), "ppt_pointmlp_cloud_rstd")
    return r


def pointmlp_pq(PQ, r, cidx, c0, B, N):
    """PQ [B*N, 2C] f32 -> (P [B*N, C] = PQ[:, :C] * r[b], Q [B*S, C] = (c0 + PQ[a, C:]) - P[a], a = b*N + cidx[b, s])."""
    _chk(PQ, torch.float32, "PQ"); _chk(r, torch.float32, "r"); _chk(cidx, torch.int64, "cidx"); _chk(c0, torch.float32, "c0")
    C = PQ.shape[1] // 2
    S = cidx.shape[1]
    P = torch.empty((B * N, C), dtype=torch.float32, device=PQ.device)
    Q = torch.empty((B * S, C), dtype=torch.float32, device=PQ.device)
    _lib.check(_lib.lib().ppt_pointmlp_pq(_p(PQ), _p(r), _p(cidx), _p(c0), _p(P), _p(Q), B, N, S, C, _stream()), "ppt_pointmlp_pq")
    return P, Q


def bn_res_act_rows(x, res, scale, shift, y_dtype, pool=1, res_affine=None):
    """relu(scale * x + shift + res') over rows [M,C]; pool > 1 returns the max over each `pool` consecutive rows.
    res' = res, or relu(rs * res + rh) with res_affine = (rs, rh)."""
    _chk(x, None, "x"); _chk(res, None, "res")
    M, C = x.shape
    assert res.shape == x.shape and M % pool == 0
    y = torch.empty((M // pool, C), dtype=y_dtype, device=x.device)
    rs, rh = res_affine if res_affine is not None else (None, None)
    _lib.check(_lib.lib().ppt_bn_res_act_rows(_p(x), dtype_code(x), _p(res), dtype_code(res), M, C, pool, _p(scale), _p(shift),
                                              _p(rs), _p(rh), _p(y), dtype_code(y), _stream()), "ppt_bn_res_act_rows")
    return y


def linear3_gelu(pts, w, b, y_dtype):
    _chk(pts, torch.float32, "pts")
    M, C = pts.shape[0], w.shape[0]
    y = torch.empty((M, C), dtype=y_dtype, device=pts.device)
    _lib.check(_lib.lib().ppt_linear3_gelu(_p(pts), M, _p(w), _p(b), C, _p(y), dtype_code(y), _stream()),
               "ppt_linear3_gelu")
    if probe is not None:
        _probe("pos_embed hidden", y)
    return y


def cls_max_pool(x, want_argmax=False):
    """x [B,T,D] -> feat [B,2D] f32 (+ argmax [B,D] i32)."""
    _chk(x, None, "x")
    B, T, D = x.shape
    out = torch.empty((B, 2 * D), dtype=torch.float32, device=x.device)
    am = torch.empty((B, D), dtype=torch.int32, device=x.device) if want_argmax else None
    _lib.check(_lib.lib().ppt_cls_max_pool(_p(x), dtype_code(x), B, T, D, _p(out), _p(am), _stream()), "ppt_cls_max_pool")
    return out, am


def convert(src, dst_dtype, scale=1.0):
    """src in another dtype; scale != 1: convert(src * scale) -- the operand copy of an fp32 activation gradient entering a 16-bit
    backward stage, multiplied by the stage's power-of-two gradient scale on the way (ppt_convert_scaled)."""
    _chk(src, None, "src")
    if src.dtype == dst_dtype and scale == 1.0:
        return src
    dst = torch.empty(src.shape, dtype=dst_dtype, device=src.device)
    if scale == 1.0:
        _lib.check(_lib.lib().ppt_convert(_p(src), dtype_code(src), _p(dst), dtype_code(dst), src.numel(), _stream()), "ppt_convert")
    else:
        _lib.check(_lib.lib().ppt_convert_scaled(_p(src), dtype_code(src), _p(dst), dtype_code(dst), src.numel(), float(scale), _stream()),
                   "ppt_convert_scaled")
    return dst


def weights_prep(items, dtype):
    """items: list of (w f32 [N, ld] contiguous 2-D view, col0, K, sub_col0 | None, Kp) -> list of (out [N, Kp], out_t [Kp, N]) in
    `dtype`: convert(w[:, col0:col0+K] (- w[:, sub_col0:sub_col0+K])), zero-padded to Kp columns, and its transpose -- ONE launch for
    all items (ppt_weights_prep)."""
    assert dtype in HALF or dtype == torch.float32
    arr = (_lib.WprepItem * len(items))()
    outs = []
    for a, (w, col0, K, sub, Kp) in zip(arr, items):
        _chk(w, torch.float32, "w")
        assert w.dim() == 2
        N = w.shape[0]
        out = torch.empty((N, Kp), dtype=dtype, device=w.device)
        out_t = torch.empty((Kp, N), dtype=dtype, device=w.device)
        a.w, a.ldw, a.N, a.col0, a.K, a.sub_col0, a.Kp, a.out, a.out_t = _p(w), w.shape[1], N, col0, K, (-1 if sub is None else sub), Kp, _p(out), _p(out_t)
        outs.append((out, out_t))
    _lib.check(_lib.lib().ppt_weights_prep(ctypes.cast(arr, ctypes.c_void_p), len(items), dtype_code(dtype), _stream()), "ppt_weights_prep")
    return outs


def labels_check(labels, n_classes, ignore_index, flags, bit):
    """flags[0] |= bit when a label lies outside [0, n_classes) and is not ignore_index (ppt_labels_check)."""
    _chk(labels, torch.int64, "labels"); _chk(flags, torch.int32, "flags")
    _lib.check(_lib.lib().ppt_labels_check(_p(labels), labels.numel(), int(n_classes), int(ignore_index), _p(flags), int(bit), _stream()),
               "ppt_labels_check")


METRIC_NONFINITE, METRIC_BAD_LABEL = 1, 2          # flag bits of the metric records (include/ppt_hip.h)
CLS_REC, PARTSEG_REC, PARTSEG_MAX_PARTS = 4, 32, 8


def cls_metrics(logits, labels, smoothing, records):
    """logits [B, C] f32, labels [B] i64 -> records [B, 4] i32 (a caller-owned slice): per sample the bits of the row loss of
    nn.CrossEntropyLoss(label_smoothing=smoothing), the rank of the target, the flag bits and the label (ppt_cls_metrics)."""
    _chk(logits, torch.float32, "logits"); _chk(labels, torch.int64, "labels"); _chk(records, torch.int32, "records")
    B, C = logits.shape
    assert labels.shape == (B,) and records.shape == (B, CLS_REC)
    _lib.check(_lib.lib().ppt_cls_metrics(_p(logits), _p(labels), float(smoothing), B, C, _p(records), _stream()), "ppt_cls_metrics")


def partseg_metrics_chunks(N):
    """workgroups one cloud of N points is split over (ppt_partseg_metrics_chunks): the scratch is B * chunks floats"""
    return _lib.lib().ppt_partseg_metrics_chunks(int(N))


def partseg_metrics(logits, labels, smoothing, part_start, part_count, max_parts, records, partial, lengths=None):
    """logits [B, N, P] f32, labels [B, N] i64, part_start / part_count [P] i32 (per part id: its category's first part and
    number of parts; max_parts = the largest count) -> records [B, 32] i32 (a caller-owned slice): per cloud the category's range,
    the correct points, the loss sum and the per-part |gt|, |pred|, |gt and pred| (ppt_partseg_metrics; layout: include/ppt_hip.h).
    partial: scratch of at least B * partseg_metrics_chunks(N) f32.
    lengths [B] i32 (device): N is the row stride and cloud b its first lengths[b] rows -- nothing behind them is counted or
    read, and the record is the one of that cloud alone (ppt_partseg_metrics_ragged)."""
    _chk(logits, torch.float32, "logits"); _chk(labels, torch.int64, "labels"); _chk(records, torch.int32, "records")
    _chk(part_start, torch.int32, "part_start"); _chk(part_count, torch.int32, "part_count"); _chk(partial, torch.float32, "partial")
    B, N, P = logits.shape
    assert labels.shape == (B, N) and records.shape == (B, PARTSEG_REC) and part_start.numel() == P and part_count.numel() == P
    assert partial.numel() >= B * partseg_metrics_chunks(N)
    if lengths is not None:
        _chk_lengths(lengths, B)
        if profiler is not None:
            profiler.begin("partseg_metrics_ragged", float(B) * N * (4 * P + 8))
        _lib.check(_lib.lib().ppt_partseg_metrics_ragged(_p(logits), _p(labels), _p(lengths), float(smoothing), B, N, P,
                                                         _p(part_start), _p(part_count), int(max_parts), _p(records), _p(partial),
                                                         _stream()), "ppt_partseg_metrics_ragged")
        if profiler is not None:
            profiler.end()
        return
    _lib.check(_lib.lib().ppt_partseg_metrics(_p(logits), _p(labels), float(smoothing), B, N, P, _p(part_start), _p(part_count),
                                              int(max_parts), _p(records), _p(partial), _stream()), "ppt_partseg_metrics")


METER_REC, METER_SCRATCH = 8, 4                    # the training meters' record and scratch (include/ppt_hip.h)
METER_KEYS = ("loss_sum", "acc_sum", "weight", "calls", "nonfinite", "last_loss", "last_acc", "bad_labels")


def _meter_args(logits, labels, loss, rec):
    _chk(logits, torch.float32, "logits"); _chk(labels, torch.int64, "labels"); _chk(loss, torch.float32, "loss")
    _chk(rec, torch.float64, "rec")
    assert loss.numel() == 1 and rec.numel() == METER_REC


def train_meter_cls(logits, labels, loss, rec, weight=1.0, metered=True):
    """One training step of main_cls.py:200-217 folded into the epoch's record rec [8] f64 (METER_KEYS; zeroed by the caller at
    the start of the epoch): logits [B, C] f32, labels [B] i64, loss a device fp32 scalar.  One launch, no read (ppt_train_meter_cls)."""
    _meter_args(logits, labels, loss, rec)
    B, C = logits.shape
    assert labels.shape == (B,)
    _lib.check(_lib.lib().ppt_train_meter_cls(_p(logits), _p(labels), _p(loss), B, C, float(weight), int(bool(metered)), _p(rec),
                                              _stream()), "ppt_train_meter_cls")


def train_meter_partseg(logits, labels, loss, part_start, part_count, rec, scratch, weight=1.0, metered=True, lengths=None):
    """One training step of main_partseg.py:218-243 folded into rec [8] f64: logits [B, N, P] f32, labels [B, N] i64, part_start /
    part_count [P] i32 as for partseg_metrics; scratch [4] i32, all zero before the first call and after every call
    (ppt_train_meter_partseg).  lengths [B] i32 (device): only rows < lengths[b] are counted or read and the accuracy's
    denominator is sum(lengths) (ppt_train_meter_partseg_ragged)."""
    _meter_args(logits, labels, loss, rec)
    _chk(part_start, torch.int32, "part_start"); _chk(part_count, torch.int32, "part_count"); _chk(scratch, torch.int32, "scratch")
    B, N, P = logits.shape
    assert labels.shape == (B, N) and part_start.numel() == P and part_count.numel() == P and scratch.numel() >= METER_SCRATCH
    if lengths is not None:
        _chk_lengths(lengths, B)
        _lib.check(_lib.lib().ppt_train_meter_partseg_ragged(_p(logits), _p(labels), _p(lengths), _p(loss), B, N, P, _p(part_start),
                                                             _p(part_count), float(weight), int(bool(metered)), _p(rec),
                                                             _p(scratch), _stream()), "ppt_train_meter_partseg_ragged")
        return
    _lib.check(_lib.lib().ppt_train_meter_partseg(_p(logits), _p(labels), _p(loss), B, N, P, _p(part_start), _p(part_count),
                                                  float(weight), int(bool(metered)), _p(rec), _p(scratch), _stream()),
               "ppt_train_meter_partseg")


def partseg_predict(logits, anchor, part_start, part_count, pred=None):
    """logits [B, N, P] f32, anchor [B] i64 (a part id that names the cloud's category: labels[:, 0]), part_start / part_count
    [P] i32 as for partseg_metrics -> pred [B, N] i32 (caller-owned, allocated when None): the first arg-max over the category's
    part range, plus its start -- the rule partseg_metrics counts by; -1 for a cloud whose anchor is outside [0, P)
    (ppt_partseg_predict)."""
    _chk(logits, torch.float32, "logits"); _chk(anchor, torch.int64, "anchor"); _chk(pred, torch.int32, "pred")
    _chk(part_start, torch.int32, "part_start"); _chk(part_count, torch.int32, "part_count")
    B, N, P = logits.shape
    if pred is None:
        pred = torch.empty((B, N), dtype=torch.int32, device=logits.device)
    assert anchor.shape == (B,) and pred.shape == (B, N) and part_start.numel() == P and part_count.numel() == P
    _lib.check(_lib.lib().ppt_partseg_predict(_p(logits), _p(anchor), B, N, P, _p(part_start), _p(part_count), _p(pred), _stream()),
               "ppt_partseg_predict")
    return pred


RENDER_MAX_RADIUS, RENDER_MAX_IMAGE, RENDER_MAX_POINTS = 16, 4096, 65536        # limits of ppt_render_balls (include/ppt_hip.h)
_BALL_PATTERNS = {}


def ball_pattern_host(radius):
    """The ball of ppt_render_balls as a host array [(2 r - 1)^2, 2] f64, r = max(radius, 1): per offset (dx, dy), row-major over
    dx, the depth dz = sqrt(r^2 - dx^2 - dy^2) and the shade dz / r inside the circle dx^2 + dy^2 < r^2; dz = -1 outside."""
    import numpy as np
    r = max(int(radius), 1)
    d = np.arange(-(r - 1), r, dtype=np.int64)
    rest = r * r - d[:, None] ** 2 - d[None, :] ** 2
    dz = np.sqrt(np.maximum(rest, 0).astype(np.float64))
    table = np.stack([dz, dz / float(r)], -1)
    table[rest <= 0] = (-1.0, 0.0)
    return np.ascontiguousarray(table.reshape(-1, 2))


def _ball_pattern(radius, device):
    key = (max(int(radius), 1), str(device))
    if key not in _BALL_PATTERNS:                   # (host -> device once per radius and device; nothing is read back)
        _BALL_PATTERNS[key] = torch.from_numpy(ball_pattern_host(radius)).to(device)
    return _BALL_PATTERNS[key]


def render_balls_workspace_bytes(G, n, H, W, radius):
    """bytes of scratch ppt_render_balls needs for G geometries of n points on H x W pictures (0: unsupported shape)"""
    return _lib.lib().ppt_render_balls_workspace_bytes(int(G), int(n), int(H), int(W), int(radius))


def render_balls(ixyz, colors, H, W, radius, background=(255, 255, 255), out=None, workspace=None):
    """ixyz [G, n, 3] i32 (row, column, depth), colors [G, K, n, 3] f32 in [0, 255] -> out [G, K, H, W, 3] u8 (caller-owned,
    allocated when None): every point a shaded ball of the given radius, the nearest wins the pixel, equal depths go to the lower
    point index, untouched pixels are `background` (ppt_render_balls; the rule: include/ppt_hip.h).  The visibility of a geometry
    is resolved once for its K colourings.  workspace: a caller-owned uint8 tensor of at least
    render_balls_workspace_bytes(G, n, H, W, radius) bytes (allocated when None)."""
    _chk(ixyz, torch.int32, "ixyz"); _chk(colors, torch.float32, "colors"); _chk(out, torch.uint8, "out")
    _chk(workspace, torch.uint8, "workspace")
    if ixyz.dim() != 3 or ixyz.shape[2] != 3 or colors.dim() != 4 or colors.shape[3] != 3:
        raise RuntimeError("render_balls: ixyz must be [G, n, 3] and colors [G, K, n, 3]")
    G, n, _ = ixyz.shape
    K = colors.shape[1]
    H, W, radius = int(H), int(W), int(radius)
    assert colors.shape[0] == G and colors.shape[2] == n
    bg = bytes(int(c) & 0xFF for c in background)
    assert len(bg) == 3
    need = _lib.lib().ppt_render_balls_workspace_bytes(G, n, H, W, radius)
    if need == 0:
        raise RuntimeError(f"render_balls: unsupported shape G={G} n={n} H={H} W={W} radius={radius} (G, H, W >= 1, radius <= "
                           f"{RENDER_MAX_RADIUS}, H, W <= {RENDER_MAX_IMAGE}, n <= {RENDER_MAX_POINTS})")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=ixyz.device)
    if out is None:
        out = torch.empty((G, K, H, W, 3), dtype=torch.uint8, device=ixyz.device)
    assert out.shape == (G, K, H, W, 3)
    pattern = _ball_pattern(radius, ixyz.device)
    _lib.check(_lib.lib().ppt_render_balls(_p(ixyz) if n else None, _p(colors) if n else None, _p(pattern), bg, radius, G, K, n, H, W,
                                           _p(out), _p(workspace), workspace.numel(), _stream()), "ppt_render_balls")
    return out


LOGREG_INFO = 8                                     # words of a fit's info record (include/ppt_hip.h)
LOGREG_CONVERGED, LOGREG_MAXITER, LOGREG_LINESEARCH, LOGREG_BADINPUT = 0, 1, 2, 3


def _bank(feat, d):
    """(ld, Nbank) of a feature bank [Nbank, >= d] f32 whose rows may be padded (row stride >= d, unit column stride)."""
    if not feat.is_cuda or feat.dtype != torch.float32 or feat.dim() != 2 or feat.stride(1) != 1 or feat.stride(0) < d or feat.shape[1] < d:
        raise RuntimeError("feature bank: expected a CUDA/HIP f32 matrix [N, >= d] with contiguous rows")
    return feat.stride(0), feat.shape[0]


def logreg_fit(feat, labels, rows, C, K, d=None, tol=1e-4, max_iter=1000, workspace=None):
    """F independent L2-regularised multinomial logistic regressions in one launch (ppt_logreg_fit_f32): fit f uses the rows
    rows[f] (int32 [F, n]) of the bank feat [Nbank, ld] f32 with labels [Nbank] i64 and the weight C[f] (a host sequence).
    -> (W [F, K, d] f32, b [F, K] f32, info [F, 8] i32: iterations, evaluations, status, the bits of max |grad F / n| and of
    F / n).  workspace: a caller-owned uint8 tensor of at least logreg_workspace_bytes(F, n, d, K) bytes (allocated when None)."""
    d = feat.shape[1] if d is None else int(d)
    ld, Nbank = _bank(feat, d)
    _chk(labels, torch.int64, "labels"); _chk(rows, torch.int32, "rows")
    F, n = rows.shape
    Cs = [float(c) for c in C]
    assert len(Cs) == F and labels.numel() == Nbank
    need = _lib.lib().ppt_logreg_workspace_bytes(F, n, d, int(K))
    if workspace is None:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=feat.device)
    W = torch.empty((F, K, d), dtype=torch.float32, device=feat.device)
    b = torch.empty((F, K), dtype=torch.float32, device=feat.device)
    info = torch.empty((F, LOGREG_INFO), dtype=torch.int32, device=feat.device)
    _lib.check(_lib.lib().ppt_logreg_fit_f32(_p(feat), ld, Nbank, _p(labels), _p(rows), F, n, d, int(K), (_lib.c_float * F)(*Cs),
                                             float(tol), int(max_iter), _p(W), _p(b), _p(info), _p(workspace), workspace.numel(),
                                             _stream()), "ppt_logreg_fit_f32")
    return W, b, info


def logreg_workspace_bytes(F, n, d, K):
    """bytes of scratch ppt_logreg_fit_f32 needs for F fits of n rows, d features, K classes (0: unsupported shape)"""
    return _lib.lib().ppt_logreg_workspace_bytes(int(F), int(n), int(d), int(K))


def logreg_predict(feat, W, b, rows=None):
    """pred[f, i] = first arg-max over k of W[f, k] . feat[rows[i]] + b[f, k], in fp32 (ppt_logreg_predict_f32).  feat [Nbank, ld]
    f32, W [F, K, d], b [F, K], rows int32 [n_eval] or None (the whole bank) -> pred [F, n_eval] i32 (-1: row outside the bank)."""
    _chk(W, torch.float32, "W"); _chk(b, torch.float32, "b"); _chk(rows, torch.int32, "rows")
    F, K, d = W.shape
    ld, Nbank = _bank(feat, d)
    n_eval = Nbank if rows is None else rows.numel()
    pred = torch.empty((F, n_eval), dtype=torch.int32, device=feat.device)
    _lib.check(_lib.lib().ppt_logreg_predict_f32(_p(feat), ld, Nbank, _p(rows), n_eval, _p(W), _p(b), F, d, K, _p(pred), _stream()),
               "ppt_logreg_predict_f32")
    return pred


def nearest_rows(q, table, k, workspace=None):
    """For each row of q [Q, D] f32 the k rows of table [V, >= D] f32 (padded rows allowed) at the smallest Euclidean distance,
    ascending, ties to the lower row (ppt_nearest_rows_f32: the direct form sqrt(sum (q - t)^2) in fp32).
    -> (idx [Q, k] int32, dist [Q, k] f32).  workspace: a caller-owned uint8 tensor of at least
    nearest_rows_workspace_bytes(Q, V, D, k) bytes (allocated when None)."""
    _chk(q, torch.float32, "q")
    if q.dim() != 2:
        raise RuntimeError("nearest_rows: q must be [Q, D]")
    Q, D = q.shape
    ld, V = _bank(table, D)
    k = int(k)
    need = _lib.lib().ppt_nearest_rows_workspace_bytes(Q, V, D, k)
    if workspace is None:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=q.device)
    idx = torch.empty((Q, k), dtype=torch.int32, device=q.device)
    dist = torch.empty((Q, k), dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().ppt_nearest_rows_f32(_p(q), Q, _p(table), ld, V, D, k, _p(idx), _p(dist), _p(workspace), workspace.numel(),
                                               _stream()), "ppt_nearest_rows_f32")
    return idx, dist


def nearest_rows_workspace_bytes(Q, V, D, k):
    """bytes of scratch ppt_nearest_rows_f32 needs for Q queries, V table rows of D columns and k results (0: unsupported shape)"""
    return _lib.lib().ppt_nearest_rows_workspace_bytes(int(Q), int(V), int(D), int(k))


TSNE_MAX_N, TSNE_MAX_D = 16384, 4096               # limits of ppt_tsne_affinities / ppt_tsne_steps (include/ppt_hip.h)


def tsne_affinities_workspace_bytes(N, D):
    """bytes of scratch ppt_tsne_affinities needs for N rows of D columns (0: unsupported shape)"""
    return _lib.lib().ppt_tsne_affinities_workspace_bytes(int(N), int(D))


def tsne_steps_workspace_bytes(N):
    """bytes of scratch ppt_tsne_steps needs for N points (0: unsupported shape)"""
    return _lib.lib().ppt_tsne_steps_workspace_bytes(int(N))


def tsne_affinities(x, perplexity, d=None, P=None, workspace=None):
    """x [N, >= D] f32 (padded rows allowed) -> (P [N, ldp] f32 -- a view [N, N] of a matrix whose row stride is a multiple of
    four --, beta [N] f32, pstats [2] f64: sum P and sum P log P): the symmetric joint probabilities of exact t-SNE at the given
    perplexity (ppt_tsne_affinities; the statement: include/ppt_hip.h).  P, workspace: caller-owned (allocated when None)."""
    if not x.is_cuda:
        raise RuntimeError("tsne_affinities: x: expected a CUDA/HIP tensor (ppt_amd has no CPU path)")
    D = x.shape[1] if d is None else int(d)
    ld, N = _bank(x, D)
    need = _lib.lib().ppt_tsne_affinities_workspace_bytes(N, D)
    if need == 0:
        raise RuntimeError(f"tsne_affinities: unsupported shape N={N} D={D} (2 <= N <= {TSNE_MAX_N}, 1 <= D <= {TSNE_MAX_D})")
    if P is None:
        P = torch.empty((N, (N + 3) & ~3), dtype=torch.float32, device=x.device)[:, :N]
    if not P.is_cuda or P.dtype != torch.float32 or P.shape != (N, N) or P.stride(1) != 1:
        raise RuntimeError("tsne_affinities: P must be a CUDA/HIP f32 matrix [N, N] with contiguous rows")
    _chk(workspace, torch.uint8, "workspace")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
    beta = torch.empty(N, dtype=torch.float32, device=x.device)
    pstats = torch.empty(2, dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().ppt_tsne_affinities(_p(x), ld, N, D, float(perplexity), _p(P), P.stride(0), _p(beta), _p(pstats), _p(workspace),
                                              workspace.numel(), _stream()), "ppt_tsne_affinities")
    return P, beta, pstats


def tsne_steps(P, pstats, y, update, gains, t0, n, *, t_switch=250, early_exaggeration=12.0, lr, check_every=0, stats=None, grad=None,
               workspace=None):
    """Iterations t0 .. t0 + n - 1 of the t-SNE descent on the state y, update, gains [N, 2] f32 (in place), enqueued by one call
    (ppt_tsne_steps): exaggeration `early_exaggeration` and momentum 0.5 while t < t_switch, then 1 and 0.8.  check_every > 0:
    every iteration with (t + 1) % check_every == 0 writes (KL, ||g||) to the next row of stats [rows, 2] f32, from row 0.
    grad [N, 2] f32 (optional) receives the gradient of the last iteration.  Nothing is read back.  -> y"""
    for name, t in (("y", y), ("update", update), ("gains", gains), ("grad", grad), ("stats", stats)):
        _chk(t, torch.float32, name)
    _chk(pstats, torch.float64, "pstats"); _chk(workspace, torch.uint8, "workspace")
    N = y.shape[0]
    if not P.is_cuda or P.dtype != torch.float32 or P.shape != (N, N) or P.stride(1) != 1:
        raise RuntimeError("tsne_steps: P must be a CUDA/HIP f32 matrix [N, N] with contiguous rows")
    assert y.shape == (N, 2) and update.shape == (N, 2) and gains.shape == (N, 2) and (grad is None or grad.shape == (N, 2))
    need = _lib.lib().ppt_tsne_steps_workspace_bytes(N)
    if need == 0:
        raise RuntimeError(f"tsne_steps: unsupported N={N} (2 <= N <= {TSNE_MAX_N})")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=y.device)
    rows = 0 if stats is None else stats.shape[0]
    assert stats is None or (stats.dim() == 2 and stats.shape[1] == 2)
    _lib.check(_lib.lib().ppt_tsne_steps(_p(P), P.stride(0), _p(pstats), N, _p(y), _p(update), _p(gains), int(t0), int(n), int(t_switch),
                                         float(early_exaggeration), float(lr), int(check_every), _p(stats), rows, _p(grad),
                                         _p(workspace), workspace.numel(), _stream()), "ppt_tsne_steps")
    return y


def health_check(x, flags, bit, maxabs=None):
    """flags[0] |= bit if x (any dtype, contiguous) holds a non-finite value; maxabs[0] = max(maxabs[0], max |finite x|) when
    given (ppt_health_check).  flags: int32 [1]; maxabs: f32 [1], non-negative."""
    _chk(x, None, "x"); _chk(flags, torch.int32, "flags"); _chk(maxabs, torch.float32, "maxabs")
    _lib.check(_lib.lib().ppt_health_check(_p(x), dtype_code(x), x.numel(), _p(flags), int(bit), _p(maxabs), _stream()), "ppt_health_check")


# tools/fp16_stress.py: when set, every wrapper below that returns a 16-bit activation reports it -- probe(name, tensor)
probe = None


def _probe(name, t):
    if probe is not None and t is not None and t.dtype in HALF:
        probe(name, t)
    return t


def scale_rows_convert(W, scale, out_dtype, cols=None, bias=None, shift=None):
    """convert(scale[:, None] * W[:, cols[0]:cols[1]]) for a row-major f32 matrix W [N, Kfull] -> [N, K] contiguous in out_dtype
    (ppt_scale_rows_convert); with bias / shift also returns scale * bias + shift [N] f32."""
    _chk(W, torch.float32, "W"); _chk(scale, torch.float32, "scale")
    N, Kf = W.shape
    c0, c1 = cols if cols is not None else (0, Kf)
    K = c1 - c0
    out = torch.empty((N, K), dtype=out_dtype, device=W.device)
    want_bs = bias is not None or shift is not None
    bs = torch.empty((N,), dtype=torch.float32, device=W.device) if want_bs else None
    src = W if c0 == 0 else W[:, c0:]
    _lib.check(_lib.lib().ppt_scale_rows_convert(ctypes.c_void_p(src.data_ptr()), Kf, N, K, _p(scale), _p(out), dtype_code(out), _p(bias), _p(shift),
                                                 _p(bs), _stream()), "ppt_scale_rows_convert")
    return (out, bs) if want_bs else out


def transpose(src, dst_dtype=None, pad_to=1):
    """[R,C] -> [C,R] (optionally converting).  pad_to > 1: the result is [C, Rp] with Rp = R rounded up
    to a multiple of pad_to and a zero tail (so that it can be the K dimension of a GEMM operand)."""
    _chk(src, None, "src")
    R, C = src.shape
    Rp = (R + pad_to - 1) // pad_to * pad_to
    dt_ = dst_dtype or src.dtype
    dst = torch.empty((C, Rp), dtype=dt_, device=src.device) if Rp == R else torch.zeros((C, Rp), dtype=dt_, device=src.device)
    _lib.check(_lib.lib().ppt_transpose(_p(src), dtype_code(src), _p(dst), dtype_code(dst), R, C, Rp, _stream()),
               "ppt_transpose")
    return dst


def col_sums(x):
    """sum over the rows of x [M,D] (any dtype, row stride free) -> [D] f32."""
    M, D = x.shape
    part = torch.empty(((M + 255) // 256, D), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().ppt_col_sums(_p(x), dtype_code(x), M, D, x.stride(0), _p(part), _stream()), "ppt_col_sums")
    return reduce_rows(part)


def reduce_rows(partial, out=None, accumulate=False):
    _chk(partial, torch.float32, "partial")
    P, D = partial.shape
    if out is None:
        out = torch.empty((D,), dtype=torch.float32, device=partial.device)
        accumulate = False
    _lib.check(_lib.lib().ppt_reduce_rows(_p(partial), P, D, _p(out), int(accumulate), _stream()), "ppt_reduce_rows")
    return out


def head_loss(feat, w, text_raw, logit_scale, labels, smoothing):
    """-> (loss 0-d, logits [B,C], d loss / d text_raw [C,E]): ppt_head_logits + ppt_head_ce_bwd (include/ppt_hip.h)."""
    for t, n in ((feat, "feat"), (w, "w [F,E]"), (text_raw, "text_raw")):
        _chk(t, torch.float32, n)
    _chk(labels, torch.int64, "labels")
    B, F = feat.shape
    C, E = text_raw.shape
    dev = feat.device
    spc = torch.empty((B, E), dtype=torch.float32, device=dev)
    logits = torch.empty((B, C), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    d_text = torch.empty((C, E), dtype=torch.float32, device=dev)
    L = _lib.lib()
    _lib.check(L.ppt_head_logits(_p(feat), _p(w), _p(text_raw), _p(logit_scale), B, F, E, C, _p(spc), _p(logits), _stream()),
               "ppt_head_logits")
    _lib.check(L.ppt_head_ce_bwd(_p(logits), _p(labels), _p(spc), _p(text_raw), float(smoothing), B, E, C, _p(loss), _p(d_text),
                                 _stream()), "ppt_head_ce_bwd")
    return loss, logits, d_text


def gemm_tn_splitk(x_a, x_b, min_blocks=768, max_splits=16):
    """C[N1,N2] (f32) = x_a[M,N1]^T @ x_b[M,N2] -- a weight gradient: the reduction runs over the M rows, and the output
    has few tiles (proj: 6 x 6), so the rows are cut into S slices that run as one batched NT GEMM over the transposed
    operands (slice z = columns [z*Mc, (z+1)*Mc) of both) and the S fp32 partial products are folded by reduce_rows in a
    fixed order.  S is chosen to reach `min_blocks` 64x64 workgroups."""
    M, N1 = x_a.shape
    N2 = x_b.shape[1]
    tiles = ((N1 + 63) // 64) * ((N2 + 63) // 64)
    if (x_a.dtype in HALF and x_b.dtype == x_a.dtype and M % 32 == 0 and N1 % 8 == 0 and N2 % 8 == 0
            and x_a.stride(1) == 1 and x_b.stride(1) == 1 and x_a.stride(0) % 8 == 0 and x_b.stride(0) % 8 == 0):
        # operands as stored (ppt_gemm_tn_bf16: transposing LDS reads), no transposed copies; the number of slices must
        # divide the number of 32-row slabs
        slabs = M // 32
        big = ((N1 + 127) // 128) * ((N2 + 127) // 128)
        want = max(1, min(max_splits * 2, (min_blocks + big - 1) // big, slabs))
        S = max(d for d in range(1, want + 1) if slabs % d == 0)
        part = torch.empty((S, N1 * N2), dtype=torch.float32, device=x_a.device)
        if profiler is not None:
            profiler.begin("gemm_bf16", 2.0 * M * N1 * N2, "ppt_gemm_tn_bf16")
        _lib.check(_lib.lib().ppt_gemm_tn_half(_p(x_a), x_a.stride(0), _p(x_b), x_b.stride(0), M, N1, N2, S, _p(part),
                                               dtype_code(x_a), _stream()), "ppt_gemm_tn_half")
        if profiler is not None:
            profiler.end()
        return (reduce_rows(part) if S > 1 else part[0]).view(N1, N2)
    S = max(1, min(max_splits, (min_blocks + tiles - 1) // tiles, (M + 63) // 64))
    Mc = ((M + S - 1) // S + 63) // 64 * 64
    at = transpose(x_a, pad_to=S * Mc)                                  # [N1, S*Mc], zero tail
    bt = transpose(x_b, pad_to=S * Mc)
    # split16: the pre-scale goes by an operand's ROLE, not by its position -- B is a weight everywhere else (x 2^4), here both
    # operands are activations / S-scaled gradients, which stay where they are like every other A operand
    role = (SPLIT16_POW2[0], SPLIT16_POW2[0]) if (_SPLIT16 and at.dtype == torch.float32) else None
    if S == 1:
        return gemm(at, bt, out_dtype=torch.float32, split=role)
    part = torch.empty((S * N1, N2), dtype=torch.float32, device=x_a.device)
    gemm(at[:, :Mc], bt[:, :Mc], out=part, batch=S, strideA=Mc, strideB=Mc, strideC=N1 * N2, split=role)
    return reduce_rows(part.view(S, N1 * N2)).view(N1, N2)


def adamw_step(p, g, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, skipped=None):
    """torch.optim.AdamW's update of ONE tensor in one launch (ppt_adamw_step); p, exp_avg, exp_avg_sq updated in place.
    grad_scale != 1: g is first multiplied by it IN PLACE (the un-scaling of a caller's loss-scaled backward).  An element whose
    gradient is not finite is skipped and counted in `skipped` (1-element int64 device tensor, or None)."""
    for t, nm in ((p, "p"), (g, "g"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, torch.float32, nm)
    if skipped is not None:
        _chk(skipped, torch.int64, "skipped")
    _lib.check(_lib.lib().ppt_adamw_step(_p(p), _p(g), _p(exp_avg), _p(exp_avg_sq), p.numel(), lr, beta1, beta2, eps, weight_decay,
                                         int(step), float(grad_scale), _p(skipped), _stream()), "ppt_adamw_step")


def adamw_multi(items, lr, beta1, beta2, eps, weight_decay, grad_scale=1.0, skipped=None, adam=False):
    """The same update for a list of (p, g, exp_avg, exp_avg_sq, step) in one launch per 64 tensors (ppt_adamw_multi).
    adam=True: torch.optim.Adam without weight decay on the same kernel (ppt_adam_multi: the hyper-parameters as doubles)."""
    arr = (_lib.AdamwTensor * len(items))()
    for a, (p, g, m, v, step) in zip(arr, items):
        for t, nm in ((p, "p"), (g, "g"), (m, "exp_avg"), (v, "exp_avg_sq")):
            _chk(t, torch.float32, nm)
        assert g.numel() == p.numel() == m.numel() == v.numel()
        a.p, a.g, a.exp_avg, a.exp_avg_sq, a.n, a.step = _p(p), _p(g), _p(m), _p(v), p.numel(), int(step)
    if skipped is not None:
        _chk(skipped, torch.int64, "skipped")
    if adam:
        assert weight_decay == 0, "Adam's weight_decay is an L2 term on the gradient, not AdamW's decay: not covered"
        _lib.check(_lib.lib().ppt_adam_multi(ctypes.cast(arr, ctypes.c_void_p), len(items), lr, beta1, beta2, eps, float(grad_scale),
                                             _p(skipped), _stream()), "ppt_adam_multi")
        return
    _lib.check(_lib.lib().ppt_adamw_multi(ctypes.cast(arr, ctypes.c_void_p), len(items), lr, beta1, beta2, eps, weight_decay,
                                          float(grad_scale), _p(skipped), _stream()), "ppt_adamw_multi")


def sgd_multi(items, lr, grad_scale=1.0, skipped=None):
    """torch.optim.SGD(params, lr)'s update p -= lr * g for a list of (p, g) in one launch per 64 tensors (ppt_sgd_multi); the
    non-finite skip and count of adamw_step."""
    arr = (_lib.AdamwTensor * len(items))()
    for a, (p, g) in zip(arr, items):
        _chk(p, torch.float32, "p"); _chk(g, torch.float32, "g")
        assert g.numel() == p.numel()
        a.p, a.g, a.n = _p(p), _p(g), p.numel()
    if skipped is not None:
        _chk(skipped, torch.int64, "skipped")
    _lib.check(_lib.lib().ppt_sgd_multi(ctypes.cast(arr, ctypes.c_void_p), len(items), lr, float(grad_scale), _p(skipped), _stream()),
               "ppt_sgd_multi")


def prompt_rows(base, slot, tokens, pos_rows):
    """out[i] = tokens[slot[i]] + pos_rows[i] where slot[i] >= 0, else base[i] (ppt_prompt_rows)."""
    _chk(base, torch.float32, "base"); _chk(slot, torch.int32, "slot"); _chk(tokens, torch.float32, "tokens")
    _chk(pos_rows, torch.float32, "pos_rows")
    rows, W = base.shape
    out = torch.empty_like(base)
    _lib.check(_lib.lib().ppt_prompt_rows(_p(base), _p(slot), _p(tokens), _p(pos_rows), rows, W, _p(out), _stream()), "ppt_prompt_rows")
    return out


def prompt_rows_bwd(g, rows_of, n_tok, scale=1.0):
    """d tokens [n_tok, W] = scale * sums of the rows of g listed per token in rows_of [n_tok, max_rows] i32 (-1 terminated)."""
    _chk(g, torch.float32, "g"); _chk(rows_of, torch.int32, "rows_of")
    W = g.shape[1]
    out = torch.empty((n_tok, W), dtype=torch.float32, device=g.device)
    _lib.check(_lib.lib().ppt_prompt_rows_bwd(_p(g), _p(rows_of), rows_of.shape[1], n_tok, W, float(scale), _p(out), _stream()),
               "ppt_prompt_rows_bwd")
    return out


# ---------------------------------------------------------------------------------------------
# zero-shot classification: the text tower on ragged sentence rows (csrc/attention_ragged.hip, csrc/zeroshot.hip; ppt_amd/zeroshot.py)
RAGGED_MAX_LEN = 128                 # positions of a sentence the ragged attention takes (two 64-key tiles); the tower's ctx is 77


def ragged_attention_plan(lens):
    """HOST: sentence lengths [S] -> the bin plan of ppt_attention_ragged_fwd, int32 numpy [nbins * 64]: entry (s << 8) | p for the
    virtual row that is position p of sentence s, -1 for an empty one.  Sentences go into bins of 64 virtual rows in order, each
    at a multiple of 16 rows and inside one bin (a new bin is opened when the next one does not fit); a sentence of 65-128
    positions takes two bins of its own.  A function of the lengths alone: make it once per sentence set and pass it as `plan=`."""
    import numpy as np
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    if lens.size == 0 or int(lens.min()) < 1 or int(lens.max()) > RAGGED_MAX_LEN:
        raise ValueError(f"ragged_attention_plan: every sentence needs 1 .. {RAGGED_MAX_LEN} positions")
    start = np.empty(lens.size, dtype=np.int64)              # first virtual row of each sentence
    fill = 0
    for s, n in enumerate(lens.tolist()):
        need = (n + 15) // 16 * 16 if n <= 64 else 128
        if fill % 64 and (n > 64 or fill % 64 + need > 64):
            fill = (fill + 63) // 64 * 64
        start[s] = fill
        fill += need
    plan = np.full(((fill + 63) // 64) * 64, -1, dtype=np.int32)
    sent = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
    pos = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    plan[start[sent] + pos] = ((sent << 8) | pos).astype(np.int32)
    return plan


def sentence_rows(table, pos, ids, offsets, rows):
    """x0 [rows, W] f32: row offsets[s] + p = table[ids[s, p]] + pos[p] for the positions of sentence s, rows >= offsets[S] zero
    (ppt_sentence_rows).  table [vocab, W] f32, pos [ctx, W] f32, ids [S, ctx] i32, offsets [S + 1] i32, all on the device."""
    _chk(table, torch.float32, "table"); _chk(pos, torch.float32, "pos"); _chk(ids, torch.int32, "ids"); _chk(offsets, torch.int32, "offsets")
    S, ctx = ids.shape
    if offsets.numel() != S + 1 or pos.shape[0] < ctx or pos.shape[1] != table.shape[1]:
        raise ValueError("sentence_rows: offsets must be [S + 1], pos [>= ctx, W]")
    out = torch.empty((int(rows), table.shape[1]), dtype=torch.float32, device=table.device)
    _lib.check(_lib.lib().ppt_sentence_rows(_p(table), table.shape[0], _p(pos), _p(ids), ctx, _p(offsets), S, table.shape[1], _p(out),
                                            int(rows), _stream()), "ppt_sentence_rows")
    return out


def attention_ragged_fwd(qkv, offsets, H, scale, plan=None):
    """causal attention of every sentence of the ragged layout: qkv [M, 3*H*64] (f32: split16 products; f16; bf16), offsets [S + 1]
    i32 on the device -> out [M, H*64]; rows >= offsets[S] are left unwritten.  plan: ragged_attention_plan of the lengths as an
    int32 DEVICE tensor; None builds it from offsets (one device read)."""
    _chk(qkv, None, "qkv"); _chk(offsets, torch.int32, "offsets")
    if plan is None:
        o = offsets.cpu().numpy()
        plan = torch.from_numpy(ragged_attention_plan(o[1:] - o[:-1])).to(qkv.device)
    _chk(plan, torch.int32, "plan")
    if qkv.dim() != 2 or qkv.shape[0] < 1 or qkv.shape[1] != 3 * H * 64:
        raise ValueError(f"attention_ragged_fwd: qkv must be [M, 3 * H * 64] with H = {H}, got {tuple(qkv.shape)}")
    if offsets.dim() != 1 or offsets.numel() < 2 or plan.dim() != 1 or plan.numel() == 0 or plan.numel() % 64:
        raise ValueError("attention_ragged_fwd: offsets must be [S + 1], plan [bins * 64] (ragged_attention_plan)")
    M = qkv.shape[0]
    out = torch.empty((M, H * 64), dtype=qkv.dtype, device=qkv.device)
    if profiler is not None:
        profiler.begin("attention_ragged_fwd", 0.0)
    _lib.check(_lib.lib().ppt_attention_ragged_fwd(_p(qkv), _p(out), _p(offsets), _p(plan), offsets.numel() - 1, M, plan.numel() // 64, H, 64,
                                                   scale, dtype_code(qkv), _stream()), "ppt_attention_ragged_fwd")
    if profiler is not None:
        profiler.end()
    return out


def template_ensemble(feat, group_offsets):
    """W [C, E] f32 = normalize(mean over the sentences of class c of normalize(feat[t])): ULIP's zero-shot classifier
    (ppt_template_ensemble).  feat [S, E] f32, group_offsets [C + 1] i32 on the device, ascending within [0, S]; the values stay on the
    device, so they are the caller's to check (zeroshot.classifier does, on the host): the kernel clamps a range to [0, S] and
    writes a zero row for an empty one."""
    _chk(feat, torch.float32, "feat"); _chk(group_offsets, torch.int32, "group_offsets")
    if feat.dim() != 2 or feat.shape[0] < 1 or group_offsets.dim() != 1 or group_offsets.numel() < 2:
        raise ValueError("template_ensemble: feat must be [S, E], group_offsets [C + 1]")
    C = group_offsets.numel() - 1
    W = torch.empty((C, feat.shape[1]), dtype=torch.float32, device=feat.device)
    _lib.check(_lib.lib().ppt_template_ensemble(_p(feat), _p(group_offsets), feat.shape[0], C, feat.shape[1], _p(W), _stream()),
               "ppt_template_ensemble")
    return W


def cosine_head(f, W, logit_scale):
    """logits [B, C] = exp(logit_scale) * <f[b] / |f[b]|, W[c]>, fp32 (ppt_cosine_head): the CLIP / ULIP zero-shot rule -- unlike
    PPT's own forward (ULIP_models.py:279-281) the point feature IS normalised.  logit_scale: a 0-dim f32 device tensor."""
    _chk(f, torch.float32, "f"); _chk(W, torch.float32, "W"); _chk(logit_scale, torch.float32, "logit_scale")
    if f.dim() != 2 or W.dim() != 2 or f.shape[1] != W.shape[1] or logit_scale.numel() != 1:
        raise ValueError("cosine_head: f [B, E], W [C, E], logit_scale one value")
    logits = torch.empty((f.shape[0], W.shape[0]), dtype=torch.float32, device=f.device)
    _lib.check(_lib.lib().ppt_cosine_head(_p(f), _p(W), _p(logit_scale), f.shape[0], W.shape[0], f.shape[1], _p(logits), _stream()),
               "ppt_cosine_head")
    return logits


# ---------------------------------------------------------------------------------------------
# the device-resident input pipeline (csrc/cloud_prep.hip; ppt_amd/data/device_loader.py)
def cloud_prep(src, item, n, *, sel=None, lengths=None, normalize=False, scale=None, shift=None, perm=None, seg_src=None):
    """src [M, Nmax, C >= 3] f32 resident clouds, item [B] i64 -> out [B, n, 3] f32 (and seg [B, n] i64 when seg_src [M, Nmax] i32
    is given): rows `sel` [B, n] i64 (None: the first n) of cloud item[b], pc_normalize if `normalize`, translate_pointcloud when
    scale / shift [B, 3] f64 are given, np.random.shuffle when perm [B, n] i32 is -- bit-identical to the reference's numpy
    (ppt_cloud_prep_f32)."""
    _chk(src, torch.float32, "src"); _chk(item, torch.int64, "item"); _chk(sel, torch.int64, "sel"); _chk(lengths, torch.int32, "lengths")
    _chk(scale, torch.float64, "scale"); _chk(shift, torch.float64, "shift"); _chk(perm, torch.int32, "perm")
    _chk(seg_src, torch.int32, "seg_src")
    if src.dim() != 3:
        raise ValueError(f"src must be [M, Nmax, C], got {tuple(src.shape)}")
    M, Nmax, C = src.shape
    B = item.numel()
    for t, shape, nm in ((sel, (B, n), "sel"), (perm, (B, n), "perm"), (scale, (B, 3), "scale"), (shift, (B, 3), "shift"),
                         (lengths, (M,), "lengths"), (seg_src, (M, Nmax), "seg_src")):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{nm} must be {shape}, got {tuple(t.shape)}")
    if (scale is None) != (shift is None):
        raise ValueError("scale and shift are given together")
    out = torch.empty((B, n, 3), dtype=torch.float32, device=src.device)
    seg = torch.empty((B, n), dtype=torch.int64, device=src.device) if seg_src is not None else None
    if profiler is not None:
        profiler.begin("cloud_prep", float(B) * n * (24 + (8 if sel is not None else 0) + (4 if perm is not None else 0)))
    _lib.check(_lib.lib().ppt_cloud_prep_f32(_p(src), M, Nmax, C, _p(lengths), _p(item), B, _p(sel), int(n), int(bool(normalize)),
                                             int(scale is not None), _p(scale), _p(shift), _p(perm), _p(seg_src), _p(seg), _p(out),
                                             _stream()), "ppt_cloud_prep_f32")
    if profiler is not None:
        profiler.end()
    return out if seg is None else (out, seg)


def cloud_draws(index, n, seed, epoch, *, rows=None, rows_all=0, start=False, affine=False, perm=False, sel=False):
    """The Philox4x32-10 draws of the samples `index` [B] i64 (ppt_cloud_draws): a dict with the requested ones of
    start [B] i64 and sel [B, n] i64 in [0, rows), scale / shift [B, 3] f64, perm [B, n] i32.  rows [B] i32 or rows_all."""
    _chk(index, torch.int64, "index"); _chk(rows, torch.int32, "rows")
    B, dev = index.numel(), index.device
    out = {}
    if start:
        out["start"] = torch.empty(B, dtype=torch.int64, device=dev)
    if affine:
        out["scale"] = torch.empty((B, 3), dtype=torch.float64, device=dev)
        out["shift"] = torch.empty((B, 3), dtype=torch.float64, device=dev)
    if perm:
        out["perm"] = torch.empty((B, n), dtype=torch.int32, device=dev)
    if sel:
        out["sel"] = torch.empty((B, n), dtype=torch.int64, device=dev)
    g = out.get
    _lib.check(_lib.lib().ppt_cloud_draws(_p(index), B, _p(rows), int(rows_all), int(n), int(seed) & (2 ** 64 - 1), int(epoch) & 0xFFFFFFFF,
                                          _p(g("start")), _p(g("scale")), _p(g("shift")), _p(g("perm")), _p(g("sel")), None, 0, None,
                                          _stream()), "ppt_cloud_draws")
    return out


def philox4x32(counters, seed):
    """counters [R, 4] i32 (the bit patterns of the 32-bit counter words) -> the Philox4x32-10 output words [R, 4] i32 under the
    64-bit key `seed` (low word = key[0]): the generator of ppt_cloud_draws, exposed for known-answer checks."""
    _chk(counters, torch.int32, "counters")
    out = torch.empty_like(counters)
    _lib.check(_lib.lib().ppt_cloud_draws(None, 0, None, 0, 0, int(seed) & (2 ** 64 - 1), 0, None, None, None, None, None, _p(counters),
                                          counters.shape[0], _p(out), _stream()), "ppt_cloud_draws")
    return out


# the reference's augmentations on a finished batch (csrc/cloud_augment.hip; ppt_amd/data/augment.py)
AUG_STAGES = {"dropout": (1, ((torch.uint8, ("B", "n")),)), "scale": (2, ((torch.float64, ("B",)),)),
              "shift": (3, ((torch.float64, ("B", 3)),)), "rotate": (4, ((torch.float64, ("B", 3, 3)),)),
              "jitter": (5, ((torch.float64, ("B", "n", 3)),)),
              "affine": (6, ((torch.float64, ("B", 3)), (torch.float64, ("B", 3)))), "height": (7, ())}
AUG_MAX_STAGES = 8
AUG_MAGNITUDES = ("max_dropout", "scale_low", "scale_high", "shift_range", "angle_sigma", "angle_clip", "jitter_sigma", "jitter_clip")
AUG_DEFAULTS = dict(zip(AUG_MAGNITUDES, (0.875, 0.8, 1.25, 0.1, 0.06, 0.18, 0.01, 0.05)))      # data/dataset_3d.py:83-131


def cloud_augment(pc, stages, *, height=False):
    """pc [B, n, 3] f32 -> a new [B, n, 3] f32 tensor ([B, n, 4] with the height column when height=True or ("height",) closes the
    list), the stages applied in order in one launch (ppt_cloud_augment_f32), each bit-identical to the reference's numpy:
        ("dropout", mask [B, n] u8)   ("scale", s [B] f64)   ("shift", t [B, 3] f64)   ("rotate", R [B, 3, 3] f64)
        ("jitter", noise [B, n, 3] f64)   ("affine", scale [B, 3] f64, shift [B, 3] f64)   ("height",)
    At most 8 stages, the height column included; n <= 8192."""
    stages = [tuple(s) for s in stages] + ([("height",)] if height else [])
    for k, st in enumerate(stages):
        if not st or st[0] not in AUG_STAGES:
            raise ValueError(f"cloud_augment: unknown stage {st[0] if st else st!r}; one of {tuple(AUG_STAGES)}")
        if len(st) - 1 != len(AUG_STAGES[st[0]][1]):
            raise ValueError(f"cloud_augment: stage {st[0]!r} takes {len(AUG_STAGES[st[0]][1])} parameter arrays, got {len(st) - 1}")
        if st[0] == "height" and k != len(stages) - 1:
            raise ValueError("cloud_augment: the height column is taken from the finished cloud: 'height' must be the last stage")
    if not 1 <= len(stages) <= AUG_MAX_STAGES:
        raise ValueError(f"cloud_augment: between 1 and {AUG_MAX_STAGES} stages (the height column counts), got {len(stages)}")
    _chk(pc, torch.float32, "pc")
    if pc.dim() != 3 or pc.shape[2] != 3:
        raise ValueError(f"pc must be [B, n, 3], got {tuple(pc.shape)}")
    B, n, _ = pc.shape
    arr = (_lib.AugStage * len(stages))()
    for k, st in enumerate(stages):
        kind, spec = AUG_STAGES[st[0]]
        arr[k].kind = kind
        for j, (t, (dtype, shape)) in enumerate(zip(st[1:], spec)):
            _chk(t, dtype, f"{st[0]} parameter {j}")
            want = tuple(B if d == "B" else n if d == "n" else d for d in shape)
            if tuple(t.shape) != want:
                raise ValueError(f"stage {st[0]!r}: parameter {j} must be {want}, got {tuple(t.shape)}")
            setattr(arr[k], "ab"[j], t.data_ptr())
    out = torch.empty((B, n, 4 if stages[-1][0] == "height" else 3), dtype=torch.float32, device=pc.device)
    if profiler is not None:
        profiler.begin("cloud_augment", float(B) * n * 28)
    _lib.check(_lib.lib().ppt_cloud_augment_f32(_p(pc), B, n, arr, len(stages), _p(out), _stream()), "ppt_cloud_augment_f32")
    if profiler is not None:
        profiler.end()
    return out


def cloud_draws_aug(index, n, seed, epoch, *, dropout=False, scale=False, shift=False, rotate_perturbation=False, rotate=False,
                    jitter=False, **magnitudes):
    """The Philox4x32-10 draws of the augmentations for the samples `index` [B] i64 (ppt_cloud_draws_aug; slots 4-10, the layout is
    stated in include/ppt_hip.h): a dict with the requested ones of
        dropout              ratio [B] f64 in [0, max_dropout), mask [B, n] u8
        scale                scale [B] f64 in [scale_low, scale_high)
        shift                shift [B, 3] f64 in [-shift_range, shift_range)
        rotate_perturbation  angles [B, 3] f64 = clip(angle_sigma N(0, 1), +-angle_clip), perturb [B, 3, 3] f64 = Rz (Ry Rx)
        rotate               angle [B] f64 in [0, 2 pi), rotate [B, 3, 3] f64 about y
        jitter               noise [B, n, 3] f64 = clip(jitter_sigma N(0, 1), +-jitter_clip)
    magnitudes: any of AUG_MAGNITUDES; the defaults are the reference's (AUG_DEFAULTS)."""
    unknown = set(magnitudes) - set(AUG_MAGNITUDES)
    if unknown:
        raise ValueError(f"cloud_draws_aug: unknown magnitude {sorted(unknown)}; one of {AUG_MAGNITUDES}")
    if not (dropout or scale or shift or rotate_perturbation or rotate or jitter):
        raise ValueError("cloud_draws_aug: nothing asked for")
    _chk(index, torch.int64, "index")
    B, dev = index.numel(), index.device
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
    out = {}
    if dropout:
        out["ratio"], out["mask"] = f64(B), torch.empty((B, n), dtype=torch.uint8, device=dev)
    if scale:
        out["scale"] = f64(B)
    if shift:
        out["shift"] = f64(B, 3)
    if rotate_perturbation:
        out["angles"], out["perturb"] = f64(B, 3), f64(B, 3, 3)
    if rotate:
        out["angle"], out["rotate"] = f64(B), f64(B, 3, 3)
    if jitter:
        out["noise"] = f64(B, n, 3)
    mag = (ctypes.c_double * len(AUG_MAGNITUDES))(*[float(magnitudes.get(k, AUG_DEFAULTS[k])) for k in AUG_MAGNITUDES])
    g = out.get
    _lib.check(_lib.lib().ppt_cloud_draws_aug(_p(index), B, int(n), int(seed) & (2 ** 64 - 1), int(epoch) & 0xFFFFFFFF, mag, _p(g("ratio")),
                                              _p(g("mask")), _p(g("scale")), _p(g("shift")), _p(g("angles")), _p(g("perturb")),
                                              _p(g("angle")), _p(g("rotate")), _p(g("noise")), _stream()), "ppt_cloud_draws_aug")
    return out
