"""Training-step harness reproducing the caller of the hot path, main_cls.py:155-234 (train()):
zero_grad, per-iteration LR, forward, CrossEntropy(label_smoothing), backward, AdamW, logit-scale
clamp -- plus the MI355X-native replacement of DistributedDataParallel (main_cls.py:47-49):
ONE RCCL all-reduce per step over a flat fp32 buffer holding the PromptLearner / PointAdapter
gradients, and a broadcast of the BatchNorm running statistics from rank 0 (DDP broadcast_buffers).
"""
import contextlib
import math

import numpy as np
import os

import torch
import torch.distributed as dist
from torch import nn


def cosine_scheduler(base_value, final_value, epochs, niter_per_ep, warmup_epochs=0, start_warmup_value=0.0):
    """utils/utils.py:253-264: one learning rate per iteration (linear warm-up, then half cosine)."""
    warm = warmup_epochs * niter_per_ep
    head = np.linspace(start_warmup_value, base_value, warm) if warmup_epochs > 0 else np.array([])
    it = np.arange(epochs * niter_per_ep - warm)
    tail = final_value + 0.5 * (base_value - final_value) * (1 + np.cos(np.pi * it / len(it)))
    sched = np.concatenate((head, tail))
    assert len(sched) == epochs * niter_per_ep
    return sched


class FlatGradSync:
    """Data parallelism for prompt tuning: the trainable parameters' .grad tensors are views into one
    flat fp32 buffer; after backward a single all-reduce (SUM) + 1/world gives DDP's averaged
    gradients.  64 KiB (head_type 0) ... 7.2 MB (head_type 3) per step -- latency-bound on xGMI, so
    one call beats any bucketing."""

    def __init__(self, params, process_group=None, lazy=False):
        """lazy=False: .grad of every trainable parameter IS a view of the flat buffer (autograd accumulates into it).
        lazy=True (train.Trainer): zero() only drops the .grad references -- autograd then ASSIGNS each gradient instead of
        adding it into a zeroed view (one ATen add per parameter per step: 46 of them in the part-seg step) -- and
        all_reduce() packs the gradients into the flat buffer with one multi-tensor copy, reduces it, and re-binds .grad to
        the views.  Without a process group nothing is packed at all: the optimizer reads the gradients where they are."""
        self.params = [p for p in params if p.requires_grad]
        self.group = process_group
        self.lazy = lazy
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        self.views = []
        off = 0
        for p in self.params:
            self.views.append(self.flat[off:off + p.numel()].view_as(p))
            if not lazy:
                p.grad = self.views[-1]
            off += p.numel()

    def zero(self):
        if self.lazy:
            # the gradients were allocated on whatever stream their backward node ran on and last read on the CURRENT stream
            # (optimizer / packing): tell the caching allocator, or dropping the reference here -- the host runs ahead of the
            # GPU -- would let their memory be reused before that read has happened
            cur = torch.cuda.current_stream() if self.flat.is_cuda else None
            for p in self.params:
                if p.grad is not None and cur is not None and p.grad.is_cuda:
                    p.grad.record_stream(cur)
                p.grad = None
            return
        self.flat.zero_()
        for p, v in zip(self.params, self.views):          # re-attach views if an optimizer / zero_grad(set_to_none) dropped them
            if p.grad is None or p.grad.data_ptr() != v.data_ptr():
                p.grad = v

    def all_reduce(self):
        if not (dist.is_available() and dist.is_initialized()):
            return
        if self.lazy and len(self.params) == 1 and self.params[0].grad is not None and self.params[0].grad.is_contiguous():
            # one trained tensor (head_type 0: the prompt tokens): reduce its gradient where it is -- no packing copy on the
            # prompt chain, which is the step's critical path; `flat` is re-pointed at it so that readers see the reduced values
            g = self.params[0].grad
            dist.all_reduce(g, op=dist.ReduceOp.SUM, group=self.group)
            w = dist.get_world_size(self.group)
            if w > 1:
                g.div_(w)
            self.flat = g.detach().view(-1)
            self.views = [self.flat.view_as(self.params[0])]        # (readers of either see the reduced gradient)
            return
        used = None
        if self.lazy:
            with torch.no_grad():
                have = [(v, p.grad) for p, v in zip(self.params, self.views) if p.grad is not None and p.grad.data_ptr() != v.data_ptr()]
                # a parameter no node wrote a gradient for (part-seg's conv2: constructed, unused in forward) travels as zeros and
                # KEEPS .grad = None afterwards -- DistributedDataParallel(find_unused_parameters=True), main_partseg.py:48, leaves
                # the gradient of a globally unused parameter untouched, so the reference's AdamW never decays or tracks it.  The
                # graph is the same on every rank, so "unused here" is "unused everywhere".
                used = [p.grad is not None for p in self.params]
                for p, v in zip(self.params, self.views):
                    if p.grad is None:
                        v.zero_()
                if have:
                    torch._foreach_copy_([v for v, _ in have], [g for _, g in have])
                    if self.flat.is_cuda:            # (read here, on this stream; allocated on their backward node's: see zero())
                        cur = torch.cuda.current_stream()
                        for _, g in have:
                            g.record_stream(cur)
        dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=self.group)
        w = dist.get_world_size(self.group)
        if w > 1:
            self.flat.div_(w)
        if self.lazy:
            for p, v, u in zip(self.params, self.views, used):
                if u:
                    p.grad = v


class BufferBroadcast:
    """DDP(broadcast_buffers=True) equivalent for the BatchNorm running statistics of the tokenizer,
    which keep updating because model.train() leaves the frozen BN layers in train mode
    (SURVEY.md App. A Q3): the float buffers are re-bound as views of one flat tensor that rank 0
    broadcasts before every forward."""

    def __init__(self, model, process_group=None):
        self.group = process_group
        bufs = [(m, n, b) for m in model.modules() for n, b in m._buffers.items()
                if b is not None and b.dtype == torch.float32]
        self.flat = None
        if bufs:
            n = sum(b.numel() for _, _, b in bufs)
            self.flat = torch.empty(n, dtype=torch.float32, device=bufs[0][2].device)
            off = 0
            for m, name, b in bufs:
                view = self.flat[off:off + b.numel()].view_as(b)
                view.copy_(b)
                m._buffers[name] = view
                off += b.numel()

    def broadcast(self):
        if self.flat is not None and dist.is_available() and dist.is_initialized():
            dist.broadcast(self.flat, src=0, group=self.group)


def broadcast_module_states(model, process_group=None, src=0, chunk_bytes=256 << 20):
    """What DistributedDataParallel's constructor does before the first forward (main_cls.py:47-49; torch's
    `_sync_module_states`): rank `src`'s parameters AND buffers overwrite every other rank's, in flat chunks of at most
    `chunk_bytes` (DDP's 250 MB buckets) -- ONE collective for the trainable set of every PPT configuration.  With the
    reference's per-rank seeding (`seed = args.seed + rank`, main_cls.py:39) this broadcast is the only thing that makes
    `learnable_tokens` and the randomly initialised un-frozen last block equal across ranks.  Tensors that are
    neither parameter nor buffer -- PromptLearner.embedding (App. A Q1) -- stay per-rank, as under DDP.
    Trainable parameters go first (their own chunk), then the frozen ones, then the buffers.  Returns the number of collectives."""
    if not (dist.is_available() and dist.is_initialized()):
        return 0
    seen, groups = set(), [[], [], []]
    for p in model.parameters():
        if id(p) not in seen:
            seen.add(id(p))
            groups[0 if p.requires_grad else 1].append(p.data)
    for b in model.buffers():
        if b is not None and id(b) not in seen:
            seen.add(id(b))
            groups[2].append(b.data)
    calls = 0
    with torch.no_grad():
        for tensors in groups:
            by_type = {}
            for t in tensors:
                by_type.setdefault((t.dtype, t.device), []).append(t)
            for (dtype, dev), ts in by_type.items():
                i = 0
                while i < len(ts):
                    j, n = i, 0
                    while j < len(ts) and (j == i or (n + ts[j].numel()) * ts[j].element_size() <= chunk_bytes):
                        n += ts[j].numel()
                        j += 1
                    flat = torch.empty(n, dtype=dtype, device=dev)
                    off = 0
                    for t in ts[i:j]:
                        flat[off:off + t.numel()].copy_(t.reshape(-1))
                        off += t.numel()
                    dist.broadcast(flat, src=src, group=process_group)
                    calls += 1
                    off = 0
                    for t in ts[i:j]:
                        t.copy_(flat[off:off + t.numel()].view_as(t))
                        off += t.numel()
                    i = j
    if calls and torch.cuda.is_available():
        torch.cuda.synchronize()             # (the collectives are complete before any hipGraph capture can begin)
    return calls


class _CrossEntropyRows(torch.autograd.Function):
    """nn.CrossEntropyLoss(label_smoothing) as one node: the forward pass over the logits also forms d loss / d logits."""

    @staticmethod
    def forward(ctx, logits, labels, smoothing, ignore_index=-100):
        from . import ops
        loss, dlogits, scale = ops.cross_entropy_rows(logits, labels, smoothing, ignore_index)
        ctx.save_for_backward(dlogits, scale)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        dlogits, scale = ctx.saved_tensors
        return dlogits * (dloss * scale), None, None, None


_OPTIM_KINDS = {torch.optim.AdamW: "adamw", torch.optim.Adam: "adam", torch.optim.SGD: "sgd"}      # main_cls.py:54-60, by exact type


class Trainer:
    """One object per rank.  `step(pc, label)` == one iteration of main_cls.py:179-214."""

    def __init__(self, model, lr=3e-3, betas=(0.9, 0.98), eps=1e-8, wd=0.1, label_smoothing=0.2,
                 lr_schedule=None, distributed=None, capturable=False, optim="adamw"):
        self.model = model
        self.criterion = nn.CrossEntropyLoss(label_smoothing=label_smoothing)       # main_cls.py:52
        # main_cls.py:55-60 builds AdamW over ALL parameters; frozen ones never get a grad and are skipped by step().
        # Here the frozen ones are left out (380 tensors the optimizer would walk every step); reference_optimizer_state
        # re-indexes the state dict to the reference's layout for checkpoints.
        trained = [p for p in model.parameters() if p.requires_grad]
        if optim == "adamw":
            self.optimizer = torch.optim.AdamW(trained, lr=lr, betas=betas, eps=eps, weight_decay=wd, capturable=capturable)
        elif optim == "adam":
            # --optim adam, main_cls.py:56-57: torch's defaults but for lr (betas, eps and wd are NOT passed on).  It steps on the
            # AdamW kernel with a decay factor of exactly 1: what is left is Adam's arithmetic (ppt_adam_multi: the same kernel,
            # hyper-parameters as doubles -- Adam's beta2 = 0.999 as a float would leave 1 - beta2 4.7e-5 off).
            self.optimizer = torch.optim.Adam(trained, lr=lr)
        elif optim == "sgd":
            self.optimizer = torch.optim.SGD(trained, lr=lr)                        # --optim sgd, main_cls.py:54-55; ppt_sgd_multi
        else:
            raise ValueError(f"Trainer: optim must be 'adamw', 'adam' or 'sgd', got {optim!r}")
        # One launch per trained tensor (ppt_adamw_step: torch.optim.AdamW's arithmetic; csrc/optim.hip) instead of the ~10
        # multi-tensor kernels of the foreach implementation, while few tensors train: every kernel of the prompt chain costs a
        # dispatch round trip.  The torch optimizer object stays the owner of hyper-parameters and state (state_dict()).
        self.fused_adamw = os.environ.get("PPT_FUSED_ADAMW", "1") != "0"
        # Gradient scaling for the performance mode's fp16 backward stages is NOT done here (rounds 2-3 seeded backward() with a
        # loss scale and un-scaled inside the optimizer -- which an unchanged main_cls.py / main_partseg.py loop never got): every
        # autograd node that carries gradients in half scales what it receives and un-scales what it hands out itself
        # (ppt_amd/gradscale.py), so `loss.backward()` below is the reference's plain call and .grad, the all-reduce and AdamW see
        # true fp32 gradients on every rank whatever the local batch size.  What remains here is the defence: both AdamW kernels
        # skip an element whose gradient is not finite and count it (`nonfinite_grad_elements()`); `step(check_finite=True)`
        # raises on a non-finite loss as main_cls.py:205-207 does, and on a non-zero count.
        self._skipped = None
        # ... and the run-time overflow watch of the half-precision stages (ppt_amd/health.py): two tiny launches per step off the
        # prompt chain, one stall-free poll every `health.every` steps; a set bit demotes the offending side to bf16.
        # PPT_HEALTH=0 turns it off, PPT_HEALTH_EVERY sets the poll interval.
        self.health = None
        self.demotions = []
        # (round 6, ADVICE r5: split16 is a guarded mode too -- its products are formed from IEEE-half pairs, so it has half's range)
        half_range = getattr(model, "precision", None) == torch.bfloat16 or getattr(model, "split16", False)
        if os.environ.get("PPT_HEALTH", "1") != "0" and half_range and hasattr(model, "health") \
                and next(model.parameters()).is_cuda:
            from . import health
            # (under a process group a poll is ONE blocking read + all-reduce so that every rank decides alike: every 200 steps)
            dflt = "200" if (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1) else "50"
            self.health = model.health = health.Monitor(next(model.parameters()).device, every=int(os.environ.get("PPT_HEALTH_EVERY", dflt)))
        # logit_scale is frozen in every PPT configuration (ULIP_models.py:487-507) and its value lies inside the clamp range:
        # main_cls.py:213's per-step clamp is then idempotent -- applied once here, and per step only if it ever trains
        if hasattr(model, "logit_scale"):
            with torch.no_grad():
                model.logit_scale.data.clamp_(0, 4.6052)
        self.lr_schedule = lr_schedule
        self.it = 0
        # Round 6: the mixed mode checks the GRADIENTS it produces against the fp32-grade mode once, on the first
        # batch of the run (calibrate_gradients below).  "switch" (default): over the threshold the model leaves the mixed mode for
        # split16; "warn": it says so and stays; "off".  Only where something besides the PromptLearner trains: with the prompt
        # tokens alone the text tower's own load-time check (ULIP_WITH_IMAGE.calibrate_text_precision) covers what they depend on.
        self.grad_check = os.environ.get("PPT_GRAD_CHECK", "switch")
        self.grad_check_threshold = float(os.environ.get("PPT_GRAD_CHECK_THRESHOLD", "2e-2"))
        self.grad_calibration = None
        self._dry = False
        self.extra_inputs = ()        # e.g. the one-hot shape category of main_partseg.py:210
        if distributed is None:
            distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        self.distributed = distributed
        self.sync = FlatGradSync(model.parameters(), lazy=os.environ.get("PPT_LAZY_GRADS", "1") != "0")
        self.run_ahead = True
        # DDP re-broadcasts rank 0's buffers before every forward.  The only float buffers here are BatchNorm running
        # statistics, which a train-mode forward never reads and which rank 0 updates from its own batches alone, so one
        # broadcast in finish() leaves every rank with exactly the state the per-step broadcast would -- without a
        # collective on the point tower's stream in every iteration.  True restores DDP's schedule.
        self.broadcast_buffers_every_step = False
        self.fused_head = True        # head_type 0 on a GPU: ULIP_WITH_IMAGE.forward_loss
        # True: the caller vouches that `pc` is complete in device memory when step() is called (a resident tensor, or a
        # loader that synchronised its copy stream) -- NOT merely queued on the current stream.  The grouping stage of the
        # point tower (FPS + kNN, a function of pc alone) then runs on its own stream as soon as step() is called, i.e.
        # under the previous iteration's transformer blocks (graphs.AheadStage, which every point encoder runs its stage through).
        self.inputs_ready = False
        # head_type 0 with inputs_ready: the frozen point tower of iteration i + 1 does not wait for iteration i's head (which
        # waits for the prompt chain) -- it runs on its own stream, back to back (ULIP_WITH_IMAGE.forward_loss).  Opt-in: it
        # does not shorten the C2 step (3.83 vs 3.80 ms, tools/ab_env.py) -- the step timeline (tools/step_timeline.py) shows
        # the caller's stream does not idle at the head for long; what bounds the step is the prompt chain's kernels getting
        # 2.3x slower beside the tower (tools/chain_under_load.py), on whatever stream the tower runs.
        self.tower_own_stream = os.environ.get("PPT_TOWER_STREAM", "0") != "0"
        self._tower_used = None
        # With a fully frozen point side (head_type 0) the tower already runs back to back on its stream with the whole
        # prompt side underneath it, the step is throughput-bound and hiding FPS buys nothing (C2: 4.22 ms without, 4.29
        # with); with a trainable last block the caller's stream has bubbles and it does (C3: 8.85 -> 8.28 ms).  Round 3: with the
        # faster prompt chain the tower is the longer side and the 0.22 ms of serial FPS picks at its head now count -- C2
        # 3.349 -> 3.283 ms with the grouping stage ahead (same box, tools/ab_env.py): on by default, PPT_GROUP_AHEAD_FROZEN=0
        # turns it off.
        self.group_ahead_when_frozen = os.environ.get("PPT_GROUP_AHEAD_FROZEN", "1") != "0"
        # head_type 0: only the prompt learner trains, so the point tower never reads a parameter the optimizer writes
        self._point_side_frozen = all(n.startswith("prompt_learner.") or not p.requires_grad
                                      for n, p in model.named_parameters())
        self._side_used = None
        # trainables outside the prompt learner and the point encoder's last block (pc_projection, logit_scale, a
        # part-seg decoder ...) are read wherever forward() likes: no gating then
        self._gated = all(n.startswith("prompt_learner.") or n.startswith("point_encoder.blocks.blocks.") or not p.requires_grad
                          for n, p in model.named_parameters())
        pe_ = getattr(model, "point_encoder", None)
        dec = ("propagation_", "dgcnn_pro_", "conv1.", "bn1.", "conv2.")
        self._decoder_gated = hasattr(pe_, "decoder_gate") and all(
            (not p.requires_grad) or n.startswith("prompt_learner.") or
            (n.startswith("point_encoder.") and n[len("point_encoder."):].startswith(dec)) for n, p in model.named_parameters())
        self.bcast = BufferBroadcast(model) if distributed else None
        if distributed:
            # DDP's constructor: rank 0's parameters and buffers everywhere before the first step (see the function)
            self.init_broadcasts = broadcast_module_states(model)
        # BufferBroadcast re-bound the BatchNorm buffers to views of its flat tensor: every state-dict view, operand copy
        # and captured hipGraph made before that points at the orphaned storage
        if hasattr(model, "reset_caches"):
            model.reset_caches()
            # the text tower's half-vs-fp32 self-check runs HERE, explicitly, on the weights every rank now shares -- not inside
            # the first step on the text stream; under a process group the verdict is all-reduced (see the method)
            if hasattr(model, "calibrate_text_precision") and next(model.parameters()).is_cuda:
                model.calibrate_text_precision()
        else:
            for m in (model, getattr(model, "point_encoder", None)):
                if hasattr(m, "_sd"):
                    m._sd = None
                if hasattr(m, "_graphs"):
                    m._graphs.clear()

    def _prompt_stream(self, pc):
        """The side stream the text tower runs on (ULIP_WITH_IMAGE.forward), or None on CPU / when disabled."""
        model = self.model
        if not (pc.is_cuda and self.run_ahead and getattr(model, "overlap_text_tower", False)
                and hasattr(model, "text_stream")):
            return None
        return model.text_stream()

    def step(self, pc, label, check_finite=False, lengths=None):
        """One iteration (lengths: refused -- a ragged batch goes through model(pc, lengths=...) and a plain loss.backward(); the
        step's graphs and ahead stages are keyed by the cloud's shape alone).  On a GPU the prompt side of the step (zero_grad, text tower, its backward, the
        gradient all-reduce, AdamW, the logit_scale clamp) is queued on the model's text stream, the point
        tower and the loss on the caller's stream.  With a fully frozen point side (head_type 0) nothing the
        point tower reads changes between iterations, so the caller's stream does not wait for the optimizer:
        iteration i+1's point tower overlaps iteration i's text backward.  `loss` and `pred` are ordinary
        tensors of the caller's stream; parameters are final after `finish()`."""
        if lengths is not None:
            raise ValueError("Trainer.step takes no lengths: run a ragged batch through model(pc, lengths=...) and loss.backward()")
        model = self.model
        if self.grad_calibration is None and not self._dry:      # (the first step of THIS trainer, whatever `it` a resume set)
            self.calibrate_gradients(pc, label)
        side = self._side_used = self._prompt_stream(pc)
        pe = getattr(model, "point_encoder", None)
        if hasattr(pe, "group_ahead"):
            from . import graphs
            # the batch is known to be complete in device memory at a point the ahead stage can wait for: the caller vouches for it
            # (inputs_ready), or its producer attached the event of its copy (ppt_amd.data.DevicePrefetcher)
            ready = self.inputs_ready or graphs.ready_event(pc) is not None
            use = ready and pc.is_cuda and side is not None and (
                self.group_ahead_when_frozen or not self._point_side_frozen or getattr(pe, "group_ahead_pays_when_frozen", False))
            # DDP's per-forward buffer broadcast writes the BatchNorm running statistics on THIS stream while an ahead stage would
            # update them on the grouping stream, which deliberately does not wait for this one: an unordered read-modify-write
            # (ADVICE r3).  With the per-step broadcast the stages stay in order; the default (one broadcast in finish()) is
            # ordered through the stage's own event.
            if self.bcast is not None and self.broadcast_buffers_every_step:
                use = False
            pe.group_ahead = graphs.shared_group_stream() if use else None
            # the promise covers every tensor the stage reads; without it a tensor must carry its own copy event, and one derived
            # from the batch on this stream (a cast, a slice) sends the stage back behind this stream (graphs.wait_inputs)
            pe.inputs_vouched = bool(self.inputs_ready)
        tower_own = (self.tower_own_stream and self.inputs_ready and pc.is_cuda and side is not None and self._point_side_frozen
                     and self.fused_head and not self.extra_inputs)
        if hasattr(model, "forward_loss"):
            from . import graphs
            model.tower_stream = self._tower_used = graphs.shared_tower_stream() if tower_own else None
        main = torch.cuda.current_stream() if side is not None else None
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            self.sync.zero()                                        # optimizer.zero_grad()
        if self.lr_schedule is not None:                            # main_cls.py:184-185
            for g in self.optimizer.param_groups:
                g['lr'] = float(self.lr_schedule[min(self.it, len(self.lr_schedule) - 1)])
        if self.bcast is not None and self.broadcast_buffers_every_step:
            self.bcast.broadcast()
        try:
            if self.fused_head and self._point_side_frozen and not self.extra_inputs and hasattr(model, "forward_loss") \
                    and pc.is_cuda and label.dim() == 1:
                # nothing on the point side trains: logits, loss and the text-feature gradient in one graph-replayed node
                loss, pred = model.forward_loss(pc, label, self.criterion.label_smoothing)
            else:
                pred = model(pc, *self.extra_inputs)                # main_cls.py:194 / main_partseg.py:210
                loss = self._loss(pred.reshape(-1, pred.shape[-1]), label.reshape(-1))         # main_partseg.py:213
        finally:
            if hasattr(pe, "group_ahead"):
                pe.group_ahead = None       # the vouching covers this call's `pc` only: a forward outside step() stays in order
                pe.inputs_vouched = False
        if self.health is not None:
            self.health.check(2, loss)                              # (BIT_LOSS; on the caller's stream)
            self.health.check_labels(label, pred.shape[-1], self.criterion.ignore_index)
        if side is not None:
            side.wait_stream(main)
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            from . import autograd as _ag
            _ag.STATIC_GRADS_OK = self.sync.lazy                    # .grad dropped before every backward, read before the next replay
            try:
                loss.backward()                                     # main_cls.py:197 (retain_graph only served Q2)
            finally:
                _ag.STATIC_GRADS_OK = False
            if self.distributed and not self._dry:
                self.sync.all_reduce()
            if not self._dry:
                self._optimizer_step()
            if model.logit_scale.requires_grad and not self._dry:
                model.logit_scale.data.clamp_(0, 4.6052)            # main_cls.py:213 (frozen: clamped once in __init__)
        if side is not None and not self._point_side_frozen:
            pe = getattr(model, "point_encoder", None)
            if self._gated and getattr(pe, "param_gate", False) is None:
                # PointBERT with an un-frozen last block: only that block (and what follows) must see this update; the
                # frozen prefix of the next iteration runs ahead (point_encoder._PointEncoderFn waits on the event)
                pe.param_gate = side.record_event()
            elif self._decoder_gated and getattr(pe, "decoder_gate", False) is None:
                # part segmentation: everything that trains on the point side is the DECODER; the frozen backbone of the next
                # iteration does not wait for the optimizer (PointTransformer_partseg.forward waits in front of the decoder)
                pe.decoder_gate = side.record_event()
            else:
                main.wait_stream(side)                              # the point tower reads updated parameters
        if self._dry:                           # (calibrate_gradients: forward + backward only; not an iteration of the run)
            if side is not None:
                main.wait_stream(side)
            return loss, pred
        if self.health is not None:
            self._health_poll(side)
        if check_finite:
            if not math.isfinite(loss.item()):                      # main_cls.py:205-207
                raise FloatingPointError(f"Loss is {loss.item()}, stopping training")
            bad = self.nonfinite_grad_elements()
            if bad:
                raise FloatingPointError(f"{bad} gradient elements were not finite (skipped by the optimizer), stopping training")
        self.it += 1
        return loss, pred

    def calibrate_gradients(self, pc, label):
        """The mixed 16-bit mode checks the gradients it hands the optimizer against the fp32-grade mode, ONCE, on the first batch
        (VERDICT r5 #4 / weak #1, #2).  Why gradients and why the whole model: on checkpoint-LIKE weights (LayerNorm gains with 5-10 x
        outlier channels) the un-frozen block's gradients are 0.10-0.12 rel-L2 off although nothing overflows and the features are
        within 1 % -- and `tools/ckpt_like_h3_error.py` (profiles/r06_ckpt_like_h3_attribution.md) shows that the error is INHERITED:
        the un-frozen block alone on fp32 operands changes nothing (0.0956 -> 0.0955), blocks 0-10 alone make it worse (0.133), the
        tokenizer alone 0.084; only the WHOLE point tower on fp32-grade products brings it to 0.007.  The part-seg decoder's deep
        gradients behave the same way (0.11 whatever single stage is promoted).  So no per-stage
        promotion can answer it; what can is the split16 mode for the run.
        Two dry forward + backward passes of the caller's first batch -- current mode, then split16 -- eagerly on the caller's
        stream, with the same RNG draws (FPS starts, DropPath, Dropout: the generator state is restored before the second pass and
        after it, so the run itself draws what it would have drawn), BatchNorm buffers saved and restored, no optimizer step.
        Worst relative L2 difference over the trained tensors above `grad_check_threshold` (2e-2): policy "switch" leaves the model
        in split16 (a RuntimeWarning says so), "warn" only says so.  Under a process group every rank takes the MAX of the ranks'
        verdicts.  The result is kept in `grad_calibration`."""
        import warnings
        model = self.model
        self.grad_calibration = {"checked": False}
        trains_more = any(q.requires_grad and not n.startswith("prompt_learner.") for n, q in model.named_parameters())
        if (self.grad_check not in ("switch", "warn") or not trains_more or not pc.is_cuda
                or getattr(model, "precision_name", None) != "mixed16" or not hasattr(model, "set_precision")):
            return self.grad_calibration
        pe = getattr(model, "point_encoder", None)
        mods = [m_ for m_ in (model, pe) if m_ is not None and hasattr(m_, "use_hip_graphs")]
        flags = [(m_, m_.use_hip_graphs) for m_ in mods]
        run_ahead, ready = self.run_ahead, self.inputs_ready
        bufs = [(b, b.detach().clone()) for b in model.buffers() if b is not None]
        rng = torch.cuda.get_rng_state(pc.device)
        cpu_rng = torch.get_rng_state()

        def dry():
            torch.cuda.set_rng_state(rng, pc.device)
            torch.set_rng_state(cpu_rng)
            self.sync.zero()
            self.step(pc, label)
            torch.cuda.synchronize()
            with torch.no_grad():
                g = {n: q.grad.detach().clone() for n, q in model.named_parameters() if q.requires_grad and q.grad is not None}
                for b, keep in bufs:
                    b.copy_(keep)
            return g

        try:
            self._dry, self.run_ahead, self.inputs_ready = True, False, False
            for m_ in mods:
                m_.use_hip_graphs = False
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                g16 = dry()
                model.set_precision("split16")
                g32 = dry()
        finally:
            self._dry, self.run_ahead, self.inputs_ready = False, run_ahead, ready
            for m_, f in flags:
                m_.use_hip_graphs = f
            self.sync.zero()
            torch.cuda.set_rng_state(rng, pc.device)
            torch.set_rng_state(cpu_rng)
        worst, which = 0.0, None
        # (a tensor whose true gradient is ZERO -- a conv bias in front of a BatchNorm -- holds rounding noise in both modes: its
        # difference is measured against 1e-4 of the largest tensor norm, not against its own)
        norms = {n: float(a.norm()) for n, a in g32.items()}
        floor = 1e-4 * max([v for v in norms.values() if math.isfinite(v)] or [0.0])
        for n, a in g32.items():
            b = g16.get(n)
            den = max(norms[n], floor)
            if b is None or den == 0.0 or not math.isfinite(den):
                continue
            rel = float((b - a).norm()) / den
            if not (rel <= worst):                   # (NaN counts as the worst)
                worst, which = (rel if math.isfinite(rel) else float("inf")), n
        bad = not (worst <= self.grad_check_threshold)
        if self.distributed and dist.is_available() and dist.is_initialized():
            v = torch.tensor([1.0 if bad else 0.0, min(worst, 1e30)], dtype=torch.float64, device=pc.device)
            dist.all_reduce(v, op=dist.ReduceOp.MAX)
            bad, worst = bool(v[0].item() > 0), float(v[1].item())
        switched = bad and self.grad_check == "switch"
        self.grad_calibration = {"checked": True, "worst_rel_l2": worst, "tensor": which, "threshold": self.grad_check_threshold,
                                 "over": bad, "mode_after": "split16" if switched else "mixed16"}
        if not switched:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                model.set_precision("mixed16")
        if bad:
            warnings.warn(f"ppt_amd: on these weights the mixed 16-bit mode's gradients differ from the fp32-grade (split16) mode's by "
                          f"{worst:.3g} relative L2 on `{which}` (threshold {self.grad_check_threshold:g}; the error is inherited from "
                          "the frozen stages' 16-bit forward, no single stage's precision fixes it): "
                          + ("the run continues in the split16 mode (fp32 storage, products from hi + lo half pairs: ~0.4 x the "
                             "mixed mode's rate, fp32-grade gradients).  PPT_GRAD_CHECK=warn keeps the mixed mode." if switched else
                             "PPT_GRAD_CHECK=switch would continue in the split16 mode."), RuntimeWarning, stacklevel=3)
        if switched and self.health is None and os.environ.get("PPT_HEALTH", "1") != "0" and hasattr(model, "health"):
            from . import health                     # (split16 is a guarded mode: it gets the monitor a split16 Trainer starts with)
            self.health = model.health = health.Monitor(pc.device, every=int(os.environ.get("PPT_HEALTH_EVERY", "50")))
        return self.grad_calibration

    def _health_poll(self, side):
        """End of a step (the optimizer is queued): look at what the monitor saw since its last poll and answer it -- demote the
        half stage that overflowed (between steps: nothing of this step is in flight on the host any more, so the graphs and
        operand copies demote() drops are re-made by the NEXT forward); a corrupt label raises; events that no demotion can
        answer any more raise after health.GIVE_UP_AFTER polls instead of being skipped silently for the rest of the run."""
        from . import health
        mon = self.health
        # (under a process group every rank decides on the union of all ranks' events, at the same step: Monitor.poll_all_ranks)
        new = mon.poll_all_ranks(self.it, side) if (self.distributed and dist.is_initialized()) else mon.poll(self.it, side)
        if not new:
            return
        if new & health.BIT_LABEL:
            raise ValueError("ppt_amd: a label outside [0, C) that is not ignore_index reached the criterion "
                             "(nn.CrossEntropyLoss raises a device assert there): the loss of that step was NaN and the "
                             "optimizer skipped it -- a DATA error, not a numeric overflow")
        done = health.demote(self.model, new)
        if new == health.BIT_SPLIT and not done:
            return                          # (the process-wide split16 counter moved for another model of this process: not ours)
        self.demotions.append((self.it, new, done))
        if done:
            mon.unanswered = 0
            return
        mon.unanswered += 1
        if mon.unanswered >= health.GIVE_UP_AFTER:
            what = "point features" if new & health.BIT_POINT else ("loss" if new & health.BIT_LOSS else "gradient elements")
            raise FloatingPointError(f"ppt_amd: non-finite {what} in {mon.unanswered} consecutive health polls although every 16-bit "
                                     "stage already runs on bf16 operands (fp32's range): this is not a half overflow -- the optimizer "
                                     f"has skipped {mon.skipped_seen} gradient elements so far; stopping instead of skipping silently")

    def _loss(self, logits, labels):
        """self.criterion (main_cls.py:52: CrossEntropyLoss with label smoothing, mean reduction); on a GPU with <= 96 classes the
        loss and its gradient come from one pass over the logits (ops.cross_entropy_rows) instead of ~10 ATen kernels."""
        # (ppt_cross_entropy_rows treats label == ignore_index -- nn.CrossEntropyLoss's default -100 -- as an ignored row: zero loss
        # and gradient, left out of the mean, as ATen does; any OTHER label outside [0, C) makes the loss NaN where ATen raises a
        # device assert: step(check_finite=True) then stops as main_cls.py:205-207 does)
        ign = self.criterion.ignore_index
        if logits.is_cuda and logits.dtype == torch.float32 and logits.shape[1] <= 96 and labels.dtype == torch.int64 \
                and self.criterion.weight is None and self.criterion.reduction == 'mean' and not (0 <= ign < logits.shape[1]):
            return _CrossEntropyRows.apply(logits.contiguous(), labels.contiguous(), float(self.criterion.label_smoothing), int(ign))
        return self.criterion(logits, labels)

    def nonfinite_grad_elements(self):
        """How many gradient elements the AdamW kernels have skipped so far because they were not finite (one host read; the
        text stream's queued work is waited for)."""
        if self._skipped is None:
            return 0
        return int(self._skipped.item())

    def _optimizer_step(self, inv_scale=1.0):
        """AdamW over the tensors that got a gradient: ONE launch (ppt_adamw_step for a single tensor, ppt_adamw_multi for up to
        64 per launch: torch.optim.AdamW's arithmetic, state kept in the torch optimizer) instead of the ~10 multi-tensor kernels
        of the foreach implementation.  inv_scale: for callers that scaled their loss themselves (folded in first).
        Trainer(optim="adam" | "sgd"): the same launch shape on ppt_adam_multi / ppt_sgd_multi."""
        opt = self.optimizer
        params = [(g, p) for g in opt.param_groups for p in g['params'] if p.grad is not None]
        # the fused path is keyed on the optimizer's TYPE (torch.optim.AdamW subclasses Adam: no isinstance): AdamW as ever; Adam on
        # the same kernels where its weight_decay (an L2 term added to the gradient, not AdamW's decay) is 0, which is how
        # main_cls.py:57 builds it; SGD as main_cls.py:55 builds it (no momentum, no weight decay) on ppt_sgd_multi
        kind = _OPTIM_KINDS.get(type(opt))
        plain = kind == "adamw" or \
            (kind == "adam" and not any(g.get('weight_decay') or g.get('decoupled_weight_decay') for g, _ in params)) or \
            (kind == "sgd" and not any(g.get('momentum') or g.get('weight_decay') or g.get('nesterov') for g, _ in params))
        if not (self.fused_adamw and params and plain
                and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()
                        and p.grad.is_contiguous() and p.grad.dtype == torch.float32 for _, p in params)
                and not any(g.get('amsgrad') or g.get('maximize') for g, _ in params)):
            if inv_scale != 1.0 and params:
                with torch.no_grad():
                    torch._foreach_mul_([p.grad for _, p in params], inv_scale)
            opt.step()
            return
        from . import ops
        # the non-finite skip exists for the 16-bit backward stages only: in the fp32 parity mode the kernels get no counter and
        # behave as torch.optim.AdamW does -- a NaN gradient reaches the parameter and main_cls.py:205-207 stops the run
        # ... and split16 is NOT that mode: its operands pass through half's range (saturated + counted, health.BIT_SPLIT), its
        # backward stages are gradient-scaled like the 16-bit ones, so it keeps the skip as well
        guard = getattr(self.model, "precision", None) != torch.float32 or getattr(self.model, "split16", False)
        if self._skipped is None and guard:
            self._skipped = torch.zeros((1,), dtype=torch.int64, device=params[0][1].device)
            if self.health is not None:
                self.health.skipped = self._skipped
        prio = self.model.chain_priority() if hasattr(self.model, "chain_priority") else 0
        with torch.no_grad(), ops.wave_priority(prio):
            by_group = {}
            if kind == "sgd":                                # no state: torch.optim.SGD keeps none without momentum
                for g, p in params:
                    by_group.setdefault(id(g), (g, []))[1].append((p.data, p.grad))
                for g, items in by_group.values():
                    ops.sgd_multi(items, float(g['lr']), grad_scale=inv_scale, skipped=self._skipped if guard else None)
                params_state, by_group = (), {}
            else:
                params_state = params
            for g, p in params_state:
                st = opt.state[p]
                if not st:                                   # the layout torch.optim.AdamW._init_group creates
                    st['step'] = torch.tensor(0.0, dtype=torch.float32)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['step'] += 1
                by_group.setdefault(id(g), (g, []))[1].append((p.data, p.grad, st['exp_avg'], st['exp_avg_sq'], int(st['step'].item())))
            for g, items in by_group.values():
                b1, b2 = g['betas']
                hyper = (float(g['lr']), float(b1), float(b2), float(g['eps']), float(g['weight_decay']))
                if kind == "adam":
                    ops.adamw_multi(items, *hyper, grad_scale=inv_scale, skipped=self._skipped if guard else None, adam=True)
                elif len(items) == 1:
                    p_, g_, m_, v_, step = items[0]
                    ops.adamw_step(p_, g_, m_, v_, *hyper, step, grad_scale=inv_scale, skipped=self._skipped if guard else None)
                else:
                    ops.adamw_multi(items, *hyper, grad_scale=inv_scale, skipped=self._skipped if guard else None)
            for _, p in params:
                # the kernel wrote through a raw pointer: tell autograd's version counter, as torch.optim.AdamW's in-place ops
                # would.  Two caches key on it -- ULIP_WITH_IMAGE._te_cache (validate()'s text features) and
                # engine.WeightCache (the bf16 / transposed operand copies of a trained last-block weight) -- and would otherwise
                # keep serving the values of the FIRST step
                torch.autograd.graph.increment_version(p)

    def _drain_gate(self):
        pe = getattr(self.model, "point_encoder", None)
        dgate = getattr(pe, "decoder_gate", None)
        if dgate is not None:
            torch.cuda.current_stream().wait_event(dgate)
            pe.decoder_gate = None
        gate = getattr(pe, "param_gate", None)
        if gate is not None:
            torch.cuda.current_stream().wait_event(gate)
            pe.param_gate = None

    def finish(self):
        """Order the caller's stream after everything `step` queued and bring every rank's BatchNorm running statistics
        to rank 0's (call before reading parameters or buffers: evaluation, checkpointing)."""
        if self._side_used is not None:
            torch.cuda.current_stream().wait_stream(self._side_used)
        if self._tower_used is not None:
            torch.cuda.current_stream().wait_stream(self._tower_used)
        self._drain_gate()
        if self.bcast is not None and not self.broadcast_buffers_every_step:
            self.bcast.broadcast()


def reference_optimizer_state(model, optimizer):
    """optimizer.state_dict() re-indexed as if the optimizer had been built over model.parameters() (main_cls.py:58):
    one param group listing every parameter index, state entries keyed by a parameter's position in
    model.parameters().  Loadable by the reference's `optimizer.load_state_dict`."""
    sd = optimizer.state_dict()
    all_params = list(model.parameters())
    pos = {id(p): i for i, p in enumerate(all_params)}
    groups, state = [], {}
    assert len(sd['param_groups']) == len(optimizer.param_groups) == 1, "one param group, as main_cls.py:58"
    g_sd, g = sd['param_groups'][0], optimizer.param_groups[0]
    for local, p in zip(g_sd['params'], g['params']):
        if local in sd['state']:
            state[pos[id(p)]] = sd['state'][local]
    groups.append({**{k: v for k, v in g_sd.items() if k != 'params'}, 'params': list(range(len(all_params)))})
    return {'state': state, 'param_groups': groups}


def load_reference_optimizer_state(model, optimizer, ref_state):
    """Inverse of reference_optimizer_state: `ref_state` is an optimizer state dict indexed over model.parameters() (what
    main_cls.py:58 / main_partseg.py:62 build and `checkpoint_best.pt` holds); `optimizer` covers any subset of the model's
    parameters (train.Trainer: the trainable ones).  Hyper-parameters of the one param group and the per-parameter state
    (`step`, `exp_avg`, `exp_avg_sq`) are taken over; `step` stays a host tensor, the moments go to the parameter's device."""
    pos = {id(p): i for i, p in enumerate(model.parameters())}
    assert len(optimizer.param_groups) == 1 and len(ref_state['param_groups']) == 1, "one param group, as main_cls.py:58"
    g = optimizer.param_groups[0]
    for k, v in ref_state['param_groups'][0].items():
        if k != 'params':
            g[k] = v
    optimizer.state.clear()
    for p in g['params']:
        st = ref_state['state'].get(pos[id(p)])
        if st is None:
            continue
        optimizer.state[p] = {k: (v.detach().clone().to(p.device) if torch.is_tensor(v) and k != 'step' else
                                  (v.detach().clone().cpu() if torch.is_tensor(v) else v)) for k, v in st.items()}
    return optimizer


def checkpoint_payload(model, optimizer, epoch, best_acc, args, head_type=0, partseg=False, best_mean_class_iou=None,
                       best_mean_inst_iou=None):
    """The dict the reference writes as checkpoint_best.pt, with the reference's keys so that its readers
    work on the file (save_recog_feats.py:29-35, interpret_prompt.py:25-28, notebook/show_balls.py:219):
      recognition (main_cls.py:118-137): 'epoch', 'state_dict' (= {'learnable_tokens'}), 'last_block' (block 11 when
        head_type > 0, else None), 'optimizer', 'best_acc', 'args';
      part segmentation (main_partseg.py:127-143): 'epoch', 'state_dict_prompt', 'state_dict_partseg' (the whole point
        encoder), 'optimizer', 'best_test_acc', 'best_mean_class_iou', 'best_mean_inst_iou', 'args' (`best_acc` is the test
        accuracy there)."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()           # Trainer.step leaves the optimizer queued on the model's text stream
    opt = reference_optimizer_state(model, optimizer)
    # One key beyond the reference's (its readers index the keys they know and ignore the rest): the precision mode the run was IN
    # -- the mixed mode may have left for split16 at its first-batch gradient self-check (Trainer.calibrate_gradients), and a
    # resumed run must evaluate and continue in that mode, not re-decide (load_prompt_checkpoint applies it).
    mode = {'ppt_precision': getattr(model, 'precision_name', None)}
    if partseg:
        return {'epoch': epoch + 1, 'state_dict_prompt': model.prompt_learner.state_dict(),
                'state_dict_partseg': model.point_encoder.state_dict(), 'optimizer': opt, 'best_test_acc': best_acc,
                'best_mean_class_iou': best_mean_class_iou, 'best_mean_inst_iou': best_mean_inst_iou, 'args': args, **mode}
    return {'epoch': epoch + 1, 'state_dict': model.prompt_learner.state_dict(),
            'last_block': model.point_encoder.blocks.blocks[-1].state_dict() if head_type > 0 else None,
            'optimizer': opt, 'best_acc': best_acc, 'args': args, **mode}


def load_prompt_checkpoint(model, ckpt):
    """Inverse of checkpoint_payload for evaluation (save_recog_feats.py:29-35): prompt tokens + optional last block."""
    prompt = ckpt['state_dict'] if 'state_dict' in ckpt else ckpt['state_dict_prompt']      # main_cls.py:132 / main_partseg.py:135
    model.prompt_learner.load_state_dict(prompt)
    if ckpt.get('last_block'):
        blk = {'point_encoder.blocks.blocks.11.' + k: v for k, v in ckpt['last_block'].items()}
        model.load_state_dict(blk, strict=False)
    if ckpt.get('state_dict_partseg'):
        model.point_encoder.load_state_dict(ckpt['state_dict_partseg'])
    mode = ckpt.get('ppt_precision')       # (absent in the reference's own files: the model keeps the mode it was built with)
    if mode and hasattr(model, "set_precision") and getattr(model, "precision_name", mode) != mode:
        model.set_precision(mode)
    return model
