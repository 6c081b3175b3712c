"""The diffusion training step of the denoiser (BASELINE configs[3]).

What one step does, and the reference lines it mirrors:

    prepare_data   x0 = sal_map + 0.01 randn;  t0 = ONE integer in [0, T) for the whole rank-batch;
                   x_t = sqrt(a_hat[t0]) x0 + sqrt(1 - a_hat[t0]) randn         R/diffusion_trainer.py:106-117, 122-137,
                                                                                R/datasets/__init__.py:8-25
    forward        pred = model(x_t, t, conditioning)  (train-mode BN with per-rank statistics, dropout 0.1)
    loss           mse_weight * sum_{chw}(pred - x0)^2 .mean(batch)              R/models/sal_losses.py:189-192
    backward       hand-written HIP backward of every operator (autograd_ops.py)
    exchange       gradient MEAN over ranks -- the one collective of the path    (DDP, R/model.py:15)
    clip + Adam    clip_grad_norm_(1.0); Adam(lr 1e-4, (0.9, 0.999), eps 1e-8)   R/diffusion_trainer.py:228-235,
                                                                                R/util/utils.py:116-123

MI355X design.  Parameters, gradients and both Adam moments live in four flat fp32 buffers; every
``nn.Parameter`` (and its ``.grad``) is a view into them, so state_dict()/load_state_dict() keep working and
the reference's per-tensor loops collapse into three streaming kernels (csrc/optim.hip) -- norm, then a fused
clip+Adam that reads the norm from device memory (no host sync anywhere in the step).  Parameters are laid out
in REVERSE registration order, so gradients become final roughly front-to-back in the flat buffer during
backward; the buffer is cut into a few large buckets (default 32 MB: xGMI is point-to-point, a ring all-reduce
is per-link bound, so few large messages beat DDP's 25 MB x many) and each bucket's all-reduce (RCCL) is
launched asynchronously from a post-accumulate hook as soon as its last gradient lands, overlapping the rest of
backward.  Only parameters that can receive a gradient are exchanged (the reference buckets 72 M dead ones).
The DDP mean is not a separate pass: 1/world is folded into the norm and Adam kernels.
``noise_source="device"`` takes the step's random inputs -- both noises, the timestep, the dropout masks -- from the counter-based
generator the sampler uses (include/diffsal.h, "training noise"): a pure function of (seed, step, sample id), drawn on the device.
BatchNorm running statistics follow DDP's ``broadcast_buffers=True``: rank 0's buffers are broadcast (one flat
message) at the start of each step.
"""
from __future__ import annotations

import contextlib
import gc
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist
from torch import Tensor, nn

from .diffusion_utils import get_beta_schedule, to_torch


def _aligned(n: int, a: int = 64) -> int:
    return (n + a - 1) // a * a


def ema_rate_at(mu: float, updates: int, warmup: bool) -> float:
    """The rate of the EMA update that follows ``updates`` earlier ones: ``mu``, or with ``warmup`` the usual ramp
    ``min(mu, (1 + updates) / (10 + updates))`` -- 0.1 for the first update, ``mu`` from the first count at which the ramp
    reaches it.  A fixed 0.9999 would leave 86 % of the initial weights in the average after 1 500 steps, the length of a
    reference run (3 epochs at batch 48); the ramp forgets them within a few dozen updates.  Python floats, no device value."""
    mu, updates = float(mu), int(updates)
    if not warmup:
        return mu
    return min(mu, (1.0 + updates) / (10.0 + updates))


class FlatParams:
    """Flat fp32 storage for the trainable parameters of ``module`` (+ grads and optimizer moments).

    Layout: reverse registration order, each tensor padded to 64 elements (256 B) so every view is 16-byte aligned
    for the vectorised kernels.  Padding stays zero in all four buffers (Adam maps 0 -> 0).  ``shadow=True`` adds a fifth,
    ``shadow``: a copy of ``flat_p`` (what ``EMAHelper.register`` makes per tensor), padding zero as well (the EMA of 0 and 0)."""

    def __init__(self, module: nn.Module, bucket_bytes: int = 32 << 20, shadow: bool = False):
        params = [p for p in module.parameters() if p.requires_grad]
        if not params:
            raise ValueError("FlatParams: module has no trainable parameters")
        dev, dt = params[0].device, params[0].dtype
        if dt != torch.float32 or any(p.dtype != dt or p.device != dev for p in params):
            raise ValueError("FlatParams: all trainable parameters must be fp32 on one device")
        self.params: List[nn.Parameter] = params[::-1]
        self.offsets: List[int] = []
        off = 0
        for p in self.params:
            self.offsets.append(off)
            off += _aligned(p.numel())
        self.numel = off
        self.live_numel = sum(p.numel() for p in self.params)
        self.flat_p = torch.zeros(off, device=dev)
        self.flat_g = torch.zeros(off, device=dev)
        self.exp_avg = torch.zeros(off, device=dev)
        self.exp_avg_sq = torch.zeros(off, device=dev)
        for p, o in zip(self.params, self.offsets):
            view = self.flat_p[o:o + p.numel()].view(p.shape)
            view.copy_(p.data)
            p.data = view
            p.grad = None
        self.shadow: Optional[Tensor] = self.flat_p.clone() if shadow else None
        # buckets: contiguous ranges of whole tensors, closed once they reach bucket_bytes
        self.buckets: List[range] = []       # element ranges of the flat buffer
        self.bucket_of: List[int] = []       # parameter index -> bucket
        start, cap = 0, max(1, bucket_bytes // 4)
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            self.bucket_of.append(len(self.buckets))
            end = o + _aligned(p.numel())
            if end - start >= cap or i == len(self.params) - 1:
                self.buckets.append(range(start, end))
                start = end
        self.bucket_size = [0] * len(self.buckets)
        self.bucket_members: List[List[int]] = [[] for _ in self.buckets]
        for i, b in enumerate(self.bucket_of):
            self.bucket_size[b] += 1
            self.bucket_members[b].append(i)

    def grad_view(self, i: int) -> Tensor:
        p, o = self.params[i], self.offsets[i]
        return self.flat_g[o:o + p.numel()].view(p.shape)

    def zero_grad(self) -> None:
        """Clear the flat gradient and detach the parameters from it: with ``p.grad is None`` autograd hands over each
        freshly computed gradient tensor without an accumulation kernel; GradReducer gathers them bucket by bucket."""
        self.flat_g.zero_()
        for p in self.params:
            p.grad = None

    def gather(self, indices: Sequence[int]) -> None:
        """Copy the gradients autograd left on ``params[indices]`` into their flat slots (one multi-tensor kernel) and
        re-point ``.grad`` at the flat views.  Parameters without a gradient keep a zero slot."""
        todo = [i for i in indices if self.params[i].grad is not None
                and self.params[i].grad.data_ptr() != self.flat_g.data_ptr() + 4 * self.offsets[i]]
        if not todo:
            return
        if self.flat_g.is_cuda:
            from . import ops

            ops.multi_copy([self.params[i].grad for i in todo], [self.offsets[i] for i in todo], self.flat_g)
        else:  # host tensors: only the gloo tests of the bucket logic come here
            for i in todo:
                self.grad_view(i).copy_(self.params[i].grad)
        for i in todo:
            self.params[i].grad = self.grad_view(i)


class GradReducer:
    """Bucketed gradient gather + asynchronous SUM over the ranks of ``group`` (the mean's 1/world is applied by the
    consumer).

    ``flat.zero_grad()`` then ``arm()`` before backward; when the last gradient of a bucket has been produced its
    per-parameter hook gathers the bucket into the flat buffer (one kernel) and launches the bucket's exchange;
    ``finish()`` handles whatever is left (buckets holding parameters that received no gradient this step) and
    waits for all of them.

    Collectives are issued strictly in bucket order 0, 1, 2, ... on every rank: a bucket that completes while an earlier
    one is still open waits for it.  Ranks whose graphs differ (a parameter that receives no gradient on ONE rank only --
    its bucket closes in ``finish()`` there, in the middle of backward elsewhere) therefore still pair the same buffers in
    the same order; an order taken from hook arrival would pair different buckets across ranks and hang RCCL.

    ``exchange``: "allreduce" -- one ring all-reduce per bucket; "reduce_scatter" -- reduce-scatter of the bucket into
    per-rank shards followed by an all-gather of the shards (same result; on xGMI's point-to-point links the two halves
    can use all seven links of a GPU where a single ring is bound by one link per hop).  Buckets whose
    length is not a multiple of the world size, and backends without reduce-scatter (gloo), use the all-reduce.

    Parameters without a gradient.  The reference wraps the model in ``DistributedDataParallel(...,
    find_unused_parameters=True)`` (R/model.py:15): the set of parameters that receive no gradient may change from step to
    step and from rank to rank.  Here a bucket holding a parameter that never receives a gradient (audio-branch weights in
    visual-only training, an unused head) would stay open until ``finish()`` -- and, the order being fixed, so would every
    later bucket: the whole exchange serialised behind backward.  ``static_unused`` (default on) PREDICTS the set: the
    parameters that received no gradient on ANY rank in the first step (one small MAX all-reduce of the "fired" flags, issued
    by every rank at the end of its first step) are counted as done by ``arm()``, so their buckets close with the last
    gradient that does arrive.  The prediction is verified every step and a wrong one is repaired, on every rank together:
    a gradient that does arrive for such a parameter (on any rank, before or after its bucket went out) is kept out of the
    bucket; ``finish()`` MAX-reduces the per-parameter "fired" flags of the predicted set over the ranks (host data, a
    gloo side group: no device synchronisation), and the flagged parameters' gradients are summed over the ranks by one
    extra all-reduce each and leave the predicted set (``relearned`` lists them).  The result is the same sum DDP's
    ``find_unused_parameters=True`` produces, whatever the arrival order.  ``reset_unused()`` re-learns the set from
    scratch, ``static_unused = False`` turns the prediction off (every bucket with a gradient-less parameter then waits
    for ``finish()``)."""

    static_unused = True

    def __init__(self, flat: FlatParams, group=None, exchange_single_rank: bool = False, exchange: str = "allreduce"):
        if exchange not in ("allreduce", "reduce_scatter"):
            raise ValueError(f"GradReducer: exchange={exchange!r} (allreduce or reduce_scatter)")
        self.flat, self.group, self.mode = flat, group, exchange
        have_group = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if have_group else 1
        self.rank = dist.get_rank(group) if have_group else 0
        # whether the collective is issued: always with more than one rank; with ONE rank only on request (the call path --
        # hook, bucket gather, asynchronous all_reduce, wait -- then runs unchanged, RCCL reducing over a single rank)
        self.exchange = self.world > 1 or (have_group and bool(exchange_single_rank))
        self._native_rs = have_group and dist.get_backend(group) == "nccl"
        self._pending: List[int] = []
        self._launched: List[bool] = []
        self._ready: List[bool] = []
        self._next = 0
        self._work = []
        self._armed = False
        self._fired: List[bool] = []           # per parameter: its gradient hook ran this step
        self._unused = None                    # None: not learnt yet; else the set of parameters without a gradient on any rank
        self._side = None                      # gloo group for the per-step check of the prediction (host flags)
        self.relearned: List[int] = []         # parameters that left the predicted set in the last step
        self.launch_order: List[int] = []
        self.collectives: List[str] = []       # what was issued per bucket in the last step ("allreduce" / "reduce_scatter+all_gather")
        self.deferred = False                  # hooks and finish() only gather; finish_deferred() exchanges (captured steps)
        for i, p in enumerate(flat.params):
            p.register_post_accumulate_grad_hook(self._make_hook(i))

    def _make_hook(self, i: int) -> Callable:
        def hook(_param):
            if not self._armed:
                return
            b = self.flat.bucket_of[i]
            self._fired[i] = True
            if self._unused and i in self._unused:      # predicted to stay without a gradient, and got one: finish() repairs
                return
            self._pending[b] -= 1
            if self._pending[b] == 0:
                self._ready[b] = True
                self._drain()
        return hook

    def _drain(self) -> None:
        while self._next < len(self._ready) and self._ready[self._next]:
            self._launch(self._next)
            self._next += 1

    def _launch(self, b: int) -> None:
        if self._launched[b]:
            return
        self._launched[b] = True
        r = self.flat.buckets[b]
        self.launch_order.append(b)
        members = self.flat.bucket_members[b]
        if self._unused:       # a surprise gradient stays out of the bucket on every rank (finish() exchanges it on its own)
            members = [i for i in members if i not in self._unused]
        self.flat.gather(members)
        if self.exchange and not self.deferred:
            self._exchange(b)

    def _exchange(self, b: int) -> None:
        r = self.flat.buckets[b]
        buf = self.flat.flat_g[r.start:r.stop]
        n = buf.numel()
        if self.mode == "reduce_scatter" and n % self.world == 0:
            self.collectives.append("reduce_scatter+all_gather")
            shard = n // self.world
            mine = buf[self.rank * shard:(self.rank + 1) * shard]
            if self._native_rs:      # in place: the output is this rank's slice of the input (RCCL's in-place form)
                self._work.append(dist.reduce_scatter_tensor(mine, buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True))
                self._work.append(dist.all_gather_into_tensor(buf, mine, group=self.group, async_op=True))
            else:                    # gloo has no reduce-scatter: same arithmetic through its all-reduce (bookkeeping tests)
                self._work.append(dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True))
        else:
            self.collectives.append("allreduce")
            self._work.append(dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def arm(self) -> None:
        self._pending = list(self.flat.bucket_size)
        self._launched = [False] * len(self.flat.buckets)
        self._ready = [False] * len(self.flat.buckets)
        self._next = 0
        self._work, self.launch_order, self.collectives = [], [], []
        self._fired = [False] * len(self.flat.params)
        self.relearned = []
        if self._unused:
            for i in self._unused:
                b = self.flat.bucket_of[i]
                self._pending[b] -= 1
                if self._pending[b] == 0:
                    self._ready[b] = True      # launched by the first drain (first hook, or finish())
        self._armed = True

    def reset_unused(self) -> None:
        """Forget which parameters were found to receive no gradient; the next step learns the set again (call it on EVERY
        rank when the training graph changes, e.g. audio conditioning switched on)."""
        self._unused = None

    def _learn_unused(self) -> None:
        fired = torch.tensor([1.0 if f else 0.0 for f in self._fired], dtype=torch.float32, device=self.flat.flat_g.device)
        if self.world > 1:
            dist.all_reduce(fired, op=dist.ReduceOp.MAX, group=self.group)
        self._unused = {i for i, f in enumerate(fired.tolist()) if f == 0.0}
        if self._unused and self.world > 1 and self._side is None:
            # every rank holds the same set, so every rank comes here together.  The per-step check reduces HOST flags: over
            # the group itself when it is a gloo group, else over a gloo twin of it
            if dist.get_backend(self.group) == "gloo":
                self._side = self.group if self.group is not None else dist.group.WORLD
            else:
                ranks = dist.get_process_group_ranks(self.group if self.group is not None else dist.group.WORLD)
                try:
                    self._side = dist.new_group(ranks=ranks, backend="gloo", use_local_synchronization=True)
                except TypeError:       # older torch: every process of the default group must make the call
                    self._side = dist.new_group(ranks=ranks, backend="gloo")

    def _verify_unused(self) -> None:
        """The prediction against this step's facts, on every rank together; parameters it got wrong are exchanged now."""
        order = sorted(self._unused)
        flags = torch.tensor([1 if self._fired[i] else 0 for i in order], dtype=torch.int32)
        if self.world > 1:
            dist.all_reduce(flags, op=dist.ReduceOp.MAX, group=self._side)
        late = [i for i, f in zip(order, flags.tolist()) if f]
        if not late:
            return
        for i in late:
            p, slot = self.flat.params[i], self.flat.grad_view(i)
            if p.grad is not None and p.grad.data_ptr() != slot.data_ptr():
                slot.copy_(p.grad)                       # else: no gradient on this rank, the slot is still zero
            p.grad = slot
            if self.exchange:
                dist.all_reduce(slot, op=dist.ReduceOp.SUM, group=self.group)
            self._unused.discard(i)
        self.relearned = late

    def finish(self) -> None:
        for b in range(len(self.flat.buckets)):     # the rest, in bucket order
            self._ready[b] = True
        self._drain()
        if self.deferred:
            # nothing has been exchanged yet, so a gradient that arrived for a parameter predicted to stay without one simply
            # joins its bucket now; the prediction itself stays as it is (a replay is this very graph: nothing to verify)
            for i in sorted(self._unused or ()):
                p, slot = self.flat.params[i], self.flat.grad_view(i)
                if self._fired[i] and p.grad is not None and p.grad.data_ptr() != slot.data_ptr():
                    slot.copy_(p.grad)
                    p.grad = slot
            self._armed = False
            return
        for w in self._work:
            w.wait()
        self._work, self._armed = [], False
        if self._unused:
            self._verify_unused()
        if self.static_unused and self._unused is None:
            self._learn_unused()


    def finish_deferred(self) -> None:
        """The exchange of a step whose gathers ran with ``deferred`` set (a replayed graph): every bucket's collective, in
        bucket order 0, 1, 2, ... as always, same form and same buffers as ``_launch`` issues them, then the wait."""
        self._work, self.launch_order, self.collectives = [], [], []
        if self.exchange:
            for b in range(len(self.flat.buckets)):
                self.launch_order.append(b)
                self._exchange(b)
        for w in self._work:
            w.wait()
        self._work = []


class _StepGraph:
    """One captured training step: the graph, its static inputs and outputs, and what its launches read besides them."""
    __slots__ = ("warm", "graph", "sal", "cond", "ids", "loss", "losses", "norm", "keep")

    def __init__(self):
        self.warm, self.graph = 0, None


class FlatAdam(torch.optim.Optimizer):
    """``torch.optim.Optimizer`` face of ``DiffusionTrainStep``'s flat Adam: ONE parameter group whose ``lr`` / ``betas`` /
    ``eps`` / ``weight_decay`` are what the fused clip + Adam kernel reads at every step, so that the reference's scheduler
    (``optim.lr_scheduler.MultiStepLR(optimizer, milestones, gamma)``, R/util/utils.py:116-123, stepped once per epoch at
    R/diffusion_trainer.py:296) -- or any other ``torch.optim.lr_scheduler`` -- drives the learning rate unchanged.
    ``step()`` runs the owner's ``optimizer_step()``; the moments live in the owner's flat buffers (``state_dict()`` /
    ``load_state_dict()`` are the owner's: the ``torch.optim.Adam`` checkpoint format)."""

    def __init__(self, owner: "DiffusionTrainStep", params, lr, betas, eps, weight_decay):
        super().__init__(list(params), dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False))
        self._owner = owner

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise RuntimeError("FlatAdam.step: closures are not supported (the loss is computed by DiffusionTrainStep)")
        self._owner.optimizer_step()

    def zero_grad(self, set_to_none: bool = True):
        self._owner.flat.zero_grad()

    def add_param_group(self, param_group):
        if getattr(self, "param_groups", None):
            raise RuntimeError("FlatAdam keeps ONE parameter group (one flat buffer, one set of hyper-parameters)")
        super().add_param_group(param_group)

    def state_dict(self):
        return self._owner.state_dict()

    def load_state_dict(self, sd):
        self._owner.load_state_dict(sd)


class DiffusionTrainStep:
    """prepare_data -> forward -> loss -> backward -> gradient mean -> clip -> Adam, for ``model``.

    ``loss_fn(pred, x0) -> scalar tensor | dict with "total"`` replaces the built-in MSE (``mse_weight * sum_chw (pred - x0)^2``
    averaged over the batch) -- pass ``loss_config=config`` to get the reference's ``get_lossv2(config, pred, x0)["total"]``
    (R/diffusion_trainer.py:219, R/models/sal_losses.py:179-259: MSE or KL main term + weighted CC / SIM / NSS, every term with
    its HIP gradient, ``diff_sal_amd.sal_losses``).  ``self.optimizer`` is a ``torch.optim.Optimizer`` (``FlatAdam``) for
    learning-rate schedulers.

    ``model`` is a ``diff_sal_amd.SalUNet`` (called as ``model(x_t, t, feat_list, audio)``) or a
    ``VideoSaliencyModel`` (called as ``model({"img", "input", "audio"}, t)``, R/diffusion_trainer.py:212-218).
    Keyword names follow the YAML fields the reference trainer reads (R/cfgs/diffusion.yml:24-28, 39-60).

    ``training_target``: "x0" (default) or "noise" -- what the loss regresses the prediction onto, the reference's
    ``train_obj = x if training_target == "x0" else noise`` (R/diffusion_trainer.py:215); ``DiffusionSampler`` has the same switch.

    ``noise_source``: "torch" (default) is the reference's behaviour, bit for bit: ``torch.randn_like`` for the two noises, numpy's
    global generator for the one ``t0`` of the rank batch, dropout hashed from ``torch.initial_seed()`` and a call counter.
    "device" draws all of them from Philox4x32-10 keyed by ``seed`` and counted by (step, purpose, sample id) -- include/diffsal.h,
    "training noise" -- in one fused prepare launch and keyed dropout kernels; ``step(..., sample_ids=...)`` then names each sample
    (a host sequence, checked to be non-negative, or an int64 GPU tensor, which saves the upload), e.g. by its dataset index.
    What a sample sees no longer depends on its position in the batch, the batch size, the rank count or the loader's order, and
    a run continued from ``state_dict()`` by a fresh object built with the same ``seed`` sees what the uninterrupted run saw:
    seed and step live in two 64-bit device words (``train_key``), the step word is advanced on the device after backward and
    rewritten by ``load_state_dict``; no value travels from the host inside a step.
    ``t_mode``: "batch" (default) keeps the reference's ONE timestep per rank batch (R/diffusion_trainer.py:111); with device
    noise it is the draw of the FIRST sample id of the call, so it depends on the batch layout by nature.  "per_sample" -- the
    ordinary DDPM recipe, device noise only -- gives every sample the timestep of its own id.

    ``hip_graph`` (default False: nothing below applies): replay the step from a captured HIP graph.  Needs
    ``noise_source="device"`` (torch's generator and numpy's ``t0`` are host state, a ``ValueError`` otherwise).  The first
    ``graph_warmup`` calls of ``step()`` (default 2: library load, discovery of the weight packs, workspace caches, the reducer's
    unused set) run eagerly; the next one captures fused prepare, forward, loss, backward with the bucket gathers, the step word's
    advance, the gradient norm and clip + Adam on ONE stream (``torch.cuda.graph``, no side stream inside) and from then on a
    ``step()`` is: copy ``sal_maps``, every tensor of ``cond`` and the sample ids into static buffers, form the optimizer's
    numbers for ``step_count + 1`` from the parameter group's CURRENT ``lr`` / ``betas`` / ``eps`` / ``weight_decay``
    (``ops.adam_args``) and enqueue their copy to the device block the captured Adam reads (``ops.adam_step_args``) -- a
    learning-rate scheduler acts on the next step without a new capture --, replay, then the host's bookkeeping (``step_count``,
    the step word's range, ``parameters_updated()`` so that a later ``eval()`` forward repacks, the optimizer face's step hooks
    and scheduler counters).  Results are bit-identical to the eager step's.
    * One capture per signature: shapes and dtypes of the inputs, the keys of ``cond``, which parameters require a gradient,
      ``grad_clip``, ``store_clipped_grad``, ``t_mode``, ``training_target``, ``gaussian_dequantization``, ``mse_weight``, the
      identity of ``loss_fn`` and the world size.  A new signature runs one eager step of its own, then captures; a signature
      that returns replays its old capture.  ``graph_captures`` / ``graph_replays`` count.  Every capture keeps its own
      activations: memory grows by about one step's peak per signature.
    * ``step(..., t0=)`` / ``noise=`` / ``dequant_noise=``, a call while ``ops.PROFILE`` is set, a call inside somebody else's
      capture and a call after ``reducer.reset_unused()`` (until the set is learnt again) run eagerly, for that call.
    * ``step()`` returns the STATIC loss tensor, and ``last_losses`` / ``last_norm`` are static too: the next step of the same
      signature overwrites them in stream order.  Work enqueued on the stream before that step reads this step's values
      (``train``'s meters add them to their device sums right after each step, so they do); ``clone()`` what must outlive it.
    * ``load_state_dict`` (and ``model.load_state_dict``) write ``train_key``, the flat buffers and the model's buffers in place,
      so a live capture goes on from the loaded state.  A failed capture raises with its cause chained: no fallback.
    * With an exchange (more than one rank, or ``exchange_single_rank``) the reducer runs deferred: the captured hooks only
      gather; after each replay ``reducer.finish_deferred()`` issues the bucket collectives in bucket order and waits, and the
      step word's advance, norm and Adam run eagerly after it.  The buffer broadcast runs eagerly before the replay.  This gives
      up the overlap of the exchange with backward.  Every rank must pass the same ``hip_graph`` (checked at construction).
    Measured on the full audio-visual step (224 x 384, batch 4, one MI355X): the replay is NOT faster, 66.0 ms
    against 65.9 ms eager on the same box -- the step is bound by the device, whose eager host issue takes 56.5 ms.  It cuts the
    host's time in a step to 2.2 ms, costs 0.7 s for the capturing call and 64 MB of peak memory (14 544 against 14 480 MB).

    ``ema`` (default None: nothing below applies): keep an exponential moving average of the trained parameters at rate
    ``ema`` in [0, 1] -- the reference's ``model.ema`` / ``model.ema_rate`` (R/cfgs/diffusion.yml) and its ``EMAHelper`` --
    in a fifth flat buffer, ``flat.shadow``, that starts as a copy of the parameters (``EMAHelper.register``).  The update
    ``shadow = (1 - mu) p + mu shadow`` runs inside the clip + Adam kernel on the new parameters (``ops.adam_ema_step``): no launch
    of its own, and bit-equal to ``EMAHelper.update`` after the step.  ``ema_warmup=True`` ramps the rate (``ema_rate_at``); the
    rate of a step is formed on the host from ``ema_updates``, the count of updates done, and reaches a captured step through the
    device block its Adam reads, so a replay needs no new capture for it.  Every rank computes the same shadow; none is exchanged.
    BatchNorm running statistics are buffers and are not averaged, as in ``EMAHelper``.
    * ``ema_weights()``: a context manager inside which the model HOLDS the average -- weights and shadow are exchanged in place
      by one launch on entry and again on exit (``ops.ema_swap``: bits move, nothing is rounded, so the exit restores the weights
      exactly), with ``parameters_updated()`` after each.  No address changes, so a live capture stays valid.  ``step()``,
      ``optimizer_step()``, ``load_ema_state_dict()`` and a nested entry raise ``RuntimeError`` inside it.
    * ``ema_state_dict()`` / ``load_ema_state_dict()`` carry the shadow by parameter name (``EMAHelper.state_dict()``'s layout), the
      update count, the rate and the warm-up switch; ``state_dict()`` stays ``torch.optim.Adam``'s format."""

    def __init__(self, model: nn.Module, *, lr: float = 1e-4, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                 weight_decay: float = 0.0, grad_clip: float = 1.0, mse_weight: float = 1.0,
                 beta_schedule: str = "cosine", beta_start: float = 1e-4, beta_end: float = 0.02,
                 num_diffusion_timesteps: int = 1000, gaussian_dequantization: bool = True,
                 bucket_mb: float = 32.0, process_group=None, broadcast_buffers: bool = True,
                 store_clipped_grad: bool = False, exchange_single_rank: bool = False,
                 loss_fn: Optional[Callable] = None, loss_config=None, exchange: str = "allreduce",
                 noise_source: str = "torch", seed: int = 0, t_mode: str = "batch", training_target: str = "x0",
                 hip_graph: bool = False, graph_warmup: int = 2, ema: Optional[float] = None, ema_warmup: bool = False):
        if ema is not None and not 0.0 <= float(ema) <= 1.0:
            raise ValueError(f"DiffusionTrainStep: ema={ema!r} must be a rate in [0, 1] (or None)")
        if ema_warmup and ema is None:
            raise ValueError("DiffusionTrainStep: ema_warmup=True needs ema=<rate>")
        if hip_graph and noise_source != "device":
            raise ValueError("DiffusionTrainStep: hip_graph=True needs noise_source='device': torch's generator and numpy's t0 "
                             "are host state, which a replayed graph would not advance")
        if noise_source not in ("torch", "device"):
            raise ValueError(f"DiffusionTrainStep: noise_source={noise_source!r} (torch or device)")
        if t_mode not in ("batch", "per_sample"):
            raise ValueError(f"DiffusionTrainStep: t_mode={t_mode!r} (batch or per_sample)")
        if training_target not in ("x0", "noise"):
            raise ValueError(f"DiffusionTrainStep: training_target={training_target!r} (x0 or noise)")
        if t_mode == "per_sample" and noise_source != "device":
            raise ValueError("DiffusionTrainStep: t_mode='per_sample' needs noise_source='device': the torch path draws ONE t0 "
                             "per rank batch from numpy's global generator, as the reference does, and has no per-sample draw")
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"DiffusionTrainStep: seed must be in [0, 2^64), got {seed}")
        self.noise_source, self.seed, self.t_mode, self.training_target = noise_source, seed, t_mode, training_target
        self.model = model
        self.grad_clip, self.mse_weight = float(grad_clip), float(mse_weight)
        if loss_fn is not None and loss_config is not None:
            raise ValueError("DiffusionTrainStep: give loss_fn or loss_config, not both")
        if loss_config is not None:
            from . import sal_losses

            def loss_fn(pred, x0, _cfg=loss_config):            # R/diffusion_trainer.py:219
                return sal_losses.get_lossv2(_cfg, pred, x0)
        self.loss_fn = loss_fn
        self.last_losses: Optional[Dict] = None      # the loss dictionary of the last step when loss_fn returns one
        self.gaussian_dequantization = bool(gaussian_dequantization)
        self.store_clipped_grad = bool(store_clipped_grad)
        betas = to_torch(get_beta_schedule(beta_schedule, beta_start=beta_start, beta_end=beta_end,
                                           num_diffusion_timesteps=num_diffusion_timesteps))
        alphas_hat = (1.0 - betas).cumprod(dim=0)
        self.sqrt_alphas_hat = torch.sqrt(alphas_hat)
        self.sqrt_one_minus_alphas_hat = torch.sqrt(1.0 - alphas_hat)
        self.num_timesteps = int(betas.shape[0])
        self.ema: Optional[float] = None if ema is None else float(ema)
        self.ema_warmup = bool(ema_warmup)
        self.ema_updates = 0                 # EMA updates done: what ema_rate_at counts from
        self._ema_swapped = False            # inside ema_weights(): flat_p holds the average, shadow the weights
        self.flat = FlatParams(model, int(bucket_mb * (1 << 20)), shadow=self.ema is not None)
        self.optimizer = FlatAdam(self, self.flat.params, float(lr), (float(beta1), float(beta2)), float(eps), float(weight_decay))
        self.group = process_group
        self.reducer = GradReducer(self.flat, process_group, exchange_single_rank, exchange)
        self.world = self.reducer.world
        self.broadcast_buffers = bool(broadcast_buffers) and self.reducer.exchange
        self.step_count = 0
        self.last_norm: Optional[Tensor] = None
        self._rng = np.random  # the reference draws t0 from numpy's global generator (diffusion_trainer.py:111)
        # device noise: the train key {seed, step} and the two coefficient tables, uploaded once (the tables are the very fp32
        # tensors the torch path reads its by-value coefficients from, so both paths multiply by the same bits)
        self.train_key: Optional[Tensor] = None
        dev = self.flat.flat_p.device
        if noise_source == "device" and dev.type == "cuda":
            from . import ops

            self.train_key = ops.train_key(seed, 0, dev)
            self._tab_a = self.sqrt_alphas_hat.to(torch.float32).contiguous().to(dev)
            self._tab_b = self.sqrt_one_minus_alphas_hat.to(torch.float32).contiguous().to(dev)
        self.hip_graph, self.graph_warmup = bool(hip_graph), max(1, int(graph_warmup))
        self.graph_captures = self.graph_replays = 0
        self._graphs: Dict[tuple, _StepGraph] = {}
        self._packs = None               # this trainer's own weight-pack table: a capture replays its launch
        self._adam_dev: Optional[Tensor] = None
        self._in_graph = False           # the device half of optimizer_step already ran inside the replayed graph
        if self.hip_graph:
            from . import ops

            self._packs = ops._PackBatch()
        if self.world > 1:               # every rank replays or none does: a mixed group would pair different collectives
            mine = 1.0 if self.hip_graph else 0.0
            seen = torch.tensor([mine, -mine], dtype=torch.float32, device=dev)
            dist.all_reduce(seen, op=dist.ReduceOp.MAX, group=process_group)
            hi, lo = seen.tolist()
            if hi != -lo:
                raise ValueError("DiffusionTrainStep: hip_graph differs between the ranks of the group; pass the same value on all")

    # hyper-parameters live in the optimizer face's single parameter group (what a scheduler rewrites)
    def _hp(self, key):
        return self.optimizer.param_groups[0][key]

    lr = property(lambda self: float(self._hp("lr")), lambda self, v: self.optimizer.param_groups[0].__setitem__("lr", float(v)))
    betas = property(lambda self: tuple(float(b) for b in self._hp("betas")),
                     lambda self, v: self.optimizer.param_groups[0].__setitem__("betas", (float(v[0]), float(v[1]))))
    eps = property(lambda self: float(self._hp("eps")), lambda self, v: self.optimizer.param_groups[0].__setitem__("eps", float(v)))
    weight_decay = property(lambda self: float(self._hp("weight_decay")),
                            lambda self, v: self.optimizer.param_groups[0].__setitem__("weight_decay", float(v)))

    @property
    def param_groups(self):
        return self.optimizer.param_groups

    # ---- R/diffusion_trainer.py:78-120 (training branch) ----
    def _sample_ids(self, sample_ids, sal_maps: Tensor, pinned: bool = False) -> Tensor:
        """Argument rules of the device-noise path, then the ids as an int64 tensor next to ``sal_maps``."""
        from . import ops

        if sample_ids is None:
            raise ValueError("DiffusionTrainStep: noise_source='device' needs sample_ids (one non-negative id per sample)")
        ids = ops.sample_ids(sample_ids, sal_maps.device, sal_maps.shape[0], pinned)       # raises for a CPU tensor, after the id checks
        if self.train_key is None:
            raise RuntimeError("diff_sal_amd device noise runs on the GPU only (no CPU fallback); the model is on the CPU")
        return ids

    def prepare_data(self, sal_maps: Tensor, *, t0: Optional[int] = None, noise: Optional[Tensor] = None,
                     dequant_noise: Optional[Tensor] = None, sample_ids=None):
        """sal_maps [B,1,H,W] in [0,1] -> (x0, x_t, t [B] int64, noise).  With device noise: ``sample_ids`` names the samples,
        ``noise`` / ``dequant_noise`` cannot be given, ``t0`` fixes the timestep of all samples, and the call is a pure function
        of (seed, step_count, ids) -- calling it twice before a step returns the same tensors."""
        from . import ops

        if self.noise_source == "device":
            if noise is not None or dequant_noise is not None:
                raise ValueError("DiffusionTrainStep: noise= / dequant_noise= cannot be given with noise_source='device' "
                                 "(the noise is drawn on the device from seed, step and sample_ids)")
            ids = self._sample_ids(sample_ids, sal_maps)
            mode = "fixed" if t0 is not None else self.t_mode
            return ops.train_prepare(sal_maps.contiguous().float(), ids, self.train_key, self._tab_a, self._tab_b,
                                     dq_scale=0.01 if self.gaussian_dequantization else 0.0, t_mode=mode, t0=t0)
        if sample_ids is not None:
            raise ValueError("DiffusionTrainStep: sample_ids mean nothing to torch's generator; use noise_source='device'")
        x = sal_maps.contiguous().float()
        if self.gaussian_dequantization:
            dq = torch.randn_like(x) if dequant_noise is None else dequant_noise
            x = ops.axpbypcz(x, 1.0, dq, 0.01)
        if noise is None:
            noise = torch.randn_like(x)
        if t0 is None:
            t0 = int(self._rng.randint(0, self.num_timesteps))
        t = torch.full((x.shape[0],), t0, dtype=torch.int64, device=x.device)
        x_t = ops.axpbypcz(x, float(self.sqrt_alphas_hat[t0]), noise, float(self.sqrt_one_minus_alphas_hat[t0]))
        return x, x_t, t, noise

    def _forward(self, x_t: Tensor, t: Tensor, cond: Dict, dropout_key=None) -> Tensor:
        from .sal_unet import SalUNet

        with contextlib.ExitStack() as scope:
            if dropout_key is not None:      # every denoiser in the module tree, the one nested in a VideoSaliencyModel included
                for m in self.model.modules():
                    if isinstance(m, SalUNet):
                        scope.enter_context(m.dropout_key_scope(dropout_key))
            if isinstance(self.model, SalUNet):
                return self.model(x_t, t, cond["feat_list"], cond.get("audio_feat"))
            data = dict(cond)
            data["input"] = x_t
            return self.model(data, t)

    def _flatten_buffers(self) -> None:
        """Floating-point buffers (BatchNorm running statistics) become views into ONE flat tensor, once: the per-step broadcast
        of rank 0's buffers (DDP's ``broadcast_buffers=True``, R/model.py:15) is then a single collective on that tensor -- no
        gather before it and no copy kernel per buffer after it (the denoiser + encoders hold ~100 such buffers; the copies were
        most of the exchange's exposed time at one rank).  Kernels that update running statistics write through the views."""
        bufs = [b for b in self.model.buffers() if b.dtype == torch.float32 and b.numel() > 0]
        self._flat_buffers = None
        if not bufs or any(b.device != bufs[0].device for b in bufs):
            return
        off, offs = 0, []
        for b in bufs:
            offs.append(off)
            off += _aligned(b.numel())
        flat = torch.zeros(off, device=bufs[0].device, dtype=torch.float32)
        for b, o in zip(bufs, offs):
            view = flat[o:o + b.numel()].view(b.shape)
            view.copy_(b)
            b.data = view
        self._flat_buffers = flat

    def _sync_buffers(self) -> None:
        stale = False
        if getattr(self, "_flat_buffers", None) is not None:       # module.to(...) / a re-registered buffer: the views are gone
            lo = self._flat_buffers.data_ptr()
            hi = lo + 4 * self._flat_buffers.numel()
            stale = any(not (lo <= b.data_ptr() < hi) for b in self.model.buffers() if b.dtype == torch.float32 and b.numel() > 0)
        if getattr(self, "_flat_buffers", "unset") == "unset" or stale:
            self._flatten_buffers()
        src = dist.get_global_rank(self.group, 0) if self.group is not None else 0
        if self._flat_buffers is not None:
            dist.broadcast(self._flat_buffers, src=src, group=self.group)
        others = [b for b in self.model.buffers() if b.dtype.is_floating_point and b.dtype != torch.float32 and b.numel() > 0]
        for b in others:           # none in the reference's model; kept exact for foreign modules
            dist.broadcast(b, src=src, group=self.group)

    def loss_and_backward(self, x0: Tensor, x_t: Tensor, t: Tensor, cond: Dict, sample_ids=None, _captured: bool = False) -> Tensor:
        """Forward + loss + backward + gradient exchange; leaves the rank-SUMMED gradient in ``flat.flat_g``.  ``x0`` is the
        regression target (the forward-process noise when ``training_target="noise"``).  With device noise ``sample_ids`` key
        the dropout masks (required then); the masks of forward and backward both read the device step word, which
        ``optimizer_step`` advances afterwards."""
        from . import autograd_ops as ag

        dropout_key = None
        if self.noise_source == "device":
            dropout_key = (self._sample_ids(sample_ids, x_t), self.train_key)
        elif sample_ids is not None:
            raise ValueError("DiffusionTrainStep: sample_ids mean nothing to torch's generator; use noise_source='device'")

        self.model.train()
        if self.broadcast_buffers and not _captured:       # a captured step broadcasts eagerly, before its replay
            self._sync_buffers()
        self.flat.zero_grad()
        self.reducer.arm()
        from . import ops

        with ops.batched_packs(self._packs):        # every parameter's kernel layouts (forward, data-gradient) rebuilt by one launch
            pred = self._forward(x_t, t, cond, dropout_key)
            if self.loss_fn is None:
                loss = ag.mse_loss(pred, x0, self.mse_weight / x0.shape[0])
                self.last_losses = None
            else:
                out = self.loss_fn(pred, x0)
                if isinstance(out, dict):
                    self.last_losses = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}
                    loss = out["total"]
                else:
                    self.last_losses, loss = None, out
                if not torch.is_tensor(loss) or loss.dim() != 0 or not loss.requires_grad:
                    raise RuntimeError("DiffusionTrainStep: loss_fn must return a scalar tensor (or a dict with 'total') that "
                                       "carries a gradient to the prediction")
            loss.backward()
        self.reducer.finish()
        return loss.detach()

    def _parameters_updated(self) -> None:
        bump = getattr(self.model, "parameters_updated", None)
        if bump is not None:
            bump()
        for m in self.model.modules():  # nested denoiser inside a VideoSaliencyModel
            if m is not self.model and hasattr(m, "parameters_updated"):
                m.parameters_updated()

    def _device_tail(self, args_dev: Optional[Tensor] = None) -> None:
        """Step word, gradient norm, clip + Adam: the launches after the exchange.  ``args_dev``: Adam's numbers come from that
        device block (a captured step) instead of the launch arguments."""
        from . import ops

        if self.train_key is not None:
            ops.train_key_advance(self.train_key)      # same stream as backward, so after the last reader of the old step
        gscale = 1.0 / self.world
        norm = ops.grad_norm(self.flat.flat_g, gscale) if self.grad_clip > 0 else None
        self.last_norm = norm
        f = self.flat
        if self.ema is not None:
            if args_dev is not None:
                ops.adam_ema_step_args(f.flat_p, f.flat_g, f.exp_avg, f.exp_avg_sq, f.shadow, args_dev, norm, self.store_clipped_grad)
            else:
                ops.adam_ema_step(f.flat_p, f.flat_g, f.exp_avg, f.exp_avg_sq, f.shadow, step=self.step_count + 1,
                                  lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay, gscale=gscale,
                                  norm=norm, max_norm=self.grad_clip, store_clipped_grad=self.store_clipped_grad,
                                  ema_mu=ema_rate_at(self.ema, self.ema_updates, self.ema_warmup))
        elif args_dev is not None:
            ops.adam_step_args(f.flat_p, f.flat_g, f.exp_avg, f.exp_avg_sq, args_dev, norm, self.store_clipped_grad)
        else:
            ops.adam_step(f.flat_p, f.flat_g, f.exp_avg, f.exp_avg_sq, step=self.step_count + 1,
                          lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay, gscale=gscale, norm=norm,
                          max_norm=self.grad_clip, store_clipped_grad=self.store_clipped_grad)

    def optimizer_step(self) -> None:
        from . import ops

        self._not_in_ema_weights("optimizer_step()")
        if self.train_key is not None:
            ops.train_draw(self.step_count + 1, 0)     # the host mirror of the draw word's 27-bit step field
        if not self._in_graph:
            self._device_tail()
        self.step_count += 1
        if self.ema is not None:
            self.ema_updates += 1
        self._parameters_updated()

    def step(self, sal_maps: Tensor, cond: Dict, *, t0: Optional[int] = None, noise: Optional[Tensor] = None,
             dequant_noise: Optional[Tensor] = None, sample_ids=None) -> Tensor:
        """One training step on this rank's clips; returns the (detached, device-resident) loss.  ``sample_ids``: one id per
        sample, required with (and only with) ``noise_source="device"``.  With ``hip_graph=True`` the returned tensor is static:
        the next step overwrites it in stream order (see the class)."""
        self._not_in_ema_weights("step()")
        if self.hip_graph and t0 is None and noise is None and dequant_noise is None and self._graphable(sal_maps):
            return self._graph_step(sal_maps, cond, sample_ids)
        return self._eager_step(sal_maps, cond, t0=t0, noise=noise, dequant_noise=dequant_noise, sample_ids=sample_ids)

    def _eager_step(self, sal_maps: Tensor, cond: Dict, *, t0=None, noise=None, dequant_noise=None, sample_ids=None) -> Tensor:
        if self.noise_source == "device" and noise is None and dequant_noise is None:
            sample_ids = self._sample_ids(sample_ids, sal_maps)        # checked and uploaded once for prepare and dropout
        x0, x_t, t, nz = self.prepare_data(sal_maps, t0=t0, noise=noise, dequant_noise=dequant_noise, sample_ids=sample_ids)
        loss = self.loss_and_backward(nz if self.training_target == "noise" else x0, x_t, t, cond, sample_ids=sample_ids)
        self.optimizer.step()          # the torch.optim.Optimizer face: step hooks and lr_scheduler bookkeeping see the step
        return loss

    # ---- hip_graph=True: one captured step per signature ----
    def _graphable(self, sal_maps: Tensor) -> bool:
        from . import ops

        if not torch.is_tensor(sal_maps) or not sal_maps.is_cuda or self.train_key is None:
            return False                    # the eager path raises what it always raised
        if ops.PROFILE is not None or torch.cuda.is_current_stream_capturing():
            return False                    # per-launch events cannot be recorded inside a capture; no capture inside a capture
        # the unused set is learnt by a host read at the end of a step: not inside a capture
        return not (self.reducer.static_unused and self.reducer._unused is None and self.step_count > 0 and self._graphs)

    @staticmethod
    def _cond_tensors(cond: Dict):
        """(structure for the signature, the tensors in a fixed order)"""
        desc, flat = [], []
        for k in sorted(cond):
            v = cond[k]
            if torch.is_tensor(v):
                desc.append((k, "t", tuple(v.shape), v.dtype))
                flat.append(v)
            elif isinstance(v, (list, tuple)) and all(torch.is_tensor(x) for x in v):
                desc.append((k, "l", tuple((tuple(x.shape), x.dtype) for x in v)))
                flat += list(v)
            elif v is None:
                desc.append((k, "n"))
            else:
                raise ValueError(f"DiffusionTrainStep(hip_graph=True): cond[{k!r}] must be a tensor, a list of tensors or None")
        return tuple(desc), flat

    @staticmethod
    def _cond_like(cond: Dict, flat: List[Tensor]) -> Dict:
        out, it = {}, iter(flat)
        for k in sorted(cond):
            v = cond[k]
            out[k] = next(it) if torch.is_tensor(v) else (None if v is None else [next(it) for _ in v])
        return out

    def _signature(self, sal_maps: Tensor, desc) -> tuple:
        return (tuple(sal_maps.shape), sal_maps.dtype, desc, tuple(p.requires_grad for p in self.model.parameters()),
                self.grad_clip, self.store_clipped_grad, self.t_mode, self.training_target, self.gaussian_dequantization,
                self.mse_weight, id(self.loss_fn), self.world)

    def _captured_step(self, ent: _StepGraph):
        x0, x_t, t, nz = self.prepare_data(ent.sal, sample_ids=ent.ids)
        loss = self.loss_and_backward(nz if self.training_target == "noise" else x0, x_t, t, ent.cond, sample_ids=ent.ids,
                                      _captured=True)
        if not self.reducer.exchange:
            self._device_tail(self._adam_dev)
        return loss

    def _capture(self, ent: _StepGraph, sal_maps: Tensor, cond: Dict, flat: List[Tensor], ids: Tensor) -> None:
        from . import ops

        dev = sal_maps.device
        ent.sal, ent.ids = torch.empty_like(sal_maps).copy_(sal_maps), ids.clone()
        ent.cond = self._cond_like(cond, [torch.empty_like(v).copy_(v) for v in flat])
        if self._adam_dev is None:
            size = ops.adam_args_size() if self.ema is None else ops.adam_ema_args_size()
            self._adam_dev = torch.zeros((_aligned(size),), dtype=torch.uint8, device=dev)
        self._parameters_updated()          # whatever an eval() forward cached since the last step is packed again inside
        with ops.batched_packs(self._packs):
            pass                            # the pack table is built (a host upload) and the dead entries leave it now
        torch.cuda.synchronize(dev)
        # Dead reference cycles that own device state (an earlier trainer with its captures and pools) are destroyed by whichever
        # thread the collector next runs on; inside a global-mode capture their frees and graph destructions are illegal calls and
        # abort the process.  torch.cuda.graph collected before a capture up to torch 2.9 and no longer does by default: collect
        # here, and keep the collector off until the capture has ended (backward runs on autograd's threads: the switch is
        # process-wide).
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        graph = torch.cuda.CUDAGraph()
        self.reducer.deferred = self.reducer.exchange
        try:
            with torch.cuda.graph(graph):
                ent.loss = self._captured_step(ent)
        except Exception as e:              # the user asked for a graph: no silent eager step
            raise RuntimeError(f"DiffusionTrainStep(hip_graph=True): capturing the training step failed "
                               f"({type(e).__name__}: {e})") from e
        finally:
            self.reducer.deferred = False
            if gc_was_on:
                gc.enable()
        ent.losses, ent.norm = self.last_losses, self.last_norm
        # the table and the packed weights the captured launches address stay alive with the capture
        ent.keep = (self._packs.table, [e[1] for e in self._packs.entries.values()])
        ent.graph = graph
        self.graph_captures += 1

    def _graph_step(self, sal_maps: Tensor, cond: Dict, sample_ids) -> Tensor:
        from . import ops

        ids = self._sample_ids(sample_ids, sal_maps, pinned=True)      # a pageable upload would stall the host behind the replay
        desc, flat = self._cond_tensors(cond)
        sig = self._signature(sal_maps, desc)
        ent = self._graphs.get(sig)
        if ent is None:
            ent = self._graphs[sig] = _StepGraph()
        need = self.graph_warmup if len(self._graphs) == 1 else 1
        if ent.graph is None and ent.warm < need:
            ent.warm += 1
            return self._eager_step(sal_maps, cond, sample_ids=ids)
        ops.train_draw(self.step_count + 1, 0)             # the step word's range, before anything is enqueued
        if ent.graph is None:
            self._capture(ent, sal_maps, cond, flat, ids)
        else:
            ent.sal.copy_(sal_maps)
            ent.ids.copy_(ids)
            for d, s in zip(self._cond_tensors(ent.cond)[1], flat):
                d.copy_(s)
        self.model.train()
        if self.reducer.exchange:
            if self.broadcast_buffers:
                self._sync_buffers()
        else:
            # a fresh pinned block every step: the host allocator hands it out again only after this copy has run
            hp = dict(step=self.step_count + 1, lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay,
                      gscale=1.0 / self.world, max_norm=self.grad_clip)
            if self.ema is None:
                block = ops.adam_args(**hp)
            else:       # this step's rate travels with Adam's numbers: a warm-up that moves every step needs no new capture
                block = ops.adam_ema_args(ema_mu=ema_rate_at(self.ema, self.ema_updates, self.ema_warmup), **hp)
            self._adam_dev[:block.numel()].copy_(block, non_blocking=True)
        ent.graph.replay()
        self.graph_replays += 1
        self.last_losses, self.last_norm = ent.losses, ent.norm
        if self.reducer.exchange:
            self.reducer.finish_deferred()
            self.optimizer.step()           # step word, norm and Adam eagerly, after the exchange
        else:
            self._in_graph = True
            try:
                self.optimizer.step()       # hooks, scheduler counters and this object's bookkeeping; Adam ran in the graph
            finally:
                self._in_graph = False
        return ent.loss

    # ---- the averaged weights ----
    def _not_in_ema_weights(self, what: str) -> None:
        if self._ema_swapped:
            raise RuntimeError(f"DiffusionTrainStep: {what} inside ema_weights(): the model holds the averaged weights; leave the "
                               "context first")

    def _need_ema(self, what: str) -> None:
        if self.ema is None:
            raise RuntimeError(f"DiffusionTrainStep: {what} needs a trainer built with ema=<rate>")

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the model's trained parameters are the average (see the class)."""
        from . import ops

        self._need_ema("ema_weights()")
        self._not_in_ema_weights("ema_weights()")
        ops.ema_swap(self.flat.flat_p, self.flat.shadow)
        self._ema_swapped = True
        self._parameters_updated()
        try:
            yield self
        finally:
            ops.ema_swap(self.flat.flat_p, self.flat.shadow)
            self._ema_swapped = False
            self._parameters_updated()

    def _named_slots(self):
        """(name, parameter, offset in the flat buffers) of every trained parameter, in ``named_parameters()`` order"""
        slot = {id(p): k for k, p in enumerate(self.flat.params)}
        return [(name, p, self.flat.offsets[slot[id(p)]]) for name, p in self.model.named_parameters() if id(p) in slot]

    def ema_state_dict(self) -> Dict:
        """``{"shadow": {parameter name: tensor}, "updates", "mu", "warmup"}``; ``shadow`` is ``EMAHelper.state_dict()``'s layout
        (the trained parameters by name), cloned out of the flat buffer."""
        self._need_ema("ema_state_dict()")
        src = self.flat.flat_p if self._ema_swapped else self.flat.shadow
        return {"shadow": {name: src[o:o + p.numel()].view(p.shape).clone() for name, p, o in self._named_slots()},
                "updates": int(self.ema_updates), "mu": float(self.ema), "warmup": bool(self.ema_warmup)}

    def load_ema_state_dict(self, sd: Dict) -> None:
        """Inverse of ``ema_state_dict``; ``{"shadow": EMAHelper.state_dict()}`` alone loads too (``updates`` then restarts at 0,
        rate and warm-up stay this trainer's).  Every name and shape is checked before anything is written; the shadow is written
        in place, so a live capture goes on from it."""
        self._need_ema("load_ema_state_dict()")
        self._not_in_ema_weights("load_ema_state_dict()")
        if not isinstance(sd, dict) or "shadow" not in sd:
            raise ValueError("load_ema_state_dict expects {'shadow': {parameter name: tensor}, 'updates', 'mu', 'warmup'}")
        shadow, slots = sd["shadow"], self._named_slots()
        missing = [name for name, _, _ in slots if name not in shadow]
        extra = sorted(set(shadow) - {name for name, _, _ in slots})
        if missing or extra:
            raise ValueError(f"load_ema_state_dict: missing {missing}, unexpected {extra}")
        for name, p, _ in slots:
            if tuple(shadow[name].shape) != tuple(p.shape):
                raise ValueError(f"load_ema_state_dict: shadow of {name!r} has shape {tuple(shadow[name].shape)}, the parameter "
                                 f"{tuple(p.shape)}")
        mu = float(sd.get("mu", self.ema))
        if not 0.0 <= mu <= 1.0:
            raise ValueError(f"load_ema_state_dict: mu={mu!r} must be in [0, 1]")
        for name, p, o in slots:
            self.flat.shadow[o:o + p.numel()].view(p.shape).copy_(shadow[name])
        self.ema, self.ema_warmup = mu, bool(sd.get("warmup", self.ema_warmup))
        self.ema_updates = int(sd.get("updates", 0))

    def reset_ema(self) -> None:
        """The shadow restarts as a copy of the current parameters with no update done: ``EMAHelper.register`` after a load."""
        self._need_ema("reset_ema()")
        self._not_in_ema_weights("reset_ema()")
        self.flat.shadow.copy_(self.flat.flat_p)
        self.ema_updates = 0

    # ---- checkpoint surface of torch.optim.Adam (R/diffusion_trainer.py:187-193, 263-268: "optim_dict") ----
    def _indexed_params(self):
        """(index in ``model.parameters()`` order -- the numbering torch.optim.Adam(model.parameters()) uses --, slot in the
        flat buffers or None for parameters that are not trained)."""
        slot = {id(p): k for k, p in enumerate(self.flat.params)}
        return [(i, p, slot.get(id(p))) for i, p in enumerate(self.model.parameters())]

    def state_dict(self) -> Dict:
        """The ``torch.optim.Adam.state_dict()`` format: ``state[i] = {step, exp_avg, exp_avg_sq}`` per trained parameter
        in ``model.parameters()`` order, one ``param_groups`` entry with lr / betas / eps / weight_decay -- what the
        reference trainer saves as ``optim_dict`` and loads back into ``optim.Adam`` (R/util/utils.py:116-123), so
        checkpoints move both ways.  The moments are gathered out of the flat buffers through ``FlatParams.offsets``."""
        idx = self._indexed_params()
        state = {}
        if self.step_count > 0:          # torch creates a parameter's state at its first step
            for i, p, k in idx:
                if k is None:
                    continue
                o = self.flat.offsets[k]
                state[i] = {"step": torch.tensor(float(self.step_count)),
                            "exp_avg": self.flat.exp_avg[o:o + p.numel()].view(p.shape).clone(),
                            "exp_avg_sq": self.flat.exp_avg_sq[o:o + p.numel()].view(p.shape).clone()}
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": [i for i, _, _ in idx]}
        for k, v in self.optimizer.param_groups[0].items():     # whatever else lives in the group (a scheduler's initial_lr)
            if k != "params" and k not in group:
                group[k] = v
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd: Dict) -> None:
        """Inverse of ``state_dict``; also accepts a checkpoint written by ``torch.optim.Adam`` over the same module.
        Validates the parameter count and every moment's shape before touching anything."""
        if "state" not in sd or "param_groups" not in sd:
            raise ValueError("load_state_dict expects the torch.optim.Adam format {'state': ..., 'param_groups': [...]}")
        groups = sd["param_groups"]
        idx = self._indexed_params()
        n_saved = sum(len(g["params"]) for g in groups)
        if n_saved != len(idx):
            raise ValueError(f"optimizer checkpoint covers {n_saved} parameters, the module has {len(idx)}")
        if any(g.get("amsgrad", False) for g in groups):
            raise ValueError("amsgrad checkpoints are not supported (the reference sets amsgrad from config, default false)")
        # parameter numbering of the checkpoint = concatenation of the groups' param lists, in module order
        order = [i for g in groups for i in g["params"]]
        state = {int(k): v for k, v in sd["state"].items()}
        steps = set()
        staged = []
        for pos, (i, p, k) in enumerate(idx):
            st = state.get(order[pos])
            if st is None:
                continue
            if k is None:
                raise ValueError(f"checkpoint has optimizer state for parameter {i}, which is not trainable here")
            for name in ("exp_avg", "exp_avg_sq"):
                if tuple(st[name].shape) != tuple(p.shape):
                    raise ValueError(f"optimizer state {name} of parameter {i}: shape {tuple(st[name].shape)} != {tuple(p.shape)}")
            steps.add(int(float(st["step"])))
            staged.append((k, p, st))
        if len(steps) > 1:
            raise ValueError(f"per-parameter step counts differ ({sorted(steps)}): the flat optimizer keeps one step count")
        step_count = steps.pop() if steps else 0
        new_key = None
        if self.train_key is not None:
            from . import ops

            new_key = ops.train_key(self.seed, step_count, self.train_key.device)      # checks the step's range
        self.flat.exp_avg.zero_()
        self.flat.exp_avg_sq.zero_()
        for k, p, st in staged:
            o = self.flat.offsets[k]
            self.flat.exp_avg[o:o + p.numel()].view(p.shape).copy_(st["exp_avg"])
            self.flat.exp_avg_sq[o:o + p.numel()].view(p.shape).copy_(st["exp_avg_sq"])
        if new_key is not None:
            self.train_key.copy_(new_key)          # the stream continues where the checkpointed run stopped
        self.step_count = step_count
        g0 = groups[0]
        self.lr = float(g0.get("lr", self.lr))
        self.betas = tuple(float(b) for b in g0.get("betas", self.betas))
        self.eps = float(g0.get("eps", self.eps))
        self.weight_decay = float(g0.get("weight_decay", self.weight_decay))
        for k, v in g0.items():
            if k not in ("params", "lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable",
                         "differentiable", "fused"):
                self.optimizer.param_groups[0][k] = v
