"""One training iteration in the reference's order (cdf_alignment_admm/resnet-20-cifar-10/main.py:288-374):
zero_grad x2 -> forward -> CE + trans_loss -> backward -> SGD.step(idx, w_cdf, w_pdf, lam, lam2) ->
ADMM_OPT.step(alterD_idx, gamma_idx, Ds, alterDs, gammas, mus, rhos).

The list gathering of main.py:313-369 is done once (indices) / per step (tensors) without host syncs;
`capture()` records the whole iteration into one HIP graph (static input buffers), which removes the
per-launch host overhead that dominates the small CIFAR shapes."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import config, paths
from .fused import DeferredLosses, DeferredWgrads, HeadCEFn, head_ce_supported, prequantize_weights
from .optimizer import ADMM_OPT, SGD, sgd_admm_step
from .schedule import HyperBlock, Schedule, office_rate, ramp


_PROBE = "alignq_capture_probe"


def retained_graph_params(params):
    """Parameters whose AccumulateGrad node is kept alive by an autograd graph of an EARLIER iteration (a retained loss / output
    tensor, or ADMM.D kept with its graph as utils/admm.py:25 does).  Such a node is bound to the stream that iteration ran on;
    a backward inside a stream capture then makes autograd synchronise that stream with the capturing one, which pulls it into
    the capture: hipStreamEndCapture finds an unjoined stream (ROCm 7.2: a segmentation fault - round 4's crash when a step was
    captured after eager iterations whose outputs were still referenced).  Found by tagging: a node nobody else holds dies when
    the probe's temporary graph goes, and the next lookup creates an untagged one."""
    token = object()
    live = [p for p in params if p.requires_grad]
    # self-check: a parameter created HERE cannot be part of any earlier graph.  If its node survives the probe's
    # temporary graph too, something pins accumulation nodes (hooks registered on the node itself, a torch that caches it): the
    # probe would then call EVERY parameter stale and capture() would blame the caller's tensors for it
    fresh = torch.nn.Parameter(torch.zeros(1))
    for p in live + [fresh]:
        p.expand_as(p).grad_fn.next_functions[0][0].metadata[_PROBE] = token
    stale = []
    for p in live + [fresh]:
        acc = p.expand_as(p).grad_fn.next_functions[0][0]
        if acc.metadata.get(_PROBE) is token:
            stale.append(p)
        acc.metadata.pop(_PROBE, None)
    if any(p is fresh for p in stale):
        raise RuntimeError("retained_graph_params: the probe is unusable in this process - the gradient-accumulation node of a "
                           "parameter created inside the probe outlived its temporary graph (this torch build, or a component "
                           "that registers hooks on the accumulation nodes themselves, keeps them alive), so a retained autograd "
                           "graph cannot be told from a pinned node here; capture() cannot verify its precondition")
    return stale


def release_step_graphs(admms):
    """What the step itself may keep of an earlier iteration's autograd graph: ADMM.D with its history (the exact-global and the
    unfused sites store D as the reference does, utils/admm.py:25; the fused sites store a detached D)."""
    for a in admms:
        if a.D is not None and a.D.grad_fn is not None:
            a.D = a.D.detach()


def assert_no_retained_graph(params, who):
    stale = retained_graph_params(params)
    if stale:
        raise RuntimeError(
            f"{who}: {len(stale)} parameter(s) are still referenced by the autograd graph of an earlier iteration (a loss / output "
            "tensor of an eager step that is still alive).  Their gradient-accumulation nodes are bound to the stream that "
            "iteration ran on; capturing a backward that reuses them pulls that stream into the capture (hipStreamEndCapture "
            "crashes on the unjoined stream).  Drop those tensors (del the step's outputs, or .detach() them) and call capture() "
            "again.")


def _detached(outs):
    """The step's results without their autograd history: the backward already ran inside the step, and a result that kept the
    iteration's graph alive would keep its gradient-accumulation nodes alive too (retained_graph_params)."""
    return tuple(t.detach() if torch.is_tensor(t) else t for t in outs)


class _CapturedStep:
    """The HIP-graph lifecycle every training step shares: static input buffers, the warm-up and the capture into one graph (or
    two around the eager data-parallel all-reduce), replay, the eager fallback for an off-shape batch and re-capture.  A
    subclass builds `model`, `channels_last`, `optimizer_t`, `optimizer_admm`, `admms` and `_wgrads`, calls `_init_capture` from
    its __init__ and supplies `_forward_backward(*inputs, set_to_none, overlap)` (overlap=True: an eager iteration, which runs
    the grad_hook itself) and `_optimizer_steps()`."""

    def _init_capture(self, grad_hook, device_hyper=False, **slots):
        """device_hyper: the learning rates (and the `slots`: alpha / coef) live in a device row (alignq_amd.schedule.HyperBlock)
        the optimizer kernels read at run time, so set_lr / new_epoch / a per-iteration alpha keep a captured graph."""
        self._hyper = None                  # the HyperBlock (device_hyper=True)
        self.grad_hook = grad_hook          # e.g. the data-parallel all-reduce (alignq_amd.dp)
        self._schedule = None               # a table that alignq_hyper_advance walks, one row per iteration (set_schedule)
        self._fresh_pending = False         # the row says fresh = 1 and no iteration has consumed it yet
        if device_hyper:
            self._refuse_hook_with_hyper(grad_hook, True)
            dev = next(self.model.parameters()).device
            self._hyper = HyperBlock(dev, len(self.optimizer_t.param_groups))
            self.optimizer_t.attach_hyper(self._hyper)
            # a new optimizer: the first iteration starts the momentum (utils/optimizer.py:222-224)
            self._hyper.set(lr=[g["lr"] for g in self.optimizer_t.param_groups], fresh=1, **slots)
            self._fresh_pending = True
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._graph2: Optional[torch.cuda.CUDAGraph] = None
        self._static = None                 # the input buffers the graphs read
        self._outs = None                   # the captured iteration's results
        self._recapture = False             # capture from the next eager call's inputs (new_epoch)
        self._producer = None               # a loader whose fill is the first work of the (first) graph (set_producer)

    def _refuse_hook_with_hyper(self, hook, hyper):
        """Data parallelism splits the capture around the eager all-reduce: the table's node and the hand-over of `fresh` are only
        defined for the one-graph step."""
        if hook is not None and hyper:
            raise NotImplementedError(f"{type(self).__name__}: device_hyper=True with a grad_hook (data parallel: alignq_amd.dp.attach "
                                      "/ attach_office) is not covered")

    def _iteration(self, *inputs, set_to_none=True):
        if self._hyper is not None:
            # (a hook can be installed by assignment after the step was built; dp.attach / attach_office refuse it themselves)
            self._refuse_hook_with_hyper(self.grad_hook, True)
        if self._schedule is not None:
            self._schedule.advance()        # this iteration's row; inside a capture: the node in front of the iteration
        outs = self._forward_backward(*inputs, set_to_none=set_to_none, overlap=True)
        self._optimizer_steps()
        return _detached(outs)

    def _backward(self, roots, grads=None, set_to_none=True):
        """All filter-gradient slab reductions of the backward in one launch behind it (fused.DeferredWgrads).  A
        DeferredWgrads(fresh_grads=True) promises that every .grad is None when the backward starts: only after set_to_none."""
        wg = self._wgrads
        if wg is not None and (set_to_none or not wg.fresh_grads):
            with wg:
                torch.autograd.backward(roots, grads)
                wg.flush()
        else:
            torch.autograd.backward(roots, grads)

    def _consumed(self):
        """Behind every iteration that has been enqueued (eager, warm-up, fallback or replay; never inside a capture): the one
        iteration that was to start the momentum afresh has done so - the row is staged again with fresh = 0.  (With a table
        the rows carry `fresh` themselves.)"""
        if self._fresh_pending:
            self._fresh_pending = False
            if self._schedule is None:
                self._hyper.set(fresh=0)

    def _need_hyper(self, what):
        if self._hyper is None:
            raise RuntimeError(f"{type(self).__name__}.{what}: needs a step built with device_hyper=True")

    def set_schedule(self, table):
        """Drive the row from `table` (float32 [iterations, n_groups + 3]: alignq_amd.schedule.multistep / office_dann /
        office_dsan): every iteration first launches alignq_hyper_advance - row min(cursor, rows - 1) into the
        row, cursor + 1 - eagerly or, after `capture`, as a node in front of the iteration (behind the producer's).  The cursor
        therefore counts the iterations run, warm-ups included (`seek`).  A run is then replays with no host write at all;
        set_lr, a per-call alpha / lambd and new_epoch's staging are the table's business and refused or skipped.  Call it
        before `capture`: an existing capture is dropped.  A table is not detached again (the row would keep its last
        values while the host's mirror holds older ones): attach another table, or build a new step."""
        self._need_hyper("set_schedule")
        if table is None:
            raise ValueError(f"{type(self).__name__}.set_schedule: a schedule table cannot be detached; attach another one or "
                             "build a new step")
        self._schedule = Schedule(self._hyper, table)
        self._graph = self._graph2 = None
        self._fresh_pending = False
        return self

    def _host_stages(self, what):
        if self._schedule is not None:
            raise RuntimeError(f"{type(self).__name__}.{what}: the schedule table owns the row (set_schedule); put the value into "
                               "the table")

    def seek(self, i):
        """The next iteration reads row `i` of the table (e.g. after the warm-up, or resuming a run)."""
        if self._schedule is None:
            raise RuntimeError(f"{type(self).__name__}.seek: no schedule table (set_schedule)")
        self._schedule.seek(i)
        return self

    def current_hyper(self):
        """The device row (lr per group, alpha, coef, fresh) and the table's cursor (None without one): one host read, for logs."""
        self._need_hyper("current_hyper")
        out = self._hyper.read()
        out["cursor"] = None if self._schedule is None else self._schedule.position()
        return out

    def __call__(self, *inputs):
        if self._graph is None:
            outs = self._iteration(*inputs)
            self._consumed()
            if self._recapture:
                self._recapture = False
                self.capture(*inputs, warmup=0)
            return outs
        if any(x.shape != s.shape for x, s in zip(inputs, self._static)):
            # off-shape batch (the reference's loaders have no drop_last: CIFAR's last batch is 80 of 128): a captured
            # graph only fits its static shapes, so this one iteration runs eagerly
            return self._eager_fallback(*inputs)
        if self._producer is not None:
            raise RuntimeError(f"{type(self).__name__}: the captured graph fills its own inputs from the attached loader (a replay "
                               "would overwrite the given tensors' copies); call next(), or capture without a producer")
        # a loader that writes its batches straight into `static_inputs()` (the target of its host-to-device copy) hands the
        # same tensors back: nothing to stage
        for x, s in zip(inputs, self._static):
            if x is not s:
                s.copy_(x, non_blocking=True)
        return self._replay()

    def _replay(self):
        if self._hyper is not None:
            self._refuse_hook_with_hyper(self.grad_hook, True)
        self._graph.replay()
        self._consumed()
        if self._graph2 is not None:
            # data-parallel: only the collectives run eagerly between the two captured halves (the buckets are packed in the
            # first graph and unpacked at the start of the second)
            self.grad_hook.reduce()
            self._graph2.replay()
        return self._outs

    def set_producer(self, loader):
        """Attach an input producer (alignq_amd.data.DeviceLoader; None detaches): the next `capture` records
        `loader.record(*static_inputs)` - one batch launch, which also moves the cursor on - as the first node of the (first) graph, and
        `next()` replays it: batch n of the epoch on the n-th call after `loader.begin_epoch`.  Without a producer every graph is
        node for node what it was.  An existing capture is dropped (the step runs eagerly until `capture` is called again)."""
        if loader is not None and not (hasattr(loader, "record") and hasattr(loader, "next_batch")):
            raise TypeError("set_producer: expected a DeviceLoader")
        self._producer = loader
        self._graph = self._graph2 = None
        return self

    def next(self):
        """The iteration on the attached loader's coming batch: one replay, no host work on the batch and no tensor passed.  The
        short last batch of an epoch (the reference's loaders have no drop_last) is filled eagerly and takes the eager fallback."""
        p = self._producer
        if p is None or self._graph is None:
            raise RuntimeError(f"{type(self).__name__}.next: needs set_producer(loader) and capture(...) first")
        rows = self._coming_rows(p)
        if rows[0] == 0:
            raise RuntimeError(f"{type(self).__name__}.next: the loader's epoch is exhausted; call loader.begin_epoch")
        if rows != self._captured_rows():
            return self._eager_fallback(*p.next_batch())
        p.skip(*rows)
        return self._replay()

    def _coming_rows(self, producer):
        """Rows of the producer's coming batch(es), and `_captured_rows`: the rows the graph was captured with."""
        return (producer.next_batch_size(),)

    def _captured_rows(self):
        return (self._static[0].shape[0],)

    def _record_inputs(self, static):
        """Inside a capture, in front of the iteration: the producer's batch launch into the graph's input buffers."""
        if self._producer is not None:
            self._producer.record(*static)

    def static_inputs(self):
        """The buffers the captured graph reads ((x, y) or (xs, ys, xt); images in the step's memory format).  Fill them in
        place — e.g. as the destination of the loader's host-to-device copy — and call the step with these very tensors: the
        per-step staging copies (a layout-converting one for NCHW input) are skipped.  None before `capture`."""
        return self._static

    def _eager_fallback(self, *inputs):
        """The graph's own gradient / D tensors (which p.grad and ADMM.D name between replays) are put back afterwards."""
        opts = [o for o in (self.optimizer_t, self.optimizer_admm) if o is not None]
        params = list({id(p): p for o in opts for g in o.param_groups for p in g["params"]}.values())
        keep_g, keep_D = [p.grad for p in params], [m.D for m in self.admms]
        # a data-parallel hook rebinds its flat bucket to the off-shape layout during this iteration; the graphs keep packing
        # into / unpacking from the bucket that was current at capture, so the eager reduce() between them must see that one
        # again afterwards (otherwise it all-reduces the stale short-batch buffer and the replicas diverge silently)
        hook = self.grad_hook
        keep_hook = hook.snapshot() if hasattr(hook, "snapshot") else None
        try:
            outs = self._iteration(*inputs)
            self._consumed()
            return outs
        finally:
            for p, g in zip(params, keep_g):
                p.grad = g
            for m, D in zip(self.admms, keep_D):
                m.D = D
            if hasattr(hook, "restore"):
                hook.restore(keep_hook)

    def _assert_momentum_buffers(self, who):
        """A momentum buffer created INSIDE a capture is baked into the graph with first=1 (buf = grad on every replay:
        silently momentum-free training) and lives in the graph's private pool.  Capture therefore needs every parameter the
        step updates to own its buffer already, i.e. at least one eager step since the optimizer was created."""
        opt = self.optimizer_t
        momentum = [p for g in opt.param_groups if g["momentum"] != 0 for p in g["params"]]
        if self._hyper is not None and all("momentum_buffer" in opt.state[p] for p in momentum):
            return                  # (SGD.attach_hyper created every buffer; the row's `fresh` slot starts the momentum)
        if momentum and (all(p.grad is None for g in opt.param_groups for p in g["params"])
                         or any(p.grad is not None and "momentum_buffer" not in opt.state[p] for p in momentum)):
            raise RuntimeError(f"{who}: a parameter has no momentum buffer yet; run at least one eager iteration "
                               "(capture(..., warmup>=1)) before capturing the step")

    def _static_clones(self, inputs):
        """The buffers a captured graph reads: clones of `inputs`, images in the step's memory format."""
        return tuple(t.clone(memory_format=torch.channels_last) if (self.channels_last and t.dim() == 4) else t.clone()
                     for t in inputs)

    def _warm_up(self, static, warmup):
        """`warmup` eager iterations on a side stream (allocator pools, pointer tables, MIOpen plans), then a device synchronise."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._iteration(*static, set_to_none=False)
                self._consumed()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()

    def _capture(self, inputs, warmup):
        who = f"{type(self).__name__}.capture"
        self._refuse_hook_with_hyper(self.grad_hook, self._hyper is not None)      # before the warm-up touches the model
        release_step_graphs(self.admms)
        assert_no_retained_graph([p for g in self.optimizer_t.param_groups for p in g["params"]], who)
        static = self._static_clones(inputs)
        self._warm_up(static, warmup)
        self._assert_momentum_buffers(who)
        release_step_graphs(self.admms)          # (an unfused site of the warm-up keeps D with its graph)
        # inside the capture grads are re-created (set_to_none=True): no zero-fill and no accumulate-add per
        # parameter; the fresh grad tensors live in the graph's private pool at fixed addresses and stay
        # referenced by p.grad, so the captured optimizer kernels (and the eager all-reduce) see them on replay.
        self.optimizer_t.zero_grad(set_to_none=True)
        if self.optimizer_admm is not None:
            self.optimizer_admm.zero_grad(set_to_none=True)
        hook = self.grad_hook
        split = hook is not None and hook.active()
        # An initialised process group matters even WITHOUT a hook: its watchdog thread polls HIP events of earlier collectives,
        # which the default (global) capture mode forbids while ANY stream captures; under capture_error_mode="thread_local" HIP
        # calls of other threads neither fail nor invalidate the capture.
        dist_on = torch.distributed.is_available() and torch.distributed.is_initialized()
        cap_mode = dict(capture_error_mode="thread_local") if dist_on else {}
        if split:
            # The warm-up iterations issued collectives: a barrier orders every rank behind its peers' warm-up collectives and the
            # device synchronise retires them, so none is in flight when the capture starts.  Only on the all-ranks data-parallel
            # path: a step without an active hook (after dp.detach, a rank-local evaluation step) must not meet its peers here.
            torch.distributed.barrier()
            torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        self._graph2 = None
        if not split:
            with torch.cuda.graph(graph, **cap_mode):
                self._record_inputs(static)
                outs = self._iteration(*static, set_to_none=True)
        else:
            # data parallel: forward + backward (+ the buckets packed) | eager all-reduces | bucket unpack + optimizer steps
            # overlapped (dp.BucketedGradAllReduce): the hooks pack each bucket and publish its flag where the captured backward
            # completes it; reduce() then starts bucket i's all-reduce beside the rest of the replayed backward.  Phased
            # (dp.GradAndDAllReduce): every bucket is packed behind the backward.
            overlapped = hasattr(hook, "capture_begin")
            with torch.cuda.graph(graph, **cap_mode):
                self._record_inputs(static)
                if overlapped:
                    hook.capture_begin()
                outs = self._forward_backward(*static, set_to_none=True, overlap=False)
                if overlapped:
                    hook.capture_end()
                else:
                    hook.pack()
            graph2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph2, pool=graph.pool(), **cap_mode):
                hook.unpack()
                self._optimizer_steps()
            self._graph2 = graph2
        self._graph = graph
        self._static, self._outs = static, _detached(outs)
        return self


class TrainStep(_CapturedStep):
    def __init__(self, model, lr=0.04, momentum=0.9, weight_decay=1e-4, grad_hook=None, defer_losses=True, fuse_bn=True,
                 channels_last=False, qconv=True, pack_bins=True, device_hyper=False, filter_images=True):
        """filter_images (with channels_last and qconv): the weight quantiser's launch also writes every body / transition filter's
        integer bins as pre-packed bf16 images, which the convolution kernels read in place of the fp32 filter (bit-identical
        results; csrc/conv_kernels.hip).
        device_hyper: the learning rate in device memory (alignq_amd.schedule): set_lr keeps a captured graph, and
        set_schedule lets the graph walk a MultiStepLR table by itself.
        channels_last: keep activations and conv weights in torch.channels_last memory (values, parameter names and
        state_dict are unchanged).  MIOpen's NHWC convolution kernels need no layout transposes around the weight-gradient
        igemm (2.22 vs 2.50 ms per ResNet-20 step on MI355X); the quantise / Gram / ADMM kernels are layout-agnostic and the
        BN fold has a channels-last form."""
        if channels_last:
            model = model.to(memory_format=torch.channels_last)
        self.channels_last = channels_last
        self.qconv = bool(channels_last and qconv)
        paths.apply(
            model,
            # Conv2d_Q's 3x3 body convolutions (forward + data gradient) on the matrix cores, exact products
            use_qconv=self.qconv,
            # fold BN into the site kernels where shapes allow (training, 64 < batch <= 128); no-op otherwise
            fuse_bn=bool(fuse_bn),
            # N2: relu(act_q0(bn0(.))) of every block feeds conv1 only -> it is stored as its int8 / int16 level
            # index (no fp32 copy): the site forward writes, the convolution forward / filter gradient and the site backward's
            # ReLU mask read 1-2 B per element instead of 4
            pack_bins=bool(self.qconv and fuse_bn and pack_bins))
        self.filter_images = bool(filter_images and self.qconv and torch.cuda.is_available())
        self._wgrads = DeferredWgrads(fresh_grads=True) if (self.qconv and torch.cuda.is_available()) else None
        self.model = model
        self.defer_losses = defer_losses
        self._deferred = DeferredLosses() if (defer_losses and torch.cuda.is_available()) else None
        named = list(model.named_parameters())
        self.param_t = [(n, p) for n, p in named if "alterD" not in n and "gamma" not in n]
        self.param_admm = [(n, p) for n, p in named if "alterD" in n or "gamma" in n]
        self.optimizer_t = SGD([p for _, p in self.param_t], lr=lr, momentum=momentum, weight_decay=weight_decay)
        self.optimizer_admm = ADMM_OPT([p for _, p in self.param_admm]) if self.param_admm else None
        # main.py:313-317: conv weights except the stem
        self.idx = [j for j, (n, _) in enumerate(self.param_t) if "conv" in n and "weight" in n][1:]
        self.alterD_idx = [j for j, (n, _) in enumerate(self.param_admm) if "alterD" in n]
        self.gamma_idx = [j for j, (n, _) in enumerate(self.param_admm) if "gamma" in n]
        self.convs = [c for layer in model.layers for c in (layer.conv0, layer.conv1, layer.skip_conv) if c is not None]
        self.all_convs = [m for m in model.modules() if hasattr(m, "quantize_fn")]
        self.admms = []
        if self.param_admm:
            self.admms = [model.admm0]
            for layer in model.layers:
                self.admms += [layer.admm0, layer.admm1]
                if layer.skip_conv is not None:
                    self.admms.append(layer.admm_skip)
        self._init_capture(grad_hook, device_hyper)
        self._one = None

    # -------------------------------------------------------------------------------------------
    def _forward_backward(self, x, y, set_to_none=True, overlap=False):
        model = self.model
        self.optimizer_t.zero_grad(set_to_none=set_to_none)
        if self.optimizer_admm is not None:
            self.optimizer_admm.zero_grad(set_to_none=set_to_none)
        if self.channels_last and x.dim() == 4:
            x = x.contiguous(memory_format=torch.channels_last)      # no-op for the captured static input
        prequantize_weights(self.all_convs, images=self.filter_images)     # all conv weights (and filter images) in one launch
        fused_head = self.channels_last and hasattr(model, "logit") and hasattr(model, "avgpool")
        model._features_only = fused_head
        ce = None
        try:
            if self._deferred is not None and self.admms:
                with self._deferred as d:
                    out = model(x)
                    logits = out[0] if isinstance(out, tuple) else out
                    if fused_head and d.can_fuse_head() and head_ce_supported(logits, model.logit.weight, y):
                        # both loss roots from one node: no reduction launches, head backward + site preparation together
                        logits, ce, trans_loss = d.total_with_head(logits, model.logit.weight, model.logit.bias, y)
                    else:
                        trans_loss = d.total()          # joins the side stream, one stacked sum
            else:
                out = model(x)
                if isinstance(out, tuple):
                    logits, trans_loss = out
                else:
                    logits, trans_loss = out, None
        finally:
            model._features_only = False
        if ce is not None:
            pass
        elif fused_head and head_ce_supported(logits, model.logit.weight, y):
            # `logits` still holds the pre-pool features: pool + linear + cross-entropy in one launch each way
            logits, ce = HeadCEFn.apply(logits, model.logit.weight, model.logit.bias, y)
        else:
            if fused_head:       # unsupported shape: finish the head the plain way
                feats = logits
                logits = model.logit(model.avgpool(feats).view(feats.size(0), -1))
            ce = F.cross_entropy(logits, y)
        # d(ce + trans_loss) = 1 * d(ce) + 1 * d(trans_loss): two roots with a persistent unit gradient instead of forming the
        # sum (one add and one ones_like fill fewer on the in-order chain; main.py:300-304 only needs the gradients of the sum)
        roots = [ce] if (trans_loss is None or not torch.is_tensor(trans_loss) or not trans_loss.requires_grad) \
            else [ce, trans_loss]
        if self._one is None or self._one.device != ce.device:
            self._one = torch.ones((), dtype=torch.float32, device=ce.device)
        self._backward(roots, [self._one] * len(roots), set_to_none)
        if overlap and self.grad_hook is not None:
            self.grad_hook(self)            # the eager iteration's all-reduce, between backward and the optimizer steps
        return logits, ce, trans_loss

    def _optimizer_steps(self):
        if config.args.bitW < 32 and self.admms:
            w_cdf = [c.quantize_fn.weight_cdf for c in self.convs]
            w_pdf = [c.quantize_fn.weight_pdf for c in self.convs]
            a = self.admms
            # the two steps of main.py:330-340 as roles of one launch (disjoint parameters: see optimizer.sgd_admm_step)
            sgd_admm_step(self.optimizer_t, (self.idx, w_cdf, w_pdf, config.args.lam, config.args.lam2), self.optimizer_admm,
                          (self.alterD_idx, self.gamma_idx, [m.D for m in a], [m.alterD for m in a], [m.gamma for m in a],
                           [m.mu for m in a], [m.rho for m in a]))
        else:
            # CDF-only tree (main.py:308 crashes as shipped): plain momentum SGD, no grad rewrite
            self.optimizer_t.step([], [], [], config.args.lam, config.args.lam2)

    # -------------------------------------------------------------------------------------------
    def set_lr(self, lr):
        """The reference steps a StepLR scheduler once per epoch (main.py:112,150).  Scalar hyper-parameters are baked into
        a captured graph as kernel arguments, so a captured step is re-captured (no warm-up iterations: the model is not
        touched) whenever the learning rate changes.  With device_hyper the rate is staged into the device row the optimizer
        kernel reads (one 16-byte copy, none if unchanged) and the graph stays."""
        if self._hyper is not None:
            self._host_stages("set_lr")
            for g in self.optimizer_t.param_groups:
                g["lr"] = lr
            self._hyper.set(lr=lr)
            return self
        changed = False
        for g in self.optimizer_t.param_groups:
            changed |= g["lr"] != lr
            g["lr"] = lr
        if changed and self._graph is not None:
            self.capture(*self._static, warmup=0)
        return self

    def capture(self, x, y, warmup=3):
        """Capture the iteration into HIP graphs.  Runs `warmup` eager iterations first (they DO update
        the model, as real steps) so allocator pools, momentum buffers, pointer tables and MIOpen plans
        exist.  Without an active grad_hook the whole iteration is ONE graph; with one (data parallel) it is two
        graphs (forward+backward | optimizer steps) with the all-reduce launched eagerly in between."""
        # refusals first: nothing below may touch the model before them (the warm-up iterations are real steps)
        if getattr(self, "_global_corr_undo", None) is not None or getattr(config.args, "global_corr", None) is not None:
            # The exact-global correlation issues all_to_all / all_reduce from INSIDE the forward and, through
            # dp._FeatureShard.backward, from inside the ONE autograd.backward call of the step: the capture region cannot be cut at
            # them (the phased form of the gradient bucket cuts BETWEEN backward and optimizer).  Capturing the collectives
            # themselves is only defined for a process group whose asynchronous error handling (its watchdog's event polling) was
            # switched off BEFORE init_process_group (TORCH_NCCL_ASYNC_ERROR_HANDLING=0, torch's own rule for whole-network
            # capture with collectives): a property of the process this library cannot change for an existing group - with it on,
            # the round-4 capture never returned.  The mode therefore runs eagerly, by design.
            raise RuntimeError("TrainStep.capture: the exact-global correlation (global_corr) is eager-only: its collectives sit "
                               "inside the forward and inside autograd's backward call, where the capture cannot be split, and "
                               "captured collectives need a process group created with TORCH_NCCL_ASYNC_ERROR_HANDLING=0 "
                               "(DESIGN.md section 6) - call the step eagerly")
        return self._capture((x, y), warmup)


class OfficeTrainStep(_CapturedStep):
    """One DANN iteration of the Office tree (cdf_alignment_admm/dann_office/main.py:343-456): zero_grad x2 -> source pass
    -> target pass -> src class CE + src/tgt domain CE + both trans losses -> backward -> SGD.step(idx, w_cdf, w_pdf, lam,
    lam2) over the three parameter groups (feature incl. alterD/gamma, class head, domain head: main.py:324-328) ->
    ADMM_OPT.step.  Each ADMM.D holds the TARGET pass's D when ADMM_OPT runs (admm.py:25 overwrites) and alterD/gamma are
    SGD-stepped first and then overwritten by the closed form, exactly like the reference."""

    def __init__(self, model, lr=0.04, momentum=0.9, weight_decay=5e-4, alpha=0.5, channels_last=False, fuse_relu=True,
                 grad_hook=None, fuse_bn=True, dual=None, qconv=True, pack_bins=True, device_hyper=False):
        """device_hyper: the three group rates, alpha and the "new SGD" flag in device memory (alignq_amd.schedule): new_epoch
        and a per-iteration alpha (dann_office/main.py:346-348) keep one captured graph.
        grad_hook: the data-parallel all-reduce (alignq_amd.dp.attach_office -> BucketedGradAllReduce): begin() right
        before backward, its buckets' collectives start from autograd hooks while the backward runs, finish() before the
        optimizer steps.
        channels_last: activations and conv weights in torch.channels_last memory (values / names unchanged): MIOpen's NHWC
        kernels run the ResNet-50 step in 30.9 instead of 34.7 ms on MI355X; the quantise / Gram kernels are layout-agnostic.
        fuse_relu: `relu(act_q(.))` of the stem and of each bottleneck's first two sites as one launch each way.
        fuse_bn (channels_last only): additionally the training-mode batch-norm in front of those quantisers is folded into
        them (fused.bn_act_relu: statistics + one elementwise pass; SURVEY.md 8f-N1 on configuration 5).
        dual (default: on with fuse_bn and channels_last): the source and the target pass as ONE traversal (DANN.forward_dual):
        the per-sample convolutions see both batches at once, batch statistics / sites / correlations stay per domain in pass
        order; every parameter then has one incoming gradient (no accumulation kernels) and the weights are quantised once."""
        if channels_last:
            model = model.to(memory_format=torch.channels_last)
        self.channels_last = channels_last
        # qconv (channels_last only): Conv2d_Q's 1x1 / 3x3 convolutions on alignq_qconv_* (exact-product GEMMs on the bf16 / f16
        # matrix cores, csrc/qgemm_kernels.hip) instead of MIOpen's fp32 kernels (the 7x7 stem included: alignq_qconv_stem7_*).  Their filter
        # gradients leave split-K slabs that one reduction launch per 32 filters finishes (fused.DeferredWgrads).
        self.qconv = bool(qconv and channels_last and torch.cuda.is_available())
        paths.apply(
            model,
            use_qconv=self.qconv,
            # every Conv2d_Q of this network is followed by a batch-norm; folded (fuse_bn) it reads the convolution's
            # per-tile statistics instead of making a pass of its own over the output
            emit_bn_stats=bool(self.qconv and fuse_bn and fuse_relu),
            # pack_bins (N2; with qconv and fuse_bn): relu(act_q1(bn1(.))) and relu(act_q2(bn2(.))) of every bottleneck
            # feed conv2 / conv3 only - they are stored as int16 level indices (no fp32 copy): the quantiser writes, the
            # convolution's forward and filter gradient read 2 B per element instead of 4
            pack_bins=bool(pack_bins and self.qconv and fuse_bn and fuse_relu),
            fuse_relu=bool(fuse_relu),
            fuse_bn=bool(fuse_bn and fuse_relu and channels_last))
        self._wgrads = DeferredWgrads() if self.qconv else None
        self.dual = bool(fuse_bn and fuse_relu and channels_last) if dual is None else bool(dual)
        self.model, self.alpha = model, alpha
        named = list(model.named_parameters())
        self.param_admm = [(n, p) for n, p in named if "alterD" in n or "gamma" in n]
        self.optimizer_t = SGD(self._param_groups(lr), lr=lr / 10, momentum=momentum, weight_decay=weight_decay)
        self.optimizer_admm = ADMM_OPT([p for _, p in self.param_admm])
        # main.py:405-410 (param_t there lists ALL named parameters, so j indexes feature.parameters())
        self.idx = [j for j, (n, _) in enumerate(named) if ("conv" in n or "downsample.0" in n) and "weight" in n][1:]
        self.alterD_idx = [j for j, (n, _) in enumerate(self.param_admm) if "alterD" in n]
        self.gamma_idx = [j for j, (n, _) in enumerate(self.param_admm) if "gamma" in n]
        f = self._backbone()
        self.blocks = [b for layer in (f.layer1, f.layer2, f.layer3, f.layer4) for b in layer]
        self.admms = [b.admm0 for b in self.blocks]
        self.convs = []
        for b in self.blocks:
            for k, conv in enumerate((b.conv1, b.conv2, b.conv3, b.downsample)):
                if conv is not None:
                    self.convs.append(conv[0] if k == 3 else conv)
        self.all_convs = [m for m in model.modules() if hasattr(m, "quantize_fn")]
        self._staged = False
        # the domain labels (main.py:360-361 builds them every iteration) are constants of the batch sizes: kept per
        # (source batch, target batch, device), so the ones a captured graph reads outlive an off-shape eager iteration
        self._dom_labels = {}
        self._init_capture(grad_hook, device_hyper, **self._hyper_slots())

    def _hyper_slots(self):
        """What the row holds besides the rates when the step is built."""
        return dict(alpha=self.alpha)

    def _alpha(self):
        """ReverseLayerF's factor: the number, or (device_hyper) the row's slot, which the backward multiplies by as a tensor."""
        return self.alpha if self._hyper is None else self._hyper.alpha

    def __call__(self, xs, ys, xt, alpha=None):
        """alpha: the gradient-reversal coefficient of this iteration (train_step.dann_alpha; None: the value in force, at first
        the constructor's).  A captured graph can only follow it through the device row."""
        if alpha is not None:
            if self._hyper is not None:
                self._host_stages("__call__(alpha=...)")
                self._hyper.set(alpha=alpha)
            elif self._graph is not None:
                raise RuntimeError(f"{type(self).__name__}: the captured graph holds alpha as a constant; build the step with "
                                   "device_hyper=True to change it per iteration")
            self.alpha = alpha
        return super().__call__(xs, ys, xt)

    def set_producer(self, pair):
        """Attach alignq_amd.data.PairLoader (None detaches): the next `capture` records `pair.record(xs, ys, xt)` - the source
        batch's launch and the target batch's, each moving its loader's cursor on - in front of the iteration, and `next()`
        replays when both coming batches have the captured sizes (otherwise: filled eagerly, the eager fallback).  Without a
        producer every graph is node for node what it was.  An existing capture is dropped."""
        if pair is not None and not (hasattr(pair, "record") and hasattr(pair, "next_batch_sizes")):
            raise TypeError("set_producer: the Office steps expect a data.PairLoader (a source and a target DeviceLoader)")
        return super().set_producer(pair)

    def _coming_rows(self, producer):
        return tuple(producer.next_batch_sizes())

    def _captured_rows(self):
        return (self._static[0].shape[0], self._static[2].shape[0])

    def _backbone(self):
        """The ResNet feature extractor (DANN: `feature`)."""
        return self.model.feature

    def _param_groups(self, rate):
        """main.py:324-328: the feature extractor at the optimizer's default learning rate (rate / 10), the heads at `rate`."""
        m = self.model
        return [{"params": list(m.feature.parameters())},
                {"params": list(m.class_classifier.parameters()), "lr": rate},
                {"params": list(m.domain_classifier.parameters()), "lr": rate}]

    def stage_weights(self, on=True):
        """Quantise the conv weights per ResNet stage, each stage right before its forward (ResNet.forward calls back), instead of
        all of them before the first layer.  Same per-tensor arithmetic (the multi-tensor kernels treat every filter alone), 5 x 2
        launches each way instead of 2.  For data parallelism: a stage's weight gradients then leave the weight quantiser's
        backward when the backward passes that stage, so their buckets' all-reduces overlap the earlier stages' backward
        (dp.attach_office switches it on)."""
        f = self._backbone()
        if on:
            layers = (f.layer1, f.layer2, f.layer3, f.layer4)
            owner = {id(m): i + 1 for i, layer in enumerate(layers) for m in layer.modules() if hasattr(m, "quantize_fn")}
            stages = [[c for c in self.all_convs if owner.get(id(c), 0) == i] for i in range(len(layers) + 1)]
            f._wq_stage = lambda i: prequantize_weights(stages[i], pack=self.qconv)
        else:
            f._wq_stage = None
        self._staged = bool(on)
        return self

    def _forward_backward(self, xs, ys, xt, set_to_none=True, overlap=False):
        """The prologue DANN and DSAN share (zero_grad x2, both batches in the step's memory format, the conv weights
        quantised), then the tree's own forward and loss (`_forward_loss`) and the backward."""
        self.optimizer_t.zero_grad(set_to_none=set_to_none)
        self.optimizer_admm.zero_grad(set_to_none=set_to_none)
        if self.channels_last:
            xs = xs.contiguous(memory_format=torch.channels_last)
            xt = xt.contiguous(memory_format=torch.channels_last)
        labels = self._domain_labels(xs, xt)
        if not self._staged:               # (staged: ResNet.forward quantises each stage's weights right before the stage)
            prequantize_weights(self.all_convs, pack=self.qconv)
        outs = self._forward_loss(xs, ys, xt, labels)
        hook = self.grad_hook if overlap else None
        if hook is not None:
            hook.begin()              # the buckets' all-reduces start from autograd hooks during this backward
        # (the weight quantiser's backward finishes the slab reductions before it reads them)
        self._backward([outs[1]], set_to_none=set_to_none)
        if hook is not None:
            hook.finish()
        return outs

    def _domain_labels(self, xs, xt):
        """The source / target domain labels (main.py:360-361), created before the weight quantisation: moving their
        allocation changes where the allocator places the iteration's other buffers, which measurably changes the step time."""
        key = (int(xs.shape[0]), int(xt.shape[0]), xs.device)
        if key not in self._dom_labels:
            self._dom_labels[key] = (torch.zeros(xs.shape[0], dtype=torch.long, device=xs.device),
                                     torch.ones(xt.shape[0], dtype=torch.long, device=xs.device))
        return self._dom_labels[key]

    def _forward_loss(self, xs, ys, xt, labels):
        """(class logits, loss, trans loss) of the DANN iteration."""
        m = self.model
        label_src, label_tgt = labels
        if self.dual and xs.shape == xt.shape:
            cls_s, dom_s, dom_t, tl_both = m.forward_dual(xs, xt, alpha=self._alpha())      # (same weights, hence the same W_q,
            tl_s, tl_t = tl_both, 0.0                                                    #  in both of the reference's passes)
        else:
            cls_s, dom_s, tl_s = m(xs, alpha=self._alpha())
            if not self._staged:
                prequantize_weights(self.all_convs, pack=self.qconv)      # the reference quantises every weight once per pass
            _, dom_t, tl_t = m(xt, alpha=self._alpha())
        # (a pass without a loss tensor contributes the NUMBER 0: adding it would be an elementwise launch of its own)
        tl = tl_s if not torch.is_tensor(tl_t) and tl_t == 0 else (tl_t if not torch.is_tensor(tl_s) and tl_s == 0 else tl_s + tl_t)
        loss = F.cross_entropy(cls_s, ys) + F.cross_entropy(dom_s, label_src) + F.cross_entropy(dom_t, label_tgt) + tl
        return cls_s, loss, tl

    def _optimizer_steps(self):
        w_cdf = [c.quantize_fn.weight_cdf for c in self.convs]
        w_pdf = [c.quantize_fn.weight_pdf for c in self.convs]
        self.optimizer_t.step(self.idx, w_cdf, w_pdf, config.args.lam, config.args.lam2)
        a = self.admms
        self.optimizer_admm.step(self.alterD_idx, self.gamma_idx, [q.D for q in a], [q.alterD for q in a],
                                 [q.gamma for q in a], [q.mu for q in a], [q.rho for q in a])

    def new_epoch(self, epoch, num_epochs, lr, momentum=0.9, weight_decay=5e-4):
        """dann_office/main.py:321-328: every epoch the reference builds a NEW SGD (so momentum buffers start from scratch)
        with LEARNING_RATE = lr / (1 + 10 (epoch-1) / num_epochs)^0.75 for the two heads and a tenth of it for the feature
        extractor.  A captured step is re-captured (graph kernel arguments hold the learning rates).
        With device_hyper the optimizer object and the graph stay: the group rates and fresh = 1 are staged into the device row,
        and the next iteration - of whatever kind - starts every momentum buffer from its gradient, as a new SGD does."""
        rate = office_rate(lr, epoch, num_epochs)
        if self._hyper is not None:
            rates = []
            for g, spec in zip(self.optimizer_t.param_groups, self._param_groups(rate)):
                if g["momentum"] != momentum or g["weight_decay"] != weight_decay:
                    raise NotImplementedError("new_epoch(device_hyper): momentum and weight decay are arguments of the captured kernels")
                g["lr"] = spec.get("lr", rate / 10)
                rates.append(g["lr"])
            if self._schedule is None:          # (a table's rows carry the epoch's rates and fresh = 1 themselves)
                self._hyper.set(lr=rates, fresh=1)
                self._fresh_pending = True
            return rate
        self.optimizer_t = SGD(self._param_groups(rate), lr=rate / 10, momentum=momentum, weight_decay=weight_decay)
        if self._graph is not None:
            # the first step of the epoch creates the fresh momentum buffers (buf = grad) and must not be the captured one
            self._graph, self._recapture = None, True
        return rate

    def capture(self, xs, ys, xt, warmup=2):
        """Capture the iteration into HIP graphs after `warmup` eager iterations (TrainStep.capture)."""
        return self._capture((xs, ys, xt), warmup)


def dann_alpha(num_iters, num_epochs, num_iterations):
    """cdf_alignment_admm/dann_office/main.py:345-348: the gradient-reversal coefficient of global iteration `num_iters` (=
    num_iterations * epoch + i, i counting from 1) of a run of `num_epochs` epochs with `num_iterations` iterations each."""
    return ramp(num_iters, num_epochs, num_iterations)


def dsan_lambd(num_iters, num_epochs, num_iterations):
    """cdf_alignment_admm/dsan_office/main.py:381-382: the LMMD ramp for global iteration `num_iters` (= num_iterations *
    epoch + i) of a run of `num_epochs` epochs with `num_iterations` iterations each."""
    return ramp(num_iters, num_epochs, num_iterations)


class DSANTrainStep(OfficeTrainStep):
    """One DSAN iteration of the Office tree (cdf_alignment_admm/dsan_office/main.py:386-478): zero_grad x2 -> DSAN forward
    (source pass, target pass, LMMD over the bottlenecked features: resnet_office.DSAN) -> CE(s_pred, y_s) + param * lambd *
    loss_mmd -> backward -> SGD.step(idx, w_cdf, w_pdf, lam, lam2) over feature_layers (lr / 10), bottle and cls_fc (lr) ->
    ADMM_OPT.step with each ADMM.D holding the target pass's D.  new_epoch re-creates the SGD as main.py:316-329 does.
    `param * lambd` lives in a device scalar that __call__ fills before the step runs, so one captured graph serves every
    iteration of the ramp.  Not covered: data parallelism, src_only_flag."""

    def __init__(self, model, lr=0.04, momentum=0.9, weight_decay=5e-4, channels_last=False, fuse_relu=True, fuse_bn=True,
                 dual=None, qconv=True, pack_bins=True, device_hyper=False):
        super().__init__(model, lr=lr, momentum=momentum, weight_decay=weight_decay, channels_last=channels_last,
                         fuse_relu=fuse_relu, fuse_bn=fuse_bn, dual=dual, qconv=qconv, pack_bins=pack_bins,
                         device_hyper=device_hyper)
        dev = next(self.model.parameters()).device
        # args.param * lambd of the coming iteration (device_hyper: the row's `coef` slot)
        self._coef = torch.zeros(1, dtype=torch.float32, device=dev) if self._hyper is None else self._hyper.coef

    def _hyper_slots(self):
        return dict(coef=0.0)

    def _backbone(self):
        return self.model.feature_layers

    def _param_groups(self, rate):
        """main.py:318-322"""
        m = self.model
        heads = ([{"params": list(m.bottle.parameters()), "lr": rate}] if m.bottle_neck else []) + \
            [{"params": list(m.cls_fc.parameters()), "lr": rate}]
        return [{"params": list(m.feature_layers.parameters())}] + heads

    def set_lambd(self, lambd):
        """Stage args.param * lambd (main.py:407, formed in Python floats as there) for the next iteration: one fill, no sync."""
        if self._hyper is not None:
            self._host_stages("set_lambd")
            self._hyper.set(coef=float(config.args.param * lambd))
        else:
            self._coef.fill_(float(config.args.param * lambd))

    def _domain_labels(self, xs, xt):
        return None                        # (no domain classifier)

    def _forward_loss(self, xs, ys, xt, labels):
        """(source logits, loss, LMMD loss) of the DSAN iteration."""
        m = self.model
        if self.dual and xs.shape == xt.shape:
            s_pred, loss_mmd = m.forward_dual(xs, xt, ys)
        else:
            # (the target pass quantises the weights itself: the parked ones are taken by the source pass)
            s_pred, loss_mmd = m(xs, xt, ys)
        return s_pred, F.cross_entropy(s_pred, ys) + self._coef * loss_mmd, loss_mmd

    def __call__(self, xs, ys, xt, lambd=None):
        """(s_pred, loss, loss_mmd) of the iteration; lambd: dsan_lambd(...) of this iteration.  It may only be left out when a
        schedule table supplies args.param * lambd (set_schedule)."""
        if lambd is None:
            if self._schedule is None:
                raise TypeError("DSANTrainStep.__call__: lambd is required (only a schedule table, set_schedule, replaces it)")
        else:
            self.set_lambd(lambd)
        return super().__call__(xs, ys, xt)

    def capture(self, xs, ys, xt, warmup=2, lambd=None):
        """OfficeTrainStep.capture; the warm-up iterations use `lambd` if given, else the last staged value."""
        if lambd is not None:
            self.set_lambd(lambd)
        return super().capture(xs, ys, xt, warmup=warmup)
