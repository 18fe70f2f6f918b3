"""The reference's test() (cdf_alignment_admm/resnet-20-cifar-10/main.py:405-441, dann_office/main.py:502-545; accuracy:
utils/common.py:78-92) as a step of this repository: eval-mode batch-norm folded into the quantiser (alignq_bnq_eval_fwd, one
launch per site), the filters quantised once per evaluation instead of once per batch, cross-entropy / Prec@1 / Prec@5
accumulated on the device (alignq_eval_metrics, one launch per batch, ONE host read per evaluation), the per-batch work
capturable as one HIP graph.

    ev = EvalStep(model, channels_last=True, qconv=True)
    with ev:                                  # begin() ... end()
        ev.capture(x0, y0)                    # optional
        for x, y in loader:
            ev(x, y)                          # enqueues; returns the logits; no synchronisation
        ce, prec1, prec5, n = ev.result()     # the one host read

Differences from the reference's test(): an ADMM site computes no Gram matrices and no ADMM loss and
leaves ADMM.D alone (test() discards the loss, and the D it stores is overwritten by the next training forward before anything
reads it); ties are ranked as include/alignq.h states for alignq_eval_metrics.  This holds where alignq_bnq_eval_fwd applies
(channels-last fp32, C a power of two in [4, 2048], a quantiser of 1..16 bits or none): any other site runs today's `model.eval()`
composition, which at an ADMM site does form the Grams and the loss and does store ADMM.D.  mobilenet.MobileNetV2 folds its sites
itself inside the step (fused.site_eval_any / site_eval_twin / dw_site_eval, include/alignq_mobile.h: any C % 4 == 0 in [4, 2048],
ReLU6, the stride-1 block tail, the depthwise convolution with its site as the epilogue).  densenet.DenseNet with
`fuse_dense_eval` (densenet.use_hip_convs(model, dense_eval=True)) runs DenseNet._forward_eval inside the step: one buffer per dense
block, every dense layer one launch with its site inside the 3x3 convolution (fused.dense_layer_eval, include/alignq_dense.h), no
concatenation; without the flag a DenseNet runs today's composition.

    ev = EvalStep(skeleton, weights=export.PackedModel.load(path))     # evaluate from packed k-bit codes (export.py): begin()
                                                                       # unpacks them; the model's fp32 filters are never read"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import fused, paths
from .train_step import _CapturedStep


class EvalStep(_CapturedStep):
    """model: resnet.PreActResNet (tree "admm" or "cdf"), resnet_office.DANN (class logits at alpha = 0), resnet_office.DSAN
    (s_pred), mobilenet.MobileNetV2 or densenet.DenseNet.  channels_last / qconv: as TrainStep / OfficeTrainStep (the folded evaluation sites need channels-last tensors;
    without it every site is today's `model.eval()` composition).  Nothing in model.state_dict() changes between begin() and
    end(); the module flags the step sets (fuse_bn, use_qconv, ...) and every training flag are put back by end()."""

    def __init__(self, model, channels_last=True, qconv=True, pack_bins=True, filter_images=True, weights=None):
        if weights is not None and not channels_last:
            raise ValueError("EvalStep(weights=): packed filters are channels-last; channels_last=True is required")
        if channels_last:
            model = model.to(memory_format=torch.channels_last)
        self.model = model
        self.channels_last = bool(channels_last)
        self.qconv = bool(qconv and channels_last and torch.cuda.is_available())
        self.pack_bins = bool(pack_bins and self.qconv)
        # the quantiser's launch also writes the convolutions' bf16 filter images: once per evaluation, read by every batch
        self.filter_images = bool(filter_images and self.qconv)
        self.all_convs = [m for m in model.modules() if hasattr(m, "quantize_fn")]
        self._office = hasattr(model, "feature") or hasattr(model, "feature_layers")
        self._acc = None             # include/alignq.h: {double sum ce, int64 top-1, int64 top-5, int64 rows}
        self._saved = None           # module flags and training modes to restore
        self._wq = None              # the parked quantised filters (persistent: a captured graph reads them)
        self._scope = None
        # weights: an export.PackedModel - begin() forms W_q, bins and images from its codes instead of quantising model's fp32
        # filters, whose values are then never read (every quantised Conv2d_Q must match an entry: ValueError here, before any launch)
        self._packed = None
        if weights is not None:
            from .export import PackedFilters
            self._packed = PackedFilters(weights, model)
        self._init_capture(None)

    # ------------------------------------------------------------------------------------------- lifecycle
    def _pack_filters(self):
        """Whether begin() also leaves the filters' integer bins for the GEMM convolutions: the Office models, and any model whose
        Conv2d_Q carry `use_qconv_pw` (mobilenet.use_hip_convs(model, pointwise=True)) or `use_qconv_k3` (densenet.use_hip_convs: the
        dense layers' launches read the parked bins) - once per evaluation, not per batch and layer"""
        return self.qconv and (self._office or any(c.use_qconv_pw or getattr(c, "use_qconv_k3", False) for c in self.all_convs))

    def _quantize_weights(self):
        """All filters once (fused.prequantize_weights; the GEMM convolutions' integer bins too), parked for every batch.  A second
        evaluation refreshes the SAME tensors in place: a captured graph keeps reading them."""
        convs = [c for c in self.all_convs
                 if getattr(c.quantize_fn, "w_bit", 32) != 32 and getattr(c.quantize_fn, "parks_filters", False)]
        if self._packed is not None:
            # from the packed codes (alignq_weight_unpack_multi) into tensors that persist (records without cdf and pdf)
            fresh = self._packed.refresh(pack=self._pack_filters(), images=self.filter_images)
            if self._wq is None or any(id(c) not in self._wq or self._wq[id(c)].q is not fresh[id(c)].q for c in convs):
                self._graph = None
            self._wq = {id(c): fresh[id(c)] for c in convs}
        else:
            fused.prequantize_weights(convs, pack=self._pack_filters(), images=self.filter_images)
            fresh = {id(c): c.quantize_fn.parked for c in convs}
            # (in place only into records of the same make-up: the same convolutions, each with bins / an image then and now)
            if (self._wq is not None and set(self._wq) == set(fresh)
                    and all((o is None) == (n is None) for key in fresh for o, n in zip(self._wq[key], fresh[key]))):
                for key, old in self._wq.items():
                    new = fresh[key]
                    old.q.copy_(new.q)
                    old.cdf.copy_(new.cdf)
                    old.pdf.copy_(new.pdf)
                    for o, n in zip(old.bins or (), new.bins or ()):     # the (bf16, f16) pair
                        o.copy_(n)
                    if old.image is not None:
                        old.image.copy_(new.image)
            else:
                self._wq = fresh
                self._graph = None           # (tensors a captured graph read are gone)
        for c in convs:
            c.quantize_fn.park(self._wq[id(c)], keep=True)

    def begin(self):
        if self._saved is not None:
            raise RuntimeError("EvalStep.begin: already begun (call end() first)")
        # (emit_bn_stats: no batch statistics in evaluation; _wq_stage: OfficeTrainStep.stage_weights re-quantises per stage and batch)
        flags = paths.apply(self.model, use_qconv=self.qconv, emit_bn_stats=False, fuse_bn=self.channels_last, fuse_relu=True,
                            pack_bins=self.pack_bins, _wq_stage=None)
        self._saved = (flags, [(m, m.training) for m in self.model.modules()])
        try:
            self.model.eval()
            dev = next(self.model.parameters()).device
            with torch.no_grad():
                self._quantize_weights()
                if self._acc is None or self._acc.device != dev:
                    self._acc = torch.zeros(4, dtype=torch.int64, device=dev)
                    self._graph = None
                else:
                    self._acc.zero_()
        except BaseException:
            self.end()              # (a failing __enter__ gets no __exit__: leave the model as it was)
            raise
        return self

    def end(self):
        for c in self.all_convs:
            if getattr(c.quantize_fn, "parks_filters", False):
                c.quantize_fn.unpark()
        flags, modes = self._saved or ((), ())
        paths.restore(flags)
        for m, training in modes:
            m.training = training
        self._saved = None
        return self

    __enter__ = begin

    def __exit__(self, *exc):
        self.end()
        return False

    # ------------------------------------------------------------------------------------------- one batch
    def _logits(self, x):
        m = self.model
        if hasattr(m, "feature"):                      # DANN: class logits; alpha only scales the reversed gradient
            feature, _ = m.feature(x)
            return m.class_classifier(feature.view(-1, 2048))
        if hasattr(m, "feature_layers"):               # DSAN: s_pred
            feature, _ = m.feature_layers(x)
            return m.cls_fc(m._head(feature))
        out = m(x)
        return out[0] if isinstance(out, tuple) else out

    def _iteration(self, x, y, set_to_none=True):
        if self._saved is None:
            raise RuntimeError("EvalStep: call begin() first (or use the step as a context manager)")
        if self.channels_last and x.dim() == 4:
            x = x.contiguous(memory_format=torch.channels_last)
        with torch.no_grad(), fused.eval_scope():
            logits = self._logits(x)
            self._metrics(logits, y)
        return logits

    def _metrics(self, logits, y):
        lg = L.dev_f32(logits, "logits")
        if y.dtype != torch.int64 or not y.is_cuda:
            raise TypeError("EvalStep: targets must be a CUDA int64 tensor")
        y = y.contiguous()
        B, K = lg.shape
        L.check(L.load().alignq_eval_metrics(L.ptr(lg), L.ptr(y), int(B), int(K), L.ptr(self._acc), L.stream_ptr()),
                "alignq_eval_metrics")

    def _eager_fallback(self, *inputs):
        return self._iteration(*inputs)

    def __call__(self, x, y):
        if self._saved is None:      # (also in front of a replay: the graph reads this evaluation's filters and accumulator)
            raise RuntimeError("EvalStep: call begin() first (or use the step as a context manager)")
        return super().__call__(x, y)

    def next(self):
        if self._saved is None:
            raise RuntimeError("EvalStep: call begin() first (or use the step as a context manager)")
        return super().next()

    def capture(self, x, y, warmup=2):
        """Record the per-batch work (forward + metrics) as one HIP graph after `warmup` eager batches (allocator pools, MIOpen /
        rocBLAS plans; at least one), on _CapturedStep's static buffers and warm-up; the warm-up batches do not count.  Later calls
        with tensors of these shapes replay it; another batch size (a short last batch) runs eagerly."""
        if self._saved is None:
            raise RuntimeError("EvalStep.capture: call begin() first")
        static = self._static_clones((x, y))
        keep = self._acc.clone()
        self._warm_up(static, max(int(warmup), 1))
        self._acc.copy_(keep)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._record_inputs(static)
            outs = self._iteration(*static)
        self._graph, self._graph2 = graph, None
        self._static, self._outs = static, outs
        return self

    # ------------------------------------------------------------------------------------------- result
    def counts(self):
        """(sum of cross-entropy, top-1 count, top-5 count, rows) as accumulated: the evaluation's one host read"""
        raw = self._acc.cpu().numpy()
        return float(raw[:1].view(np.float64)[0]), int(raw[1]), int(raw[2]), int(raw[3])

    def result(self):
        """(mean cross-entropy, Prec@1, Prec@5, n) over the batches since begin().  Precisions in percent, like utils.accuracy."""
        ce, n1, n5, n = self.counts()
        if n == 0:
            return float("nan"), 0.0, 0.0, 0
        return ce / n, 100.0 * n1 / n, 100.0 * n5 / n, n
