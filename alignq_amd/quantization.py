"""Host-side mirror of the reference's model/quantization.py for the three source trees.

`make_namespace(tree)` builds the module-level names the reference exports
(`uniform_quantize`, `cdf`, `weight_quantize_fn`, `activation_quantize_fn[2]`, `corr`, `conv2d_Q_fn`)
with the signatures and return arities of that tree:

  tree="admm"   cdf_alignment_admm/resnet-{20,56}-cifar-10/model/quantization.py:19-156
  tree="cdf"    cdf_alignment/*/model/quantization.py:15-122
  tree="office" cdf_alignment_admm/{dann,dsan}_office/model/quantization.py:20-181

Importable drop-ins: alignq_amd.cdf_alignment_admm, alignq_amd.cdf_alignment, alignq_amd.office.
All arithmetic runs in hand-written HIP kernels (alignq_amd/csrc) through ops.py; there is no eager
fallback.  Options the reference reads from its global `args` come from alignq_amd.config.args.
"""
from __future__ import annotations

import types
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import config, fused, ops

_FORMULA = {"admm": L.FORMULA_ADMM, "office": L.FORMULA_ADMM, "cdf": L.FORMULA_CDF}
_EPS = {"admm": 0.0, "office": 1e-5, "cdf": 0.0}


def uniform_quantize(k):
    """model/quantization.py:19-38 — returns a callable Tensor -> Tensor (round forward, STE backward)."""
    def apply(x):
        return ops.UniformQuantizeFn.apply(x, k)
    return apply


def make_namespace(tree: str) -> types.SimpleNamespace:
    formula, eps = _FORMULA[tree], _EPS[tree]

    class cdf(nn.Module):
        """cdf(m, s, quant_src).forward(tensor) -> (cdf, pdf)  (ADMM tree :41-59; CDF tree :37-50).  Values from the HIP weight
        kernel with the given (m, s); gradients of BOTH outputs w.r.t. `tensor` and - when they are tensors of the autograd graph,
        as in the reference's own use cdf(torch.mean(x), torch.std(x), 'w') (:78) - w.r.t. m and s (ops.CdfFn)."""

        def __init__(self, m, s, quant_src):
            super().__init__()
            self.m, self.s, self.quant_src = m, s, quant_src

        def forward(self, tensor):
            x = L.dev_f32(tensor, "tensor")
            m = torch.as_tensor(self.m, dtype=torch.float32, device=x.device).reshape(())
            s_ = torch.as_tensor(self.s, dtype=torch.float32, device=x.device).reshape(())
            kc = 1.0 if tree == "cdf" else (2.0 * config.args.act_range if self.quant_src == "a" else 2.0)
            scale = config.args.act_range if (tree != "cdf" and self.quant_src == "a") else 1.0
            return ops.CdfFn.apply(x, m, s_, formula, float(kc), float(scale))

    class weight_quantize_fn(nn.Module):
        parks_filters = True     # park() takes a fused.QuantizedFilter: EvalStep and export handle only such quantisers' filters

        def __init__(self, w_bit, stage):
            super().__init__()
            self.w_bit = w_bit
            self.stage = stage
            self.uniform_q = uniform_quantize(k=w_bit)
            self._formula = formula
            self._parked = None     # the QuantizedFilter waiting for the next forward
            self._keep = False
            self._served = None     # (weak reference to the q the last forward returned, its bins, its image)

        def park(self, record, keep=False):
            """Leave a fused.QuantizedFilter for the next forward: called with `record.weight` itself it returns `record.q` and launches
            nothing.  That forward consumes the record unless `keep` (EvalStep: the filters do not change over an evaluation), which
            serves every forward until unpark()."""
            self._parked, self._keep = record, bool(keep)

        @property
        def parked(self):
            return self._parked

        def unpark(self):
            self._parked, self._keep = None, False

        def forward(self, x):
            if self.w_bit == 32:
                if tree != "cdf":
                    self.weight_cdf = x
                    self.weight_q = x
                return x
            rec = self._parked
            if not self._keep:
                self._parked = None
            self._served = None
            if rec is not None and rec.weight is x:
                q, c, pdf = rec.q, rec.cdf, rec.pdf
                self._served = (weakref.ref(q), rec.bins, rec.image)     # (q only weakly: it carries the iteration's autograd history)
            else:
                q, c, pdf = ops.WeightQuantFn.apply(x, self.w_bit, formula)
            if tree != "cdf":   # the CDF tree keeps these as locals (quantization.py:70-72)
                # (weight_q is kept WITHOUT its autograd history: same values for every reader - main.py:326-327 reads cdf / pdf -
                # but a module attribute with history would keep each iteration's graph alive into the next: see
                # train_step.retained_graph_params)
                self.weight_cdf, self.weight_pdf, self.weight_q = c, pdf, q.detach()
            else:
                self._weight_cdf, self._weight_pdf = c, pdf
            return q

        def filter_of(self, weight_q):
            """A QuantizedFilter around `weight_q` (its `weight`, cdf and pdf are not kept) with the bins and the image a parked record
            brought along, if `weight_q` is the very tensor object the last forward returned; for any other tensor - a copy, a hook's
            replacement - a record without them: the convolution then packs the bins itself and reads the fp32 filter."""
            served = self._served
            if served is not None and served[0]() is weight_q:
                return fused.QuantizedFilter(None, weight_q, bins=served[1], image=served[2])
            return fused.QuantizedFilter(None, weight_q)

    def _plain_act(x, a_bit, stage):
        if a_bit == 32 and stage != "align":
            return x
        if a_bit == 32 and tree == "cdf":
            # returns the raw cdf (quantization.py:100-101)
            xx = L.dev_f32(x, "activation")
            ms = torch.tensor([0.0, 1.0], dtype=torch.float32, device=xx.device)
            _, c, pdf, _ = ops.weight_quant_given_stats(xx.detach(), ms, 32, L.FORMULA_CDF, True)
            return _AttachGrad.apply(x, c, pdf * 0.5) if x.requires_grad else c
        return ops.ActQuantFn.apply(x, a_bit, config.args.act_range, formula)

    def _plain_act_relu(x, a_bit, stage):
        """relu(_plain_act(x)); one launch each way when the quantiser is active."""
        if (a_bit == 32) or not (x.is_cuda and x.dtype == torch.float32 and x.numel() % 4 == 0):
            return torch.relu(_plain_act(x, a_bit, stage))
        if config.args.pack_bins and ops.bin_dtype(a_bit, config.args.act_range, formula) is not None:
            # N2: the node keeps the 1-2 B level index instead of fp32 relu(x_q) (no narrow form: 16 < k < 32 or a large
            # act_range -> the fp32 path below, like the reference)
            return ops.ActQuantPackedFn.apply(x, a_bit, config.args.act_range, formula, True)[0]
        return ops.ActQuantReluFn.apply(x, a_bit, config.args.act_range, formula)

    def _site_act(mod, x):
        a_bit = mod.a_bit
        if a_bit == 32 and mod.stage != "align":
            return x, 0
        gc = getattr(mod, "global_corr", None)        # set per model by dp.attach(..., global_corr=True)
        if gc is None:
            gc = getattr(config.args, "global_corr", None)       # process-wide switch (tests)
        if config.args.method == "ours" and a_bit < 32 and gc is not None:
            # opt-in exact-global-batch correlation (dp.attach(..., global_corr=True)): D is the
            # [B_g, B_g] matrix of the concatenated batch, identical on every rank.  ADMM tree (round 4): x is exchanged ONCE, the
            # feature shard re-forms the transform and leaves D_r from the pair kernels (dp.global_site_D); the CDF-only formula
            # keeps the two-correlation composition
            from . import dp
            grp = None if gc is True else gc
            admm = mod.opt
            r_ = config.args.act_range
            xq = ops.ActQuantFn.apply(x, a_bit, r_, formula)
            if formula == L.FORMULA_ADMM and x.is_cuda:
                D = dp.global_site_D(x, a_bit, r_, eps, grp)
            else:
                t = ops.ActQuantFn.apply(x, 32, r_, formula)        # k == 32 writes the pre-round transform itself
                D = dp.global_corr(t, eps, grp) - dp.global_corr(x, eps, grp)
            return xq, admm(D)
        if config.args.method == "ours" and a_bit < 32 and x.shape[0] > L.MAX_BATCH:
            # above the 128 rows the fused kernels hold on chip: the site composed from the blocked correlation
            admm = mod.opt
            xq, loss, D = ops.site_unfused(x, admm, a_bit, config.args.act_range, eps, formula)
            admm.D = D
            return xq, loss
        if config.args.method == "ours" and a_bit < 32:
            admm = mod.opt
            from . import fused
            deferred = fused.active_deferred()
            if deferred is not None:
                bufs = None
                if deferred.side is not None:        # persistent buffers only matter for side-stream launches
                    if not hasattr(mod, "_site_bufs"):
                        mod._site_bufs = {}
                    bufs = mod._site_bufs
                rec = deferred.new_record(x.shape[0], x.device)
                xq, loss, D = ops.SiteFn.apply(x, admm.alterD, admm.gamma, a_bit, config.args.act_range, eps,
                                               admm.mu, admm.rho, deferred.side, bufs, rec)
                admm.D = D
                (deferred.add_record_loss if rec is not None else deferred.add)(loss)
                return xq, 0.0          # the real loss is summed once by DeferredLosses.total()
            xq, loss, D = ops.SiteFn.apply(x, admm.alterD, admm.gamma, a_bit, config.args.act_range, eps,
                                           admm.mu, admm.rho)
            admm.D = D
            return xq, loss
        return _plain_act(x, a_bit, mod.stage), 0

    def _site_act_res_relu(mod, x, residual):
        """(relu(act(x)[0] + residual), loss): the Office bottleneck's tail.  One launch each way on the small-batch site
        kernels when they apply (and no deferred-loss context is active), else exactly the composition."""
        from . import fused
        if (config.args.method == "ours" and mod.a_bit < 32 and fused.active_deferred() is None
                and ops.site_res_supported(x, residual)):
            admm = mod.opt
            y, loss, D = ops.SiteFn.apply(x, admm.alterD, admm.gamma, mod.a_bit, config.args.act_range, eps, admm.mu,
                                          admm.rho, None, None, None, residual, True)
            admm.D = D
            return y, loss
        out, loss = _site_act(mod, x)
        out = out + residual
        return torch.relu(out), loss

    class _act_plain(nn.Module):
        def __init__(self, a_bit, stage):
            super().__init__()
            self.a_bit, self.stage = a_bit, stage
            self.uniform_q = uniform_quantize(k=a_bit)
            self._formula = formula      # (read by the folded evaluation sites: fused.site_eval_any)

        def forward(self, x):
            return _plain_act(x, self.a_bit, self.stage)

        def forward_relu(self, x):
            """relu(self(x)) in one launch each way (not part of the reference's interface: an opt-in for the caller)."""
            return _plain_act_relu(x, self.a_bit, self.stage)

        def forward_bn_relu(self, bn, z, groups=1, pack=False):
            """relu(self(bn(z))) with the training-mode batch-norm folded into the quantiser (SURVEY.md §8f-N1 on the Office
            path; not part of the reference's interface: an opt-in for the caller, alignq_amd.fused.bn_act_relu).  groups:
            z holds that many batch slices which the reference sends through the module one after the other."""
            from . import fused
            return fused.bn_act_relu(bn, self, z, formula, relu=True, groups=groups, pack=pack)

        def forward_packed(self, x, relu=False):
            """([relu](self(x)), bins): the quantised activation both as fp32 and as its narrow integer level index
            (ops.dequant_bins(bins, ...) reproduces the fp32 tensor bit for bit)."""
            return ops.ActQuantPackedFn.apply(x, self.a_bit, config.args.act_range, formula, relu)

    class _act_admm(nn.Module):
        def __init__(self, a_bit, stage, admm):
            super().__init__()
            self.a_bit, self.stage = a_bit, stage
            self.uniform_q = uniform_quantize(k=a_bit)
            self.opt = admm

        def forward(self, x):
            return _site_act(self, x)

        def forward_res_relu(self, x, residual):
            """(relu(self(x)[0] + residual), loss) (not part of the reference's interface: an opt-in for the caller)."""
            return _site_act_res_relu(self, x, residual)

        def forward_bn_res_relu(self, bn, z, residual, groups=1, loss_vec=False):
            """(relu(self(bn(z))[0] + residual), loss) with the training-mode batch-norm folded into the small-batch site
            kernels where that applies (SURVEY.md §8f-N1 on the Office path), else the composition.  groups > 1: the batch
            slices go through one after the other (loss = their sum, ADMM.D = the last slice's, like successive passes)."""
            from . import fused
            out = fused.bn_site_res_relu(bn, self, z, residual, eps, groups, loss_vec)      # (loss_vec: see there)
            if out is not None:
                return out
            if groups == 1:
                return _site_act_res_relu(self, bn(z), residual)
            Bg = z.shape[0] // groups
            outs, loss = [], 0.
            for i in range(groups):
                o, l_ = _site_act_res_relu(self, bn(z[i * Bg:(i + 1) * Bg]), residual[i * Bg:(i + 1) * Bg])
                outs.append(o)
                loss = loss + l_
            return torch.cat(outs, 0), loss

    def corr(x, y):
        """corr(x, y) -> [B,B] (ADMM tree :134-137; Office :158-161).  The reference only ever calls it with y is x: that
        is the SYRK served by the fused MFMA kernels; any other y takes the general exact-fp32 kernels."""
        if y is x or (y.data_ptr() == x.data_ptr() and y.shape == x.shape and y.stride() == x.stride()):
            return ops.CorrFn.apply(x, eps)
        return ops.CorrXYFn.apply(x, y, eps)

    def conv2d_Q_fn(w_bit, stage):
        class Conv2d_Q(nn.Conv2d):
            # kernel-path flags, off unless set (alignq_amd.paths; INTEGRATION.md, "Kernel-path flags")
            use_qconv = False
            use_qconv_pw = False
            emit_bn_stats = False

            def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                         bias=True):
                super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias)
                self.quantize_fn = weight_quantize_fn(w_bit=w_bit, stage=stage)

            def forward(self, input, order=None):
                return self._conv(input, self.quantize_fn(self.weight))

            def _conv(self, input, weight_q):
                out = ops.conv2d_q(self, input, weight_q)      # the family of this repository's kernels that takes it, if any
                if out is not None:
                    return out
                return F.conv2d(input, weight_q, self.bias, self.stride, self.padding, self.dilation, self.groups)

            def forward_with_shortcut(self, input):
                """(conv(input), alias of input) for a block that uses its input twice — as the identity shortcut
                (`shortcut = x`) or as the input of the shortcut convolution: when the convolution runs on this repository's
                kernels (and a gradient is needed) the alias is an output of the same autograd node, so the second gradient
                is added inside the data-gradient kernel; otherwise plainly (forward(input), input)."""
                weight_q = self.quantize_fn(self.weight)
                out = ops.conv2d_q(self, input, weight_q, tap=True)
                if out is not None:
                    return out
                return self._conv(input, weight_q), input

        return Conv2d_Q

    ns = types.SimpleNamespace(uniform_quantize=uniform_quantize, cdf=cdf, weight_quantize_fn=weight_quantize_fn,
                               conv2d_Q_fn=conv2d_Q_fn)
    if tree == "cdf":
        _act_plain.__name__ = _act_plain.__qualname__ = "activation_quantize_fn"
        ns.activation_quantize_fn = _act_plain
    elif tree == "admm":
        _act_admm.__name__ = _act_admm.__qualname__ = "activation_quantize_fn"
        ns.activation_quantize_fn = _act_admm
        ns.corr = corr
    else:
        _act_plain.__name__ = _act_plain.__qualname__ = "activation_quantize_fn"
        _act_admm.__name__ = _act_admm.__qualname__ = "activation_quantize_fn2"
        ns.activation_quantize_fn = _act_plain
        ns.activation_quantize_fn2 = _act_admm
        ns.corr = corr
    return ns


def make_uniform_admm_namespace() -> types.SimpleNamespace:
    """The paper's `use_cdf=False` ablation: cdf_alignment_admm/resnet-20-cifar-10/model/
    quantization_uniform_admm.py — plain uniform quantisers with the ADMM loss still attached.

    weight_quantize_fn.forward (:61-85): W_q = uniform_quantize(k)(W) (no CDF; only `.weight_q` is stored, plus
    `.weight_cdf = x` for w_bit == 32).  activation_quantize_fn.forward (:88-139): x_q = uniform_quantize(k)(x) and, with
    args.method containing 'ours' and a_bit < 32, D = corr(x,x) - corr(x,x) (zero wherever the correlation is finite, NaN
    where a feature has zero batch variance, exactly like the reference) and trans_loss = admm(D).  The two corr terms are
    the same tensor, so the reference's gradient of D w.r.t. x cancels term by term; D is detached here."""
    base = make_namespace("admm")

    class weight_quantize_fn(nn.Module):
        def __init__(self, w_bit, stage):
            super().__init__()
            self.w_bit, self.stage = w_bit, stage
            self.uniform_q = uniform_quantize(k=w_bit)

        def forward(self, x):
            if self.w_bit == 32:
                self.weight_cdf = x
                self.weight_q = x
                return x
            self.weight_q = self.uniform_q(x)
            return self.weight_q

    class activation_quantize_fn(nn.Module):
        def __init__(self, a_bit, stage, admm):
            super().__init__()
            self.a_bit, self.stage = a_bit, stage
            self.uniform_q = uniform_quantize(k=a_bit)
            self.opt = admm

        def forward(self, x):
            if self.a_bit == 32 and self.stage != "align":
                return x, 0
            activation_q = self.uniform_q(x)
            if "ours" in config.args.method and self.a_bit < 32:
                G = ops.CorrFn.apply(x.detach(), 0.0)
                trans_loss = self.opt(G - G)
            else:
                trans_loss = 0
            return (x if self.a_bit == 32 else activation_q), trans_loss

    def conv2d_Q_fn(w_bit, stage):
        class Conv2d_Q(nn.Conv2d):
            def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                         bias=True):
                super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias)
                self.quantize_fn = weight_quantize_fn(w_bit=w_bit, stage=stage)

            def forward(self, input, order=None):
                weight_q = self.quantize_fn(self.weight)
                return F.conv2d(input, weight_q, self.bias, self.stride, self.padding, self.dilation, self.groups)

        return Conv2d_Q

    return types.SimpleNamespace(uniform_quantize=uniform_quantize, cdf=base.cdf, weight_quantize_fn=weight_quantize_fn,
                                 activation_quantize_fn=activation_quantize_fn, corr=base.corr, conv2d_Q_fn=conv2d_Q_fn)


class _AttachGrad(torch.autograd.Function):
    """y = value (precomputed by a kernel) with dy/dx = jac elementwise."""

    @staticmethod
    def forward(ctx, x, value, jac):
        ctx.save_for_backward(jac)
        return value.clone()

    @staticmethod
    def backward(ctx, g):
        (jac,) = ctx.saved_tensors
        return g * jac, None, None
