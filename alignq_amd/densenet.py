"""DenseNet-40 for CIFAR-10, wired like the reference's cdf_alignment/dense-cifar-10/model/densenet.py (:17-159) on the CDF-only
namespace (alignq_amd.cdf_alignment), with the SAME class names, constructor signatures and attribute names (`conv1`,
`dense{1,2,3}[i].{bn1,act_q0,conv1}`, `trans{1,2}.{bn1,act_q0,conv1}`, `bn`, `act_q0`, `fc`), so that state_dict() keys and shapes equal
the reference's and its checkpoints load by name.

What the reference does and this file keeps: a dense layer is bn1 -> act_q0 -> ReLU -> 3x3 convolution (CIN -> growthRate), its output
concatenated BEHIND its input (`torch.cat((x, out), 1)`); `F.dropout` where dropRate > 0; a transition is the same site, a 1x1
convolution and a 2x2 average pool; the head is bn -> act_q0 -> ReLU -> AvgPool2d(8) -> Linear; convolutions are initialised
N(0, 2 / (k k C_out)), batch-norms to (1, 0).  `filters` / `indexes` are the reference's arguments (the input width of every
convolution in order; `indexes` is accepted and not read, as there).  densenet_40_quant passes compressionRate=1: 24 -> 168 | 168 ->
312 | 312 -> 456 channels.

Every weight and activation quantiser runs on this repository's kernels.  With use_hip_convs(model) and channels-last inputs the 3x3
dense layers (CIN = 24, 36, ..., 444 -> 12: multiples of 4, not of 8) run on csrc/k3conv_kernels.hip (include/alignq_k3conv.h) and
the two transitions on csrc/pointwise_kernels.hip; the 3 -> 24 stem, batch-norm, the pools and the linear layer go to MIOpen /
rocBLAS through PyTorch-ROCm.  With use_hip_convs(model, stem=True) the stem runs on csrc/k3image_kernels.hip
(include/alignq_k3image.h) as well, and every Conv2d_Q of the model has arithmetic this repository defines.  The sites run as the
composition, or, with use_hip_convs(model, train_sites=True), folded in training: batch-norm, quantiser and ReLU as three launches each way
on csrc/bnq_any_kernels.hip (include/alignq_bnq_any.h) at every width.  With use_hip_convs(model, dense_train=True) a training
forward also runs every dense block as ONE autograd node on ONE buffer (fused.DenseBlockFn, csrc/dense_train_kernels.hip,
include/alignq_dense_train.h): nothing is concatenated, and neither a copy of a layer's input nor its quantised activation nor a mask is
kept for the backward; the bits are those of train_sites=True.  Training is eager iterations (alignq_amd.optimizer.SGD).

Evaluation (eval_step.EvalStep) with use_hip_convs(model, dense_eval=True): DenseNet._forward_eval keeps ONE buffer per dense block;
a dense layer is one alignq_dense_layer_eval_fwd launch (include/alignq_dense.h: the site applied while the convolution stages its
input, the 12 output channels written right behind the input), nothing is concatenated, and a transition's pool writes into the
next block's buffer.  With stem=True the stem writes into the first block's buffer itself (fused.stem_eval_into: one launch, no copy).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import cdf_alignment as _cdf
from . import fused, paths


def conv2d_Q3_fn(w_bit, stage):
    """Conv2d_Q of the CDF namespace plus two opt-in flags: with `use_qconv_k3` the 3x3 / stride 1 / padding 1 convolutions at channel
    counts that are multiples of 4 run on alignq_k3conv_*, ahead of every other family; with `use_qconv_k3_image` the one on the
    3-channel image (the stem) runs on alignq_k3image_* (ops.conv2d_q reads the flags).  They are declared HERE, not on Conv2d_Q: no
    other model's modules carry them."""
    base = _cdf.conv2d_Q_fn(w_bit=w_bit, stage=stage)

    class Conv2d_Q3(base):
        use_qconv_k3 = False          # kernel-path flag, off unless set (alignq_amd.paths; INTEGRATION.md, "Kernel-path flags")
        use_qconv_k3_image = False    # likewise

    return Conv2d_Q3


def _site(mod, bn, act, x):
    """relu(act(bn(x))).  With the module's `fuse_train_sites` on, a training forward runs it as one folded chain at any channel count
    (fused.bn_act_any: three launches each way, the normalised activation never written); where that does not apply, and always with
    the flag off, it is the composition."""
    if mod.fuse_train_sites and mod.training and not fused.eval_active():
        out = fused.bn_act_any(bn, act, x, fused.CLAMP_RELU)
        if out is not None:
            return out
    return mod.relu(act(bn(x)))


class DenseBasicBlock(nn.Module):
    fuse_train_sites = False          # kernel-path flag, off unless set (alignq_amd.paths; INTEGRATION.md, "Kernel-path flags")

    def __init__(self, stage, wbit, abit, inplanes, filters, index, expansion=1, growthRate=12, dropRate=0):
        super().__init__()
        Conv2d = conv2d_Q3_fn(w_bit=wbit, stage=stage)
        self.act_q0 = _cdf.activation_quantize_fn(a_bit=abit, stage=stage)
        self.bn1 = nn.BatchNorm2d(inplanes)
        self.conv1 = Conv2d(filters, growthRate, kernel_size=3, padding=1, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.dropRate = dropRate

    def forward(self, x):
        out = self.conv1(_site(self, self.bn1, self.act_q0, x))
        if self.dropRate > 0:
            out = F.dropout(out, p=self.dropRate, training=self.training)
        return torch.cat((x, out), 1)          # channels-last inputs give a channels-last result


class Transition(nn.Module):
    fuse_train_sites = False          # likewise

    def __init__(self, stage, wbit, abit, inplanes, outplanes, filters, index):
        super().__init__()
        Conv2d = _cdf.conv2d_Q_fn(w_bit=wbit, stage=stage)
        self.act_q0 = _cdf.activation_quantize_fn(a_bit=abit, stage=stage)
        self.bn1 = nn.BatchNorm2d(inplanes)
        self.conv1 = Conv2d(filters, outplanes, kernel_size=1, bias=False)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return F.avg_pool2d(self.conv1(_site(self, self.bn1, self.act_q0, x)), 2)


class DenseNet(nn.Module):
    fuse_dense_eval = False           # kernel-path flag, off unless set (alignq_amd.paths; INTEGRATION.md, "Kernel-path flags")
    fuse_train_sites = False          # likewise
    fuse_dense_train = False          # likewise

    def __init__(self, wbit, abit, stage, depth=40, block=DenseBasicBlock, dropRate=0, num_classes=10, growthRate=12,
                 compressionRate=2, filters=None, indexes=None):
        super().__init__()
        self.wbit, self.abit, self.stage = wbit, abit, stage
        if (depth - 4) % 3 != 0:
            raise ValueError("DenseNet: depth must be 3 n + 4")
        n = (depth - 4) // 3
        if filters is None:
            filters, start = [], 2 * growthRate
            for _ in range(3):          # per stage: the n layers' input widths, then the width its transition (or the head) takes
                filters += [start + growthRate * i for i in range(n + 1)]
                start = (start + growthRate * n) // compressionRate
            indexes = [None] * len(filters)
        self.growthRate, self.dropRate = growthRate, dropRate
        self.inplanes = 2 * growthRate
        self.conv1 = conv2d_Q3_fn(w_bit=wbit, stage=stage)(3, self.inplanes, kernel_size=3, padding=1, bias=False)
        self.dense1 = self._make_denseblock(block, n, filters[0:n], indexes[0:n])
        self.trans1 = self._make_transition(Transition, compressionRate, filters[n], indexes[n])
        self.dense2 = self._make_denseblock(block, n, filters[n + 1:2 * n + 1], indexes[n + 1:2 * n + 1])
        self.trans2 = self._make_transition(Transition, compressionRate, filters[2 * n + 1], indexes[2 * n + 1])
        self.dense3 = self._make_denseblock(block, n, filters[2 * n + 2:3 * n + 2], indexes[2 * n + 2:3 * n + 2])
        self.bn = nn.BatchNorm2d(self.inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.avgpool = nn.AvgPool2d(8)
        self.fc = nn.Linear(self.inplanes, num_classes)
        self.act_q0 = _cdf.activation_quantize_fn(a_bit=abit, stage=stage)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.data.normal_(0, math.sqrt(2.0 / (m.kernel_size[0] * m.kernel_size[1] * m.out_channels)))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    def _make_denseblock(self, block, blocks, filters, indexes):
        if not (blocks == len(filters) == len(indexes)):
            raise ValueError("DenseNet: one `filters` / `indexes` entry per dense layer")
        layers = []
        for i in range(blocks):
            layers.append(block(stage=self.stage, wbit=self.wbit, abit=self.abit, inplanes=self.inplanes, filters=filters[i],
                                index=indexes[i], growthRate=self.growthRate, dropRate=self.dropRate))
            self.inplanes += self.growthRate
        return nn.Sequential(*layers)

    def _make_transition(self, transition, compressionRate, filters, index):
        inplanes, outplanes = self.inplanes, self.inplanes // compressionRate
        self.inplanes = outplanes
        return transition(self.stage, self.wbit, self.abit, inplanes, outplanes, filters, index)

    def forward(self, x):
        if self.fuse_dense_eval and fused.eval_active():
            return self._forward_eval(x)
        x = self._dense(self.dense1, self.conv1(x))
        x = self._dense(self.dense2, self.trans1(x))
        x = self._dense(self.dense3, self.trans2(x))
        x = self.avgpool(_site(self, self.bn, self.act_q0, x))
        return self.fc(x.reshape(x.size(0), -1))

    def _dense(self, dense, x):
        """One dense block: with `fuse_dense_train` on, a training forward runs it as one node on one buffer (fused.dense_block_train);
        where that does not apply (dropout, a batch-norm without tracked statistics, another quantiser, an unsupported shape), and
        always with the flag off, it is the modules."""
        if self.fuse_dense_train and self.training and not fused.eval_active():
            out = fused.dense_block_train(dense, x)
            if out is not None:
                return out
        return dense(x)

    # ---- evaluation without concatenations (inside fused.eval_scope: eval_step.EvalStep) ----
    def _forward_eval(self, x):
        """forward() with one buffer per dense block (168 / 312 / 456 channels at depth 40): the block's input is copied into its
        first channels once (with `use_qconv_k3_image` the stem writes them itself: _stem_eval), every dense layer is one launch in place (fused.dense_layer_eval), a transition is its site on the full
        buffer (fused.site_eval_any), the 1x1 convolution and the pool into the next block's buffer (fused.avgpool2_into), the head its
        site, the pool and the linear layer.  Whatever has no kernel runs the composition of forward().  Dropout is inactive in
        evaluation."""
        x = self._dense_eval(self.dense1, *self._stem_eval(x))
        x = self._dense_eval(self.dense2, *self._transition_eval(self.trans1, x, self.dense2))
        x = self._dense_eval(self.dense3, *self._transition_eval(self.trans2, x, self.dense3))
        y = fused.site_eval_any(self.bn, self.act_q0, x, fused.CLAMP_RELU)
        if y is None:
            y = self.relu(self.act_q0(self.bn(x)))
        x = self.avgpool(y)
        return self.fc(x.reshape(x.size(0), -1))

    def _stem_eval(self, x):
        """(conv1(x), None), or (None, buf) with the stem's output in the first channels of the first block's buffer"""
        dense = self.dense1
        if (getattr(self.conv1, "use_qconv_k3_image", False) and len(dense) and not self.training and fused._nhwc_f32(x)
                and self.conv1.out_channels == dense[0].bn1.num_features):
            buf = self._block_buffer(dense, x.shape[0], x.shape[2], x.shape[3], x.device)
            if fused.stem_eval_into(self.conv1, x, buf) is not None:
                return None, buf
        return self.conv1(x), None

    @staticmethod
    def _block_buffer(dense, B, H, W, device):
        c_end = dense[0].bn1.num_features + sum(layer.conv1.out_channels for layer in dense)
        return torch.empty((B, c_end, H, W), dtype=torch.float32, device=device, memory_format=torch.channels_last)

    def _dense_eval(self, dense, x, buf):
        """One dense block.  x: its input, or None when `buf` already holds it in its first channels."""
        if len(dense) == 0 or self.training:
            return dense(x)
        cin = dense[0].bn1.num_features
        if buf is None:
            if not (fused._nhwc_f32(x) and x.shape[1] == cin):
                return dense(x)
            buf = self._block_buffer(dense, x.shape[0], x.shape[2], x.shape[3], x.device)
            buf[:, :cin].copy_(x)
        for i, layer in enumerate(dense):
            if fused.dense_layer_eval(layer.conv1, layer.bn1, layer.act_q0, buf, cin) is None:
                # the composition for the rest of the block, on the channels filled so far
                return dense[i:](buf[:, :cin].contiguous(memory_format=torch.channels_last))
            cin += layer.conv1.out_channels
        return buf

    def _transition_eval(self, trans, x, dense):
        """(x, None) = the transition's output, or (None, buf) with the output in the first channels of the next block's buffer"""
        y = fused.site_eval_any(trans.bn1, trans.act_q0, x, fused.CLAMP_RELU)
        if y is None:
            y = trans.relu(trans.act_q0(trans.bn1(x)))
        z = trans.conv1(y)
        if len(dense) and fused._nhwc_f32(z) and z.shape[1] == dense[0].bn1.num_features and z.shape[2] >= 2 and z.shape[3] >= 2:
            buf = self._block_buffer(dense, z.shape[0], z.shape[2] // 2, z.shape[3] // 2, z.device)
            if fused.avgpool2_into(z, buf) is not None:
                return None, buf
        return F.avg_pool2d(z, 2), None


def densenet_40_quant(bitW, abitW, stage, pretrained=False, **kwargs):
    return DenseNet(wbit=bitW, abit=abitW, stage=stage, depth=40, block=DenseBasicBlock, compressionRate=1, **kwargs)


def use_hip_convs(model, dense_eval=False, stem=False, train_sites=False, dense_train=False):
    """Channels-last parameters plus `use_qconv`, `use_qconv_pw` (the transitions) and `use_qconv_k3` (the dense layers): with
    channels-last inputs every dense layer then runs on alignq_k3conv_* and both transitions on alignq_pwconv_*; the concatenations keep
    the layout, so no dense layer falls back to MIOpen.  Values, parameter names and state_dict are unchanged.
    dense_eval=True also sets `fuse_dense_eval`: inside eval_step.EvalStep the model then runs DenseNet._forward_eval (one launch per
    dense layer, no concatenation); every other forward is unchanged.
    stem=True also sets `use_qconv_k3_image`: the 3 -> 24 stem then runs on alignq_k3image_*, and inside _forward_eval it writes into
    the first block's buffer by one launch.  Without it every launch is what it was.
    train_sites=True also sets `fuse_train_sites`: in training forwards every bn -> act_q0 -> ReLU site (dense layers, transitions, head)
    then runs folded on alignq_bnq_any_* (include/alignq_bnq_any.h).  Without it every launch is what it was.
    dense_train=True implies train_sites and also sets `fuse_dense_train`: in training forwards every dense block then runs as one
    fused.DenseBlockFn node on alignq_dense_train_* (include/alignq_dense_train.h), with the bits of train_sites=True.  Without it every
    launch is what it was."""
    model = model.to(memory_format=torch.channels_last)
    paths.apply(model, use_qconv=True, use_qconv_pw=True, use_qconv_k3=True)
    if stem:
        paths.apply(model, use_qconv_k3_image=True)
    if dense_eval:
        paths.apply(model, fuse_dense_eval=True)
    if train_sites or dense_train:
        paths.apply(model, fuse_train_sites=True)
    if dense_train:
        paths.apply(model, fuse_dense_train=True)
    return model
