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
rocBLAS through PyTorch-ROCm.  The sites run as the composition; training is eager iterations (alignq_amd.optimizer.SGD).

Evaluation (eval_step.EvalStep) with use_hip_convs(model, dense_eval=True): DenseNet._forward_eval keeps ONE buffer per dense block;
a dense layer is one alignq_dense_layer_eval_fwd launch (include/alignq_dense.h: the site applied while the convolution stages its
input, the 12 output channels written right behind the input), nothing is concatenated, and a transition's pool writes into the
next block's buffer.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import cdf_alignment as _cdf
from . import fused, paths


def conv2d_Q3_fn(w_bit, stage):
    """Conv2d_Q of the CDF namespace plus one opt-in flag: with it the 3x3 / stride 1 / padding 1 convolutions at channel counts that
    are multiples of 4 run on alignq_k3conv_*, ahead of every other family (ops.conv2d_q reads the flag).  The flag is declared HERE,
    not on Conv2d_Q: no other model's modules carry it."""
    base = _cdf.conv2d_Q_fn(w_bit=w_bit, stage=stage)

    class Conv2d_Q3(base):
        use_qconv_k3 = False          # kernel-path flag, off unless set (alignq_amd.paths; INTEGRATION.md, "Kernel-path flags")

    return Conv2d_Q3


class DenseBasicBlock(nn.Module):
    def __init__(self, stage, wbit, abit, inplanes, filters, index, expansion=1, growthRate=12, dropRate=0):
        super().__init__()
        Conv2d = conv2d_Q3_fn(w_bit=wbit, stage=stage)
        self.act_q0 = _cdf.activation_quantize_fn(a_bit=abit, stage=stage)
        self.bn1 = nn.BatchNorm2d(inplanes)
        self.conv1 = Conv2d(filters, growthRate, kernel_size=3, padding=1, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.dropRate = dropRate

    def forward(self, x):
        out = self.conv1(self.relu(self.act_q0(self.bn1(x))))
        if self.dropRate > 0:
            out = F.dropout(out, p=self.dropRate, training=self.training)
        return torch.cat((x, out), 1)          # channels-last inputs give a channels-last result


class Transition(nn.Module):
    def __init__(self, stage, wbit, abit, inplanes, outplanes, filters, index):
        super().__init__()
        Conv2d = _cdf.conv2d_Q_fn(w_bit=wbit, stage=stage)
        self.act_q0 = _cdf.activation_quantize_fn(a_bit=abit, stage=stage)
        self.bn1 = nn.BatchNorm2d(inplanes)
        self.conv1 = Conv2d(filters, outplanes, kernel_size=1, bias=False)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return F.avg_pool2d(self.conv1(self.relu(self.act_q0(self.bn1(x)))), 2)


class DenseNet(nn.Module):
    fuse_dense_eval = False           # kernel-path flag, off unless set (alignq_amd.paths; INTEGRATION.md, "Kernel-path flags")

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
        x = self.dense1(self.conv1(x))
        x = self.dense2(self.trans1(x))
        x = self.dense3(self.trans2(x))
        x = self.avgpool(self.relu(self.act_q0(self.bn(x))))
        return self.fc(x.reshape(x.size(0), -1))


    # ---- evaluation without concatenations (inside fused.eval_scope: eval_step.EvalStep) ----
    def _forward_eval(self, x):
        """forward() with one buffer per dense block (168 / 312 / 456 channels at depth 40): the block's input is copied into its
        first channels once, every dense layer is one launch in place (fused.dense_layer_eval), a transition is its site on the full
        buffer (fused.site_eval_any), the 1x1 convolution and the pool into the next block's buffer (fused.avgpool2_into), the head its
        site, the pool and the linear layer.  Whatever has no kernel runs the composition of forward().  Dropout is inactive in
        evaluation."""
        x = self._dense_eval(self.dense1, self.conv1(x), None)
        x = self._dense_eval(self.dense2, *self._transition_eval(self.trans1, x, self.dense2))
        x = self._dense_eval(self.dense3, *self._transition_eval(self.trans2, x, self.dense3))
        y = fused.site_eval_any(self.bn, self.act_q0, x, fused.CLAMP_RELU)
        if y is None:
            y = self.relu(self.act_q0(self.bn(x)))
        x = self.avgpool(y)
        return self.fc(x.reshape(x.size(0), -1))

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


def use_hip_convs(model, dense_eval=False):
    """Channels-last parameters plus `use_qconv`, `use_qconv_pw` (the transitions) and `use_qconv_k3` (the dense layers): with
    channels-last inputs every dense layer then runs on alignq_k3conv_* and both transitions on alignq_pwconv_*; the concatenations keep
    the layout, so no dense layer falls back to MIOpen.  Values, parameter names and state_dict are unchanged.
    dense_eval=True also sets `fuse_dense_eval`: inside eval_step.EvalStep the model then runs DenseNet._forward_eval (one launch per
    dense layer, no concatenation); every other forward is unchanged."""
    model = model.to(memory_format=torch.channels_last)
    paths.apply(model, use_qconv=True, use_qconv_pw=True, use_qconv_k3=True)
    if dense_eval:
        paths.apply(model, fuse_dense_eval=True)
    return model
