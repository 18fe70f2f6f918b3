"""MobileNet-V2 for SVHN, wired like the reference's cdf_alignment/mobilenet-v2-svhn/model/mobilenetV2.py (:25-135) on the CDF-only
namespace (alignq_amd.cdf_alignment), with the SAME attribute names (`conv1`, `bn1`, `act_q1`, `layers[i].{act_q1,act_q2,act_q3,
act_skip,conv1,bn1,conv2,bn2,conv3,bn3,shortcut.{0,1}}`, `conv2`, `bn2`, `act_q2`, `linear`), so that state_dict() keys and shapes
equal the reference's and its checkpoints load by name.

What the reference does and this file keeps: `cfg` is a class attribute; EVERY stride-1 block has the shortcut convolution +
batch-norm + `act_skip` + ReLU, also where in_planes == out_planes; ReLU6 follows act_q1 / act_q2 of a block and nothing follows
act_q3; the shortcut is added in place; the head is AvgPool2d(4) (a 4x4 map for 32x32 inputs), kept as `self.out`, and
Linear(1280, num_classes).

Every weight and activation quantiser runs on this repository's kernels.  With use_hip_convs(model) and channels-last inputs the
depthwise 3x3 convolutions (`layers[i].conv2`) run on csrc/dwconv_kernels.hip and the pointwise ones whose channel counts are
multiples of 64 on the exact-product GEMMs; with use_hip_convs(model, pointwise=True) the other pointwise ones (channel counts
multiples of 8) run on csrc/pointwise_kernels.hip with the same arithmetic; the stem (and, without the opt-in, those pointwise
convolutions), batch-norm and the linear layer go to MIOpen / rocBLAS through PyTorch-ROCm.

Inside eval_step.EvalStep (fused.eval_scope) both forwards fold every site into one launch (include/alignq_mobile.h): the eval-mode
batch-norm, the quantiser and ReLU / ReLU6 (fused.site_eval_any), the depthwise convolution with its site as the epilogue
(fused.dw_site_eval) and the stride-1 tail `act_q3(bn3(.)) + relu(act_skip(bn_s(.)))` (fused.site_eval_twin).  Outside it - training,
or a bare `model.eval(); model(x)` - they are the composition above.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import cdf_alignment as _cdf
from . import fused, paths


class Block(nn.Module):
    """Inverted residual: 1x1 expansion, depthwise 3x3 (stride), 1x1 projection; a convolutional shortcut at stride 1."""

    def __init__(self, stage, wbit, abit, in_planes, out_planes, expansion, stride):
        super().__init__()
        self.stride = stride
        planes = expansion * in_planes
        Conv2d = _cdf.conv2d_Q_fn(w_bit=wbit, stage=stage)
        for name in ("act_q1", "act_q2", "act_q3", "act_skip"):
            setattr(self, name, _cdf.activation_quantize_fn(a_bit=abit, stage=stage))
        self.conv1 = Conv2d(in_planes, planes, kernel_size=1, stride=1, padding=0, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, groups=planes, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = Conv2d(planes, out_planes, kernel_size=1, stride=1, padding=0, bias=False)
        self.bn3 = nn.BatchNorm2d(out_planes)
        self.relu = nn.ReLU6()
        self.shortcut = None
        if stride == 1:
            self.shortcut = nn.Sequential(Conv2d(in_planes, out_planes, kernel_size=1, stride=1, padding=0, bias=False),
                                          nn.BatchNorm2d(out_planes), self.act_skip, nn.ReLU(inplace=True))

    def forward(self, x):
        if fused.eval_active():
            return self._forward_eval(x)
        out = self.relu(self.act_q1(self.bn1(self.conv1(x))))
        out = self.relu(self.act_q2(self.bn2(self.conv2(out))))
        out = self.act_q3(self.bn3(self.conv3(out)))
        if self.stride == 1:
            out += self.shortcut(x)
        return out

    def _forward_eval(self, x):
        """forward() inside fused.eval_scope (eval_step.EvalStep): every site one launch - batch-norm's running statistics, the
        quantiser and ReLU6 folded (fused.site_eval_any), the depthwise convolution with its site as the epilogue
        (fused.dw_site_eval), the stride-1 tail `act_q3(bn3(.)) + relu(act_skip(bn_s(.)))` in one pass (fused.site_eval_twin).  A site
        whose kernel does not apply runs the composition of forward()."""
        z = self.conv1(x)
        out = fused.site_eval_any(self.bn1, self.act_q1, z, fused.CLAMP_RELU6)
        if out is None:
            out = self.relu(self.act_q1(self.bn1(z)))
        mid = fused.dw_site_eval(self.conv2, self.bn2, self.act_q2, out, fused.CLAMP_RELU6)
        if mid is None:
            mid = self.relu(self.act_q2(self.bn2(self.conv2(out))))
        z = self.conv3(mid)
        if self.stride != 1:
            out = fused.site_eval_any(self.bn3, self.act_q3, z, fused.CLAMP_NONE)
            return self.act_q3(self.bn3(z)) if out is None else out
        conv_s, bn_s, act_s, relu_s = self.shortcut
        zs = conv_s(x)
        out = fused.site_eval_twin(self.bn3, self.act_q3, z, bn_s, act_s, zs, fused.CLAMP_RELU)
        if out is None:
            out = self.act_q3(self.bn3(z))
            out += relu_s(act_s(bn_s(zs)))
        return out


class MobileNetV2(nn.Module):
    # (expansion, out_planes, num_blocks, stride)
    cfg = [(1, 16, 1, 1), (6, 24, 2, 1), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]

    def __init__(self, block, wbit, abit, stage, num_classes=10):
        super().__init__()
        Conv2d = _cdf.conv2d_Q_fn(w_bit=wbit, stage=stage)
        self.act_q1 = _cdf.activation_quantize_fn(a_bit=abit, stage=stage)
        self.act_q2 = _cdf.activation_quantize_fn(a_bit=abit, stage=stage)
        self.conv1 = Conv2d(3, 32, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(32)
        self.layers = self._make_layers(block, wbit, abit, stage, in_planes=32)
        self.conv2 = Conv2d(320, 1280, kernel_size=1, stride=1, padding=0, bias=False)
        self.bn2 = nn.BatchNorm2d(1280)
        self.linear = nn.Linear(1280, num_classes)
        self.relu = nn.ReLU(inplace=True)
        self.avg_pool2d = nn.AvgPool2d(4)

    def _make_layers(self, block, wbit, abit, stage, in_planes):
        layers = []
        for expansion, out_planes, num_blocks, stride in self.cfg:
            for s in [stride] + [1] * (num_blocks - 1):
                layers.append(block(stage, wbit, abit, in_planes, out_planes, expansion, s))
                in_planes = out_planes
        return nn.Sequential(*layers)

    def _site(self, bn, act, z):
        """relu(act(bn(z))): one launch inside fused.eval_scope where the folded kernel applies, else the composition"""
        out = fused.site_eval_any(bn, act, z, fused.CLAMP_RELU) if fused.eval_active() else None
        return self.relu(act(bn(z))) if out is None else out

    def forward(self, x):
        if fused.eval_active():
            out = self.layers(self._site(self.bn1, self.act_q1, self.conv1(x)))
            out = self._site(self.bn2, self.act_q2, self.conv2(out))
            self.out = self.avg_pool2d(out)
            return self.linear(self.out.view(self.out.size(0), -1))
        out = self.relu(self.act_q1(self.bn1(self.conv1(x))))
        out = self.layers(out)
        out = self.relu(self.act_q2(self.bn2(self.conv2(out))))
        self.out = self.avg_pool2d(out)
        return self.linear(self.out.view(self.out.size(0), -1))


def mobile_v2(wbit, abit, stage, num_classes=10):
    return MobileNetV2(Block, wbit, abit, stage, num_classes=num_classes)


def use_hip_convs(model, pointwise=False):
    """Channels-last parameters plus `use_qconv` on every Conv2d_Q (what TrainStep(channels_last=True, qconv=True) does for its
    models): with channels-last inputs the convolutions this repository has kernels for then run on them.  Values, parameter
    names and state_dict are unchanged.
    pointwise=True also sets `use_qconv_pw`: the 1x1 convolutions whose channel counts are multiples of 8 (and not both of 64) run
    on alignq_pwconv_* (include/alignq_pointwise.h) instead of F.conv2d - every supported shape, whatever its speed: the point is
    the defined arithmetic.  Off by default: every launch is then what it was."""
    model = model.to(memory_format=torch.channels_last)
    paths.apply(model, use_qconv=True, **({"use_qconv_pw": True} if pointwise else {}))
    return model
