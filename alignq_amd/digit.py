"""The digit-domain DANN (MNIST -> MNIST-M and the like), wired like the 'ours' branch of the reference's cdf_alignment/dann_digit/
model/dann.py (MNISTmodel_quant, :125-230) on the CDF-only namespace (alignq_amd.cdf_alignment), with the SAME attribute names and
Sequential indices (`feature.{0,1,5,6}`, `classifier.{0,1,3,4,6}`, `discriminator.{0,1,3}`), so that state_dict() keys and shapes equal
the reference's and its checkpoints load by name.

What the reference does and this file keeps: `feature` is conv 5x5 (3 -> 32, WITH a bias) -> BN -> act_q -> ReLU -> MaxPool(2) -> conv
5x5 (32 -> 48, with a bias) -> BN -> act_q -> Dropout2d -> ReLU -> MaxPool(2); the 768 features go to the class head and, through the
gradient reversal, to the domain head; forward(input_data, alpha) expands a 1-channel image to 3 channels and returns
(class_output, domain_output).  `img_size` is the reference's args.img_size (28).

Every weight and activation quantiser runs on this repository's kernels.  With use_hip_convs(model) the two convolutions run on
csrc/k5conv_kernels.hip (include/alignq_k5conv.h): the first on its image form (3 input channels folded with the 25 taps into one K),
the second on its body form; batch-norm, ReLU, Dropout2d, the pools and the linear layers go to MIOpen / rocBLAS through PyTorch-ROCm.
The sites run as the composition, or with use_hip_convs(model, train_sites=True) each as one fused.BNQuantPoolFn node
(include/alignq_bnq_pool.h: batch-norm, quantiser, ReLU and the 2 x 2 max-pool folded, three launches each way); training is eager
iterations (train_iteration, with alignq_amd.optimizer.SGD).

Evaluation (eval_step.EvalStep) with use_hip_convs(model, eval_fused=True): MNISTmodel_quant._forward_eval runs each half of `feature`
as ONE alignq_k5conv_site_pool_eval_fwd launch (include/alignq_digit.h: eval-mode batch-norm, quantiser, ReLU and the 2 x 2 max-pool
as the convolution's epilogue); the first reads the one-channel image directly, the second writes the classifier's (B, 768) matrix.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import cdf_alignment as _cdf
from . import fused, paths
from .resnet_office import ReverseLayerF


def conv2d_Q5_fn(w_bit, stage):
    """Conv2d_Q of the CDF namespace plus one opt-in flag: with it the 5x5 / stride 1 / padding 0 convolutions, bias included, run on
    alignq_k5conv_* (ops.conv2d_q reads the flag).  The flag is declared HERE, not on Conv2d_Q: no other model's modules carry it."""
    base = _cdf.conv2d_Q_fn(w_bit=w_bit, stage=stage)

    class Conv2d_Q5(base):
        use_qconv_k5 = False          # kernel-path flag, off unless set (alignq_amd.paths; INTEGRATION.md, "Kernel-path flags")

    return Conv2d_Q5


class MNISTmodel_quant(nn.Module):
    fuse_digit_eval = False           # kernel-path flag, off unless set (alignq_amd.paths; INTEGRATION.md, "Kernel-path flags")
    fuse_train_sites = False          # likewise

    def __init__(self, stage, wbit, abit, img_size=28):
        super().__init__()
        self.restored = False
        self.img_size = img_size
        Conv2d = conv2d_Q5_fn(w_bit=wbit, stage=stage)
        self.feature = nn.Sequential(
            Conv2d(in_channels=3, out_channels=32, kernel_size=(5, 5)),          # 3 28 28 -> 32 24 24
            nn.BatchNorm2d(32),
            _cdf.activation_quantize_fn(a_bit=abit, stage=stage),
            nn.ReLU(inplace=True),
            nn.MaxPool2d(kernel_size=(2, 2)),                                    # 32 12 12
            Conv2d(in_channels=32, out_channels=48, kernel_size=(5, 5)),         # 48 8 8
            nn.BatchNorm2d(48),
            _cdf.activation_quantize_fn(a_bit=abit, stage=stage),
            nn.Dropout2d(),
            nn.ReLU(inplace=True),
            nn.MaxPool2d(kernel_size=(2, 2)),                                    # 48 4 4
        )
        self.classifier = nn.Sequential(
            nn.Linear(48 * 4 * 4, 100), nn.BatchNorm1d(100), nn.ReLU(inplace=True),
            nn.Linear(100, 100), nn.BatchNorm1d(100), nn.ReLU(inplace=True),
            nn.Linear(100, 10),
        )
        self.discriminator = nn.Sequential(
            nn.Linear(48 * 4 * 4, 100), nn.BatchNorm1d(100), nn.ReLU(inplace=True),
            nn.Linear(100, 2),
        )

    def forward(self, input_data, alpha):
        input_data = input_data.expand(input_data.shape[0], 3, self.img_size, self.img_size)
        if self.feature[0].use_qconv_k5:
            # the kernels read a dense channels-last image (the expanded view has a channel stride of 0)
            input_data = input_data.contiguous(memory_format=torch.channels_last)
        if self.fuse_train_sites and self.training and not fused.eval_active():
            feature = self._half_train(5, self._half_train(0, input_data))
        else:
            feature = self.feature(input_data)
        feature = feature.reshape(-1, 48 * 4 * 4)          # (c, h, w) order whatever the layout, as the reference's view
        reverse_feature = ReverseLayerF.apply(feature, alpha)
        return self.classifier(feature), self.discriminator(reverse_feature)

    def _half_train(self, i, x):
        """feature[i : i + 5 or 6] on x in training with `fuse_train_sites`: the convolution, then BN -> act_q -> ReLU -> MaxPool2d(2)
        as one fused.BNQuantPoolFn node (include/alignq_bnq_pool.h); where fused.bn_act_pool returns None, the modules.  The second
        half's Dropout2d runs on the POOLED tensor: its noise is one draw per (sample, channel), independent of H x W, and scaling a
        whole channel by 0 or 2 commutes with ReLU and with the window maximum, so the values are those of the reference's order
        (a zero may differ in sign)."""
        f = self.feature
        z = f[i](x)
        drop = f[i + 3] if isinstance(f[i + 3], nn.Dropout2d) else None
        y = fused.bn_act_pool(f[i + 1], f[i + 2], z)
        if y is None:
            return f[i + 1:i + (6 if drop is not None else 5)](z)
        return y if drop is None else drop(y)

    # ---- evaluation (eval_step.EvalStep: the reference's test(), main.py:436-487 - eval mode, alpha = 0, the class logits) ----
    def _half_eval(self, i, x, flat):
        """feature[i : i + 5 or 6] on x in evaluation: conv 5x5 + bias, BN, act_q, (Dropout2d: the identity,) ReLU, MaxPool2d(2).  With
        `fuse_digit_eval` one launch (fused.k5_site_pool_eval); where that returns None, or without the flag, the modules.  x may be
        the one-channel image for the first half."""
        conv, bn, act = self.feature[i], self.feature[i + 1], self.feature[i + 2]
        y = fused.k5_site_pool_eval(conv, bn, act, x, flat=flat) if self.fuse_digit_eval and fused.eval_active() else None
        if y is None:
            if x.shape[1] != conv.in_channels:
                x = x.expand(x.shape[0], conv.in_channels, x.shape[2], x.shape[3])
                if conv.use_qconv_k5:
                    x = x.contiguous(memory_format=torch.channels_last)
            y = F.max_pool2d(F.relu(act(bn(conv(x)))), 2)
            if flat:
                y = y.reshape(y.shape[0], -1)          # (c, h, w) order whatever the layout
        return y

    def _forward_eval(self, input_data):
        """The class logits of forward(input_data, alpha) in eval mode (alpha only scales the reversed gradient; the domain head is not
        evaluated).  The second half hands the classifier its (B, 768) matrix directly."""
        if self.training:
            raise RuntimeError("MNISTmodel_quant._forward_eval: the model is in training mode")
        x = self._half_eval(0, input_data, False)
        return self.classifier(self._half_eval(5, x, True))


def use_hip_convs(model, eval_fused=False, train_sites=False):
    """Channels-last parameters plus `use_qconv` and `use_qconv_k5`: both convolutions then run on alignq_k5conv_*, and `forward` hands
    the first one a dense channels-last image.  Values, parameter names and state_dict are unchanged.
    eval_fused=True also sets `fuse_digit_eval`: inside eval_step.EvalStep each half of `feature` is then one launch
    (include/alignq_digit.h); `forward` and every other launch are unchanged.
    train_sites=True also sets `fuse_train_sites`: in training forwards each BN -> act_q -> [Dropout2d ->] ReLU -> MaxPool2d(2) of
    `feature` is one fused.BNQuantPoolFn node (include/alignq_bnq_pool.h), Dropout2d applied to the pooled tensor."""
    model = model.to(memory_format=torch.channels_last)
    paths.apply(model, use_qconv=True, use_qconv_k5=True)
    if eval_fused:
        paths.apply(model, fuse_digit_eval=True)
    if train_sites:
        paths.apply(model, fuse_train_sites=True)
    return model


def train_iteration(model, optimizer, images_src, class_src, images_tgt, alpha):
    """One eager training iteration of the reference's main.py:355-372: the source batch's class and domain losses plus the target
    batch's domain loss (source = domain 0, target = domain 1), backward, one SGD step (alignq_amd.optimizer.SGD; no tensor is in the
    CDF-approximated set).  Returns the three losses."""
    optimizer.zero_grad()
    src_class, src_domain = model(images_src, alpha)
    _, tgt_domain = model(images_tgt, alpha)
    dev = images_src.device
    losses = (F.cross_entropy(src_class, class_src),
              F.cross_entropy(src_domain, torch.zeros(len(images_src), dtype=torch.long, device=dev)),
              F.cross_entropy(tgt_domain, torch.ones(len(images_tgt), dtype=torch.long, device=dev)))
    sum(losses).backward()
    optimizer.step([], [], [], 0.0, 0.0)
    return losses
