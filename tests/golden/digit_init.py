"""Deterministic parameters of the digit-DANN fixture (G23), shared by the generator (reference side) and the tests (this repository's
model): det_init's recipe - torch's CPU generator seeded per tensor by its position in named_parameters order - with the batch-norm
gains told by shape and name (the model's batch-norms sit in Sequentials: `feature.1.weight`, `classifier.4.weight`; no name says
`bn`): every 1-D `weight` is a gain and is drawn around 1."""
import math

import torch


def digit_init_(module, seed=2300):
    with torch.no_grad():
        for i, (name, p) in enumerate(module.named_parameters()):
            g = torch.Generator().manual_seed(seed + i)
            if p.dim() == 4:                                          # conv weight: kaiming fan_out scale
                v = torch.randn(p.shape, generator=g) * math.sqrt(2.0 / (p.shape[0] * p.shape[2] * p.shape[3]))
            elif p.dim() == 2:                                        # linear weight
                v = torch.randn(p.shape, generator=g) * 0.05
            elif name.endswith("weight"):                             # batch-norm gain
                v = 1.0 + 0.1 * torch.randn(p.shape, generator=g)
            else:                                                     # biases
                v = 0.05 * torch.randn(p.shape, generator=g)
            p.copy_(v.to(p.device))
    return module
