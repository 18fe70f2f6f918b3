"""Deterministic parameters of the MobileNet-V2 fixtures (G19), shared by the generator (reference side) and the tests (this
repository's model): det_init.det_init_, then the shortcut batch-norm gains (`shortcut.1.weight`, which det_init_'s name rule takes
for a bias) redrawn around 1 like every other batch-norm gain, so that the shortcut branches carry weight in the wiring check."""
import torch

try:
    from .det_init import det_init_          # imported as tests.golden.mobilenet_init (the tests)
except ImportError:
    from det_init import det_init_           # imported from the generator's own directory

REDUCED_CFG = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 320, 1, 2)]      # a 4x4 map in front of AvgPool2d(4) for 16x16 inputs


def mobilenet_init_(module, seed=1000):
    det_init_(module, seed)
    with torch.no_grad():
        for i, (name, p) in enumerate(module.named_parameters()):
            if name.endswith("shortcut.1.weight"):
                g = torch.Generator().manual_seed(seed + 100000 + i)
                p.copy_((1.0 + 0.1 * torch.randn(p.shape, generator=g)).to(p.device))
    return module
