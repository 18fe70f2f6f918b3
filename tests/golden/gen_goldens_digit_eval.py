#!/usr/bin/env python3
"""Golden-vector generator for the digit-domain DANN's evaluation pass (the reference's test(), cdf_alignment/dann_digit/main.py:
436-487): imports the reference's own model/dann.py on CPU by gen_goldens_digit.py's recipe and writes

  G24 g24_digit_eval.npz
    MNISTmodel_quant at 8W/32A (the weight quantiser rounds - it is bit-exact against the reference elsewhere; with 32-bit activations
    no activation level can flip), parameters from digit_init.digit_init_, eval mode, alpha = 0, a seeded (4, 1, 28, 28) input:
    the class output of the fp32 model and of a .double() copy, and e_ref, their largest difference.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_goldens_digit_eval.py
"""
import copy
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import gen_goldens as G  # noqa: E402

G.VARIANTS["digit"] = ("cdf_alignment/dann_digit", "utils.options")


def gen():
    import torch
    from digit_init import digit_init_
    q, args = G._enter("digit", ["--bitW", "8", "--abitW", "32"])          # (sets q.device = cpu)
    try:          # model/dann.py imports torchvision.models and never reads it: an empty stand-in where torchvision is not installed
        import torchvision.models  # noqa: F401
    except ImportError:
        tv = types.ModuleType("torchvision")
        tv.models = sys.modules["torchvision.models"] = types.ModuleType("torchvision.models")
        sys.modules["torchvision"] = tv
    m = importlib.import_module("model.dann")
    assert args.method == "ours" and args.img_size == 28
    net32 = digit_init_(m.MNISTmodel_quant(args.stage, 8, 32)).eval()
    net64 = copy.deepcopy(net32).double()
    x = torch.randn(4, 1, 28, 28, generator=torch.Generator().manual_seed(24))
    with torch.no_grad():
        c32, _ = net32(x, 0.0)
        c64, _ = net64(x.double(), 0.0)
    e_ref = float((c32.double() - c64).abs().max())
    print("e_ref", e_ref, "max |class|", float(c64.abs().max()))
    assert 0.0 < e_ref < 2e-6 * float(c64.abs().max())          # (a sanity bound on the fixture: a few fp32 roundings of the logits' scale)
    G._save("g24_digit_eval", stage=np.array(str(args.stage)), x=G._np(x), class32=G._np(c32), class64=G._np(c64),
            e_ref=np.array(e_ref))
    assert os.path.getsize(os.path.join(HERE, "g24_digit_eval.npz")) < 1000000


if __name__ == "__main__":
    gen()
