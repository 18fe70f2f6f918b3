#!/usr/bin/env python3
"""Golden-vector generator for the digit-domain DANN (cdf_alignment/dann_digit): imports the reference's own model/dann.py and
model/quantization.py on CPU (the recipe of gen_goldens_densenet.py, whose helpers it shares through gen_goldens.py) and writes

  G23 g23_digit.npz
    (a) state_dict key names and shapes of MNISTmodel_quant ('ours' branch);
    (b) the wiring check at 32W/32A in eval mode (no quantiser rounds, dropout is inactive): both outputs of the fp32 model and of a
        .double() copy on a seeded (4, 1, 28, 28) input with alpha = 0.5, parameters from digit_init.digit_init_, and e_ref, their
        largest difference.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_goldens_digit.py
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
ALPHA = 0.5


def gen():
    import torch
    from digit_init import digit_init_
    q, args = G._enter("digit", ["--bitW", "32", "--abitW", "32"])          # (sets q.device = cpu)
    try:          # model/dann.py imports torchvision.models and never reads it: an empty stand-in where torchvision is not installed
        import torchvision.models  # noqa: F401
    except ImportError:
        tv = types.ModuleType("torchvision")
        tv.models = sys.modules["torchvision.models"] = types.ModuleType("torchvision.models")
        sys.modules["torchvision"] = tv
    m = importlib.import_module("model.dann")
    assert args.method == "ours" and args.img_size == 28
    net32 = m.MNISTmodel_quant(args.stage, 32, 32)
    sd = net32.state_dict()
    out = {"stage": np.array(str(args.stage)), "alpha": np.array(ALPHA),
           "keys": np.array(list(sd.keys())), "shapes": np.array([",".join(map(str, v.shape)) for v in sd.values()])}

    digit_init_(net32).eval()
    net64 = copy.deepcopy(net32).double()
    x = torch.randn(4, 1, 28, 28, generator=torch.Generator().manual_seed(23))
    c32, d32 = net32(x, ALPHA)
    c64, d64 = net64(x.double(), ALPHA)
    e_ref = max(float((c32.double() - c64).abs().max().detach()), float((d32.double() - d64).abs().max().detach()))
    print("e_ref", e_ref, "max |out|", float(c64.detach().abs().max()), float(d64.detach().abs().max()))
    assert 0.0 < e_ref < 1e-5
    out.update({"x": G._np(x), "class32": G._np(c32), "domain32": G._np(d32), "class64": G._np(c64), "domain64": G._np(d64),
                "e_ref": np.array(e_ref)})
    G._save("g23_digit", **out)
    size = os.path.getsize(os.path.join(HERE, "g23_digit.npz"))
    assert size < 1000000, size
    print("bytes", size)


if __name__ == "__main__":
    gen()
