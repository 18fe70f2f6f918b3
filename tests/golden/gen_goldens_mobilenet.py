#!/usr/bin/env python3
"""Golden-vector generator for MobileNet-V2 (cdf_alignment/mobilenet-v2-svhn): imports the reference's own model/mobilenetV2.py and
model/quantization.py on CPU (the recipe of gen_goldens.py, whose helpers it uses; `mobilenetV2.device` is overwritten with cpu like
`q.device`) and writes

  G19 g19_mobilenet.npz
    (a) state_dict key names and shapes at the reduced cfg of mobilenet_init.REDUCED_CFG and at the class's own cfg;
    (b) the depthwise layers layers[0..3].conv2 of the reduced model at 4W/4A, teacher-forced: raw filter, the module's own input
        x (the first TF_BATCH samples of the batch of 4: the fixture's size), the quantiser's weight_q, the output y, a seeded dy
        and autograd's dx, d weight_q, d weight;
    (c) the wiring check at 32W/32A: the logits of the fp32 model and of a .double() copy on the same input, and e_ref, their
        largest difference.

  Two conditions are asserted on (b), the filter seeds being searched until they hold: tests/oracle_c.py's weight quantiser gives
  weight_q bit-equal to the reference's, and every weight's pre-round value (cdf * 15, in bin units) is at least MARGIN away from
  a rounding boundary, so that no implementation's last-bit noise can move a level.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_goldens_mobilenet.py
"""
import copy
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import gen_goldens as G  # noqa: E402

G.VARIANTS["mobilenet"] = ("cdf_alignment/mobilenet-v2-svhn", "utils.options")
MARGIN = 1e-3
N_DW = 4
TF_BATCH = 2


def _enter(bits):
    import torch
    q, args = G._enter("mobilenet", ["--bitW", str(bits), "--abitW", str(bits)])
    m = importlib.import_module("model.mobilenetV2")
    m.device = torch.device("cpu")
    return q, args, m


def _keys(net):
    sd = net.state_dict()
    return np.array(list(sd.keys())), np.array([",".join(map(str, v.shape)) for v in sd.values()])


def _safe_filter(q, C, seed0):
    """A seeded (C, 1, 3, 3) filter whose 4-bit levels no rounding noise can move, and which the C oracle quantises like the
    reference: (filter, seed, smallest distance to a rounding boundary in bin units)."""
    import torch
    from tests import oracle_c as O
    for seed in range(seed0, seed0 + 2000):
        w = torch.randn((C, 1, 3, 3), generator=torch.Generator().manual_seed(seed)) * (2.0 / (C * 9)) ** 0.5
        pre = G._np(q.cdf(torch.mean(w), torch.std(w), "w")(w)[0]).astype(np.float32) * np.float32(15)
        dist = float(np.abs((pre - np.floor(pre)) - 0.5).min())
        if dist < MARGIN:
            continue
        ref_q = G._np(q.weight_quantize_fn(4, "no_align")(w))
        ours = O.weight_quant_fwd(G._np(w), O.weight_stats(G._np(w)), 4, O.FORMULA_CDF)[0]
        if np.array_equal(ours.view(np.uint32), ref_q.view(np.uint32)):
            return w, seed, dist
    raise AssertionError(f"no filter seed for C={C}")


def gen():
    import torch
    from mobilenet_init import REDUCED_CFG, mobilenet_init_
    torch.manual_seed(0)
    q, args, m = _enter(4)
    assert args.bitW == 4 and args.abitW == 4 and float(args.act_range) == 2.0
    out = {"stage": np.array(str(args.stage)), "act_range": np.array(float(args.act_range)), "margin": np.array(MARGIN)}

    # (a) names and shapes
    out["keys_full"], out["shapes_full"] = _keys(m.mobile_v2(4, 4, args.stage))
    full_cfg = list(m.MobileNetV2.cfg)
    m.MobileNetV2.cfg = list(REDUCED_CFG)
    net = m.mobile_v2(4, 4, args.stage)
    out["keys_reduced"], out["shapes_reduced"] = _keys(net)
    out["cfg_reduced"], out["cfg_full"] = np.array(REDUCED_CFG), np.array(full_cfg)
    print("reduced model parameters:", sum(p.numel() for p in net.parameters()))

    # (b) the depthwise layers, teacher-forced
    mobilenet_init_(net)
    net.train()
    dws = [net.layers[i].conv2 for i in range(N_DW)]
    seeds, dists = [], []
    with torch.no_grad():
        for i, conv in enumerate(dws):
            w, seed, dist = _safe_filter(q, conv.weight.shape[0], 1900 + 10000 * i)
            conv.weight.copy_(w)
            seeds.append(seed)
            dists.append(dist)
    out["filter_seeds"], out["boundary_dist"] = np.array(seeds), np.array(dists)
    xin = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(19))
    seen = {}
    hooks = [conv.register_forward_pre_hook(lambda mod, inp, i=i: seen.__setitem__(i, inp[0].detach().clone()))
             for i, conv in enumerate(dws)]
    logits = net(xin)
    assert torch.isfinite(logits).all()
    for h in hooks:
        h.remove()
    g = torch.Generator().manual_seed(1919)
    for i, conv in enumerate(dws):
        x = seen[i][:TF_BATCH].clone().requires_grad_(True)
        held = {}

        def keep(mod, inp, res, held=held):
            res.retain_grad()
            held["wq"] = res
        h = conv.quantize_fn.register_forward_hook(keep)
        conv.weight.grad = None
        y = conv(x)
        h.remove()
        dy = torch.randn(y.shape, generator=g)
        y.backward(dy)
        wq = held["wq"]
        C, s = conv.weight.shape[0], conv.stride[0]
        assert tuple(x.shape[1:]) == {0: (32, 16, 16), 1: (96, 16, 16), 2: (144, 8, 8), 3: (144, 8, 8)}[i] and s == (1, 2, 1, 2)[i]
        out.update({f"dw{i}_w": G._np(conv.weight), f"dw{i}_x": G._np(x), f"dw{i}_wq": G._np(wq), f"dw{i}_y": G._np(y),
                    f"dw{i}_dy": G._np(dy), f"dw{i}_dx": G._np(x.grad), f"dw{i}_dwq": G._np(wq.grad),
                    f"dw{i}_dw": G._np(conv.weight.grad), f"dw{i}_stride": np.array(s)})
        # the two conditions, on what is stored
        from tests import oracle_c as O
        ours = O.weight_quant_fwd(out[f"dw{i}_w"], O.weight_stats(out[f"dw{i}_w"]), 4, O.FORMULA_CDF)[0]
        assert np.array_equal(ours.view(np.uint32), out[f"dw{i}_wq"].view(np.uint32)), i
        pre = G._np(q.cdf(torch.mean(conv.weight), torch.std(conv.weight), "w")(conv.weight)[0]).astype(np.float32) * np.float32(15)
        assert float(np.abs((pre - np.floor(pre)) - 0.5).min()) >= MARGIN, i

    # (c) the wiring check at 32 / 32 bits: no rounding anywhere.  (weight_quantize_fn / activation_quantize_fn read their widths
    # from the constructor arguments, so the model is built in this process)
    net32 = mobilenet_init_(m.mobile_v2(32, 32, args.stage)).train()
    net64 = copy.deepcopy(net32).double()          # before the first forward: the model keeps self.out, which deepcopy refuses
    l32 = net32(xin)
    l64 = net64(xin.double())
    e_ref = float((l32.double() - l64).abs().max().detach())
    print("e_ref", e_ref, "max |logit|", float(l64.detach().abs().max()))
    assert 0.0 < e_ref < 1e-5
    out.update({"c_x": G._np(xin), "c_logits32": G._np(l32), "c_logits64": G._np(l64), "c_e_ref": np.array(e_ref)})
    G._save("g19_mobilenet", **out)
    size = os.path.getsize(os.path.join(HERE, "g19_mobilenet.npz"))
    assert size < 1000000, size
    print("bytes", size)


if __name__ == "__main__":
    gen()
