#!/usr/bin/env python3
"""Golden-vector generator for DenseNet-40 (cdf_alignment/dense-cifar-10): imports the reference's own model/densenet.py and
model/quantization.py on CPU (the recipe of gen_goldens_mobilenet.py, whose helpers it shares through gen_goldens.py) and writes

  G21 g21_densenet.npz
    (a) state_dict key names and shapes at depth 40 (densenet_40_quant: 236 keys) and at the reduced geometry of
        densenet_init.REDUCED (depth 10, compressionRate 1);
    (b) the dense layers dense1[0], dense2[0], dense2[1], dense3[1] of the reduced model at 4W/4A, teacher-forced on the FIRST sample
        of the batch: raw filter, the module's own input x, the quantiser's weight_q, the output y, a seeded dy and autograd's dx,
        d weight_q, d weight;
    (c) the wiring check at 32W/32A: the logits of the fp32 model and of a .double() copy on the same input, and e_ref, their
        largest difference.

  Two conditions are asserted on (b), the filter seeds being searched until they hold (G19's, with its MARGIN): tests/oracle_c.py's
  weight quantiser gives weight_q bit-equal to the reference's, and every weight's pre-round value (cdf * 15, in bin units) is at
  least MARGIN away from a rounding boundary, so that no implementation's last-bit noise can move a level.  G19's filters have 9 C
  weights; these have up to 9072, where no plain draw keeps all of them clear, so every seeded draw is first repaired (_safe_filter:
  the few weights near a boundary are moved off it) and the conditions are then asserted on what is stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_goldens_densenet.py
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

G.VARIANTS["densenet"] = ("cdf_alignment/dense-cifar-10", "utils.options")
MARGIN = 1e-3


def _enter(bits):
    q, args = G._enter("densenet", ["--bitW", str(bits), "--abitW", str(bits)])          # (sets q.device = cpu)
    return q, args, importlib.import_module("model.densenet")


def _keys(net):
    sd = net.state_dict()
    return np.array(list(sd.keys())), np.array([",".join(map(str, v.shape)) for v in sd.values()])


def _pre_round_dist(q, w):
    import torch
    pre = G._np(q.cdf(torch.mean(w), torch.std(w), "w")(w)[0]).astype(np.float32) * np.float32(15)
    return float(np.abs((pre - np.floor(pre)) - 0.5).min())


def _safe_filter(q, shape, seed0):
    """A seeded filter whose 4-bit levels no rounding noise can move, and which the C oracle quantises like the reference:
    (filter, seed, smallest distance to a rounding boundary in bin units)."""
    import torch
    from tests import oracle_c as O
    cout, cin = shape[0], shape[1]
    for seed in range(seed0, seed0 + 200):
        w = torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * (2.0 / (cout * 9)) ** 0.5
        # These filters have 2592 to 9072 weights: a plain draw keeps ALL of them MARGIN away from a boundary once in e^5 to e^18
        # seeds.  So the draw is repaired: a weight closer than 3 MARGIN is moved by 2 % of the filter's standard deviation, away
        # from the boundary, and the filter is looked at again (its mean and deviation move a little with every repair).
        for _ in range(50):
            pre = q.cdf(torch.mean(w), torch.std(w), "w")(w)[0].detach().to(torch.float32) * 15.0
            off = (pre - torch.floor(pre)) - 0.5
            near = off.abs() < 3 * MARGIN
            if not bool(near.any()):
                break
            step = 0.02 * float(torch.std(w))
            w = torch.where(near, w + torch.where(off >= 0, step, -step), w)
        dist = _pre_round_dist(q, w)
        if dist < MARGIN:
            continue
        ref_q = G._np(q.weight_quantize_fn(4, "no_align")(w))
        ours = O.weight_quant_fwd(G._np(w), O.weight_stats(G._np(w)), 4, O.FORMULA_CDF)[0]
        if np.array_equal(ours.view(np.uint32), ref_q.view(np.uint32)):
            return w, seed, dist
    raise AssertionError(f"no filter seed for {cin} -> {cout}")


def gen():
    import torch
    from densenet_init import REDUCED, TF_LAYERS, densenet_init_
    torch.manual_seed(0)
    q, args, m = _enter(4)
    assert args.bitW == 4 and args.abitW == 4 and float(args.act_range) == 2.0
    out = {"stage": np.array(str(args.stage)), "act_range": np.array(float(args.act_range)), "margin": np.array(MARGIN)}

    # (a) names and shapes
    out["keys_full"], out["shapes_full"] = _keys(m.densenet_40_quant(4, 4, args.stage))
    assert len(out["keys_full"]) == 236
    net = m.DenseNet(4, 4, args.stage, **REDUCED)
    out["keys_reduced"], out["shapes_reduced"] = _keys(net)
    print("reduced model parameters:", sum(p.numel() for p in net.parameters()))

    # (b) four dense layers, teacher-forced
    densenet_init_(net)
    net.train()
    convs = [getattr(net, stage)[i].conv1 for stage, i in TF_LAYERS]
    seeds, dists = [], []
    with torch.no_grad():
        for i, conv in enumerate(convs):
            w, seed, dist = _safe_filter(q, tuple(conv.weight.shape), 2100 + 10000 * i)
            conv.weight.copy_(w)
            seeds.append(seed)
            dists.append(dist)
    out["filter_seeds"], out["boundary_dist"] = np.array(seeds), np.array(dists)
    xin = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(21))
    seen = {}
    hooks = [conv.register_forward_pre_hook(lambda mod, inp, i=i: seen.__setitem__(i, inp[0].detach().clone()))
             for i, conv in enumerate(convs)]
    logits = net(xin)
    assert torch.isfinite(logits).all()
    for h in hooks:
        h.remove()
    g = torch.Generator().manual_seed(2121)
    from tests import oracle_c as O
    for i, conv in enumerate(convs):
        x = seen[i][:1].clone().requires_grad_(True)
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
        assert tuple(x.shape[1:]) == {0: (24, 32, 32), 1: (48, 16, 16), 2: (60, 16, 16), 3: (84, 8, 8)}[i] and y.shape[1] == 12
        out.update({f"k{i}_w": G._np(conv.weight), f"k{i}_x": G._np(x), f"k{i}_wq": G._np(wq), f"k{i}_y": G._np(y),
                    f"k{i}_dy": G._np(dy), f"k{i}_dx": G._np(x.grad), f"k{i}_dwq": G._np(wq.grad), f"k{i}_dw": G._np(conv.weight.grad)})
        # the two conditions, on what is stored
        ours = O.weight_quant_fwd(out[f"k{i}_w"], O.weight_stats(out[f"k{i}_w"]), 4, O.FORMULA_CDF)[0]
        assert np.array_equal(ours.view(np.uint32), out[f"k{i}_wq"].view(np.uint32)), i
        assert _pre_round_dist(q, conv.weight) >= MARGIN, i

    # (c) the wiring check at 32 / 32 bits: no rounding anywhere.  (weight_quantize_fn / activation_quantize_fn read their widths
    # from the constructor arguments, so the model is built in this process)
    net32 = densenet_init_(m.DenseNet(32, 32, args.stage, **REDUCED)).train()
    net64 = copy.deepcopy(net32).double()
    l32 = net32(xin)
    l64 = net64(xin.double())
    e_ref = float((l32.double() - l64).abs().max().detach())
    print("e_ref", e_ref, "max |logit|", float(l64.detach().abs().max()))
    assert 0.0 < e_ref < 1e-5
    out.update({"c_x": G._np(xin), "c_logits32": G._np(l32), "c_logits64": G._np(l64), "c_e_ref": np.array(e_ref)})
    G._save("g21_densenet", **out)
    size = os.path.getsize(os.path.join(HERE, "g21_densenet.npz"))
    assert size < 1000000, size
    print("bytes", size)


if __name__ == "__main__":
    gen()
