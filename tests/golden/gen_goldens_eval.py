#!/usr/bin/env python3
"""Golden-vector generator for the evaluation pass (the reference's test(): eval mode, forward under no_grad, cross-entropy,
utils.accuracy): imports the reference's own modules on the CPU (the recipe of gen_goldens.py, whose helpers it uses) and writes,
per tree (admm = cdf_alignment_admm/resnet-56-cifar-10, cdf = cdf_alignment/resnet-20-cifar-10, office = .../dann_office):

  G17 g17_eval_site_<tree>.npz   one site: relu(act_q(bn.eval()(z)) + residual) for k in {2, 4, 8}, the quantiser's own output,
                                 and n_flip_ref = the elements whose level differs between this fp32 and an fp64 evaluation;
  G18 g18_eval_net_<tree>.npz    a whole network in eval mode after a few training-mode forwards: logits, cross-entropy,
                                 Prec@1 / Prec@5 from utils.accuracy, the batch-norm buffers after the training forwards.

Inputs and initial parameters come from eval_inputs.py / det_init.py by seed and are not stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_goldens_eval.py            # all (one child process per tree)
    python tests/golden/gen_goldens_eval.py --variant admm                       # one tree
"""
import argparse
import math
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import eval_inputs as E  # noqa: E402
import gen_goldens as G  # noqa: E402

VARIANT = {"admm": "admm_cifar", "cdf": "cdf_only", "office": "office"}


def _enter(tree):
    B, _, _, bits, _ = E.NET[tree]
    return G._enter(VARIANT[tree], ["--bitW", str(bits), "--abitW", str(bits), "--train_batch_size", str(B),
                                    "--eval_batch_size", str(B)])


def _site_act(q, tree, k, stage, B):
    """the tree's activation quantiser as its ResNet builds it; returns a callable x -> x_q"""
    if tree == "cdf":
        return q.activation_quantize_fn(k, stage)
    from utils.admm import ADMM
    import torch
    torch.manual_seed(17)
    mod = (q.activation_quantize_fn2 if tree == "office" else q.activation_quantize_fn)(k, stage, ADMM(B))
    return lambda x: mod(x)[0]              # test() discards the trans loss


def gen_site(tree, q, args):
    import torch
    z, res, gamma, beta, mean, var = E.site_inputs(tree)
    bn = E.site_bn(tree)
    r = float(args.act_range)
    stage = "second" if tree != "office" else str(args.stage)
    out = {"act_range": np.array(r, dtype=np.float32), "bn_eps": np.array(E.BN_EPS), "ks": np.array(E.SITE_KS),
           "shape": np.array(E.SITE_SHAPE[tree])}
    # the same site in float64: batch-norm as torch's eval mode writes it, then the transform and the rounding
    z64 = z.double()
    sh = (1, -1, 1, 1)
    x64 = (z64 - mean.double().view(sh)) / torch.sqrt(var.double().view(sh) + E.BN_EPS) * gamma.double().view(sh) + beta.double().view(sh)
    phi64 = 0.5 * (1.0 + torch.erf(x64 / math.sqrt(2.0)))
    with torch.no_grad():
        for k in E.SITE_KS:
            n = 2 ** k - 1
            act = _site_act(q, tree, k, stage, z.shape[0])
            xq = act(bn(z))
            y = torch.relu(xq + res)
            idx64 = torch.round(phi64 * n) if tree == "cdf" else torch.round((phi64 * 2 - 1) * r * n)
            idx32 = E.levels(G._np(xq), k, r, tree)
            out[f"xq_k{k}"], out[f"y_k{k}"] = G._np(xq), G._np(y)
            out[f"n_flip_ref_k{k}"] = np.array(int(np.count_nonzero(idx32 != idx64.numpy().astype(np.int64))))
    G._save("g17_eval_site_" + tree, **out)


def _build_net(tree, args):
    import importlib
    import torch
    from det_init import det_init_
    r = importlib.import_module("model.resnet")
    r.device = torch.device("cpu")
    bits = E.NET[tree][3]
    torch.manual_seed(0)
    if tree == "office":
        net = r.DANN(lambda w, a, s: r.ResNet(w, a, s, r.Bottleneck, [1, 1, 1, 1], width_per_group=8), bits, bits, args.stage)
    else:
        net = r.PreActResNet(r.PreActBlock_conv_Q, [1, 1, 1], bits, bits, "second", 10)
    det_init_(net)
    return net


def _logits(tree, net, x):
    if tree == "office":
        return net(x, alpha=0)[0]           # dann_office/main.py test(): class_output, _, _ = model(inputs, alpha)
    out = net(x)
    return out[0] if isinstance(out, tuple) else out


def gen_net(tree, q, args):
    import torch
    from utils.common import accuracy
    B, S, classes, bits, n_train = E.NET[tree]
    net = _build_net(tree, args)
    xtr, xev, _ = E.net_inputs(tree)
    net.train()
    with torch.no_grad():
        for i in range(n_train):            # training-mode forwards move the running statistics
            _logits(tree, net, xtr[i])
    net.eval()
    with torch.no_grad():
        logits = _logits(tree, net, xev)
    lg = G._np(logits)
    for seed in range(500, 600):            # targets whose counts no bin flip decides
        _, _, y = E.net_inputs(tree, seed)
        if E.margins(lg, y.numpy()).min() > E.MARGIN:
            break
    else:
        raise AssertionError("no target draw with the margin")
    assert E.margins(lg, y.numpy()).min() > E.MARGIN
    ce = torch.nn.CrossEntropyLoss()(logits, y)
    prec1, prec5 = accuracy(logits, y, topk=(1, 5))
    out = {"logits": lg, "ce": G._np(ce), "prec1": G._np(prec1[0]), "prec5": G._np(prec5[0]), "target_seed": np.array(seed),
           "bits": np.array(bits), "batch": np.array(B), "margin": np.array(E.MARGIN), "stage": np.array(str(args.stage)),
           "act_range": np.array(float(args.act_range), dtype=np.float32),
           "names": np.array([n for n, _ in net.named_parameters()])}
    for name, buf in net.named_buffers():
        if name.endswith("running_mean") or name.endswith("running_var") or name.endswith("num_batches_tracked"):
            out["buf/" + name] = G._np(buf)
    G._save("g18_eval_net_" + tree, **out)


def gen(tree):
    q, args = _enter(tree)
    gen_site(tree, q, args)
    gen_net(tree, q, args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=sorted(VARIANT), default=None)
    a = ap.parse_args()
    if a.variant is None:
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
        for v in VARIANT:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", v], check=True, env=env)
        return
    gen(a.variant)


if __name__ == "__main__":
    main()
