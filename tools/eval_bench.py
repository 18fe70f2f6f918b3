#!/usr/bin/env python
"""Images/s of a whole evaluation (100 batches, including begin() and result()) for the `model.eval()` path that EvalStep replaces
and for EvalStep, eager and captured.  Prints one JSON line.

    python tools/eval_bench.py [--batches 100] [--configs r20_admm,r20_cdf,r56_admm,r50_dann] [--rounds 3]

The baseline is the reference's test() on this repository's modules as they stood before EvalStep: eval mode, no_grad, the same
memory layout and use_qconv, F.cross_entropy + topk accuracy with their two host reads per batch (utils/common.py:78-92).  The
paths are timed in interleaved rounds in one process; the median round is reported."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alignq_amd import config  # noqa: E402
from alignq_amd.eval_step import EvalStep  # noqa: E402

CONFIGS = {          # name: (kind, units / None, bits, batch, classes, image side)
    "r20_admm": ("admm", [3, 3, 3], 8, 100, 10, 32),
    "r20_cdf": ("cdf", [3, 3, 3], 8, 100, 10, 32),
    "r56_admm": ("admm", [9, 9, 9], 4, 100, 10, 32),
    "r50_dann": ("dann", None, 8, 28, 31, 224),
}


def build(kind, units, bits, dev):
    config.args.bitW = config.args.abitW = bits
    torch.manual_seed(0)
    if kind == "dann":
        from alignq_amd.resnet_office import resnet50_dann
        config.args.train_batch_size = 28
        net = resnet50_dann(bits, bits).to(dev)
    else:
        from alignq_amd.resnet import PreActBlock_conv_Q, PreActResNet
        config.args.train_batch_size = 128
        net = PreActResNet(PreActBlock_conv_Q, units, bits, bits, "second", 10, tree=kind).to(dev)
    net = net.to(memory_format=torch.channels_last)
    for m in net.modules():
        if hasattr(m, "quantize_fn"):
            m.use_qconv = True
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0.0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    return net.train()


def accuracy(output, target, topk=(1, 5)):
    """utils/common.py:78-92"""
    maxk = max(topk)
    _, pred = output.topk(maxk, 1, True, True)
    correct = pred.t().eq(target.view(1, -1).expand_as(pred.t()))
    return [correct[:k].reshape(-1).float().sum(0).mul_(100.0 / target.size(0)) for k in topk]


def run_baseline(net, kind, xs, ys, n):
    net.eval()
    loss = p1 = p5 = 0.0
    with torch.no_grad():
        for i in range(n):
            x, y = xs[i % len(xs)], ys[i % len(ys)]
            out = net(x, 0.0)[0] if kind == "dann" else net(x)
            out = out[0] if isinstance(out, tuple) else out
            loss += F.cross_entropy(out, y).item()
            a1, a5 = accuracy(out, y)
            p1 += a1.item()
            p5 += a5.item()
    net.train()
    return loss / n, p1 / n, p5 / n


def run_eval_step(ev, xs, ys, n, captured):
    with ev:
        if captured and ev._graph is None:
            ev.capture(xs[0], ys[0], warmup=1)
        for i in range(n):
            ev(xs[i % len(xs)], ys[i % len(ys)])
        return ev.result()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"batches": a.batches, "rounds": a.rounds, "configs": {}}
    for name in a.configs.split(","):
        kind, units, bits, batch, classes, side = CONFIGS[name]
        net = build(kind, units, bits, dev)
        xs = [torch.randn(batch, 3, side, side, device=dev).contiguous(memory_format=torch.channels_last) for _ in range(4)]
        ys = [torch.randint(0, classes, (batch,), device=dev) for _ in range(4)]
        ev_e, ev_c = EvalStep(net), EvalStep(net)
        paths = {"model_eval": lambda: run_baseline(net, kind, xs, ys, a.batches),
                 "eval_step_eager": lambda: run_eval_step(ev_e, xs, ys, a.batches, False),
                 "eval_step_captured": lambda: run_eval_step(ev_c, xs, ys, a.batches, True)}
        for f in paths.values():          # warm-up round (plans, allocator pools, the capture itself), not timed
            f()
        times = {k: [] for k in paths}
        results = {}
        for _ in range(a.rounds):
            for k, f in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                results[k] = f()
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
        n_img = a.batches * batch
        rec = {k: {"images_per_s": n_img / statistics.median(v), "best_images_per_s": n_img / min(v)} for k, v in times.items()}
        base = rec["model_eval"]["images_per_s"]
        rec["speedup_eager"] = rec["eval_step_eager"]["images_per_s"] / base
        rec["speedup_captured"] = rec["eval_step_captured"]["images_per_s"] / base
        rec["prec1"] = {k: float(v[1]) for k, v in results.items()}
        rec["batch"], rec["bits"] = batch, bits
        out["configs"][name] = rec
        del net, ev_e, ev_c, xs, ys
        torch.cuda.empty_cache()
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = 128
    print(json.dumps(out))


if __name__ == "__main__":
    main()
