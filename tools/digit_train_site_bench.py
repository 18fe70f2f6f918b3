#!/usr/bin/env python3
"""The digit DANN's two training sites at a batch of 64 (z of 64 x 32 x 24 x 24 and 64 x 48 x 8 x 8), forward + backward:
  composition  nn.BatchNorm2d (MIOpen) -> act_q -> [Dropout2d ->] ReLU -> MaxPool2d(2), what `feature` runs without the flag;
  fused        fused.bn_act_pool [-> Dropout2d on the pooled tensor] (include/alignq_bnq_pool.h, three launches each way).
Each form's forward + backward is captured as a graph of REPS repetitions; the two graphs of a site are replayed alternately, device
events around every 40 replays, median and range of the rounds in microseconds per forward + backward (digit_conv_bench.py's method).
Then one whole eager digit.train_iteration with digit.use_hip_convs(model) and with train_sites=True, run alternately, a host clock
around `--iters` iterations that end in a device synchronise.

    python tools/digit_train_site_bench.py --out profiles/digit_train_site_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import alignq_amd.cdf_alignment as A  # noqa: E402
from alignq_amd import config, digit, fused  # noqa: E402
from alignq_amd.optimizer import SGD  # noqa: E402
from digit_conv_bench import REPLAYS, REPS, graph_of, time_graphs  # noqa: E402

SITES = ((32, 24, False), (48, 8, True))          # (C, H, Dropout2d) of feature[1:5] and feature[6:11]


def bench_sites(a, dev, res):
    act = A.activation_quantize_fn(a_bit=a.bits, stage="second")
    for C, H, dropout in SITES:
        torch.manual_seed(C)
        bn = torch.nn.BatchNorm2d(C).to(dev).train()
        z = torch.randn(a.batch, C, H, H, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        g = torch.randn(a.batch, C, H // 2, H // 2, device=dev).contiguous(memory_format=torch.channels_last)
        drop = (lambda t: F.dropout2d(t, 0.5, True)) if dropout else (lambda t: t)
        forms = {"composition": lambda: F.max_pool2d(torch.relu(drop(act(bn(z)))), 2), "fused": lambda: drop(fused.bn_act_pool(bn, act, z))}
        assert fused.bn_act_pool(bn, act, z) is not None
        step = lambda fn: torch.autograd.grad(fn(), [z, bn.weight, bn.bias], g)      # noqa: E731
        t = time_graphs({k: graph_of(lambda fn=fn: step(fn)) for k, fn in forms.items()}, a.rounds)
        row = {"C": C, "H": H, "B": a.batch, "dropout2d": dropout}
        for k, v in t.items():
            row[f"{k}_us"], row[f"{k}_us_range"] = round(statistics.median(v), 2), [round(min(v), 2), round(max(v), 2)]
        row["composition_over_fused"] = round(row["composition_us"] / row["fused_us"], 2)
        res["sites"].append(row)
        print(json.dumps(row), flush=True)


def bench_iteration(a, dev, res):
    models = {}
    for name in ("flag_off", "flag_on"):
        torch.manual_seed(0)
        net = digit.use_hip_convs(digit.MNISTmodel_quant("second", a.bits, a.bits).to(dev), train_sites=name == "flag_on")
        models[name] = (net.train(), SGD(net.parameters(), lr=0.01, momentum=0.9))
    g = torch.Generator(device="cpu").manual_seed(1)
    src, tgt = torch.randn(a.batch, 1, 28, 28, generator=g).to(dev), torch.randn(a.batch, 3, 28, 28, generator=g).to(dev)
    labels = torch.randint(0, 10, (a.batch,), generator=g).to(dev)
    times = {k: [] for k in models}
    for net, opt in models.values():
        for _ in range(a.warmup):
            digit.train_iteration(net, opt, src, labels, tgt, 0.5)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, (net, opt) in models.items():
            t0 = time.perf_counter()
            for _ in range(a.iters):
                losses = digit.train_iteration(net, opt, src, labels, tgt, 0.5)
            torch.cuda.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t0) / a.iters)
            assert all(bool(torch.isfinite(v)) for v in losses)
    res["iteration"] = {k: {"ms": round(statistics.median(v), 3), "ms_range": [round(min(v), 3), round(max(v), 3)]} for k, v in times.items()}
    res["iteration"]["what"] = "eager source + target forward, three cross-entropies, backward, SGD step; host clock to a synchronise"
    print(json.dumps(res["iteration"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("digit_train_site_bench: needs the GPU (no number is produced without one)")
    dev = torch.device("cuda:0")
    config.args.bitW = config.args.abitW = a.bits
    res = {"batch": a.batch, "bits": a.bits, "rounds": a.rounds, "reps": REPS, "replays": REPLAYS, "device": torch.cuda.get_device_name(0),
           "sites": []}
    bench_iteration(a, dev, res)
    bench_sites(a, dev, res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
