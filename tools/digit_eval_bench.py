#!/usr/bin/env python
"""The digit DANN (MNISTmodel_quant, 28 x 28 one-channel images) evaluated at the reference's eval_batch_size = 100
(cdf_alignment/dann_digit/utils/options.py) through EvalStep, with `fuse_digit_eval` off and on, on the same commit.
Prints one JSON line; --out also writes it to a file.

    python tools/digit_eval_bench.py [--batches 2000] [--rounds 7] [--out profiles/digit_eval_bench.json]

Two paths timed in interleaved rounds in one process (median, best and worst round reported), each a captured EvalStep replayed
`batches` times between device synchronisations:
  composed   digit.use_hip_convs(model): per half of `feature` alignq_k5conv_fwd, batch-norm, quantiser, ReLU and MaxPool2d, the
             expanded channels-last copy of the image in front and the reshape-copy behind;
  fused      digit.use_hip_convs(model, eval_fused=True): one alignq_k5conv_site_pool_eval_fwd per half.
Per path also what one eager batch issues: the calls of this library's entry points and the ATen operators that launch work, counted as
tools/dense_eval_bench.py counts them.  The two paths' logits are compared before they are timed (reported, not asserted: the composed
path's sites are not the folded ones)."""
import argparse
import collections
import copy
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from alignq_amd import _lib as L  # noqa: E402
from alignq_amd import config, digit  # noqa: E402
from alignq_amd.eval_step import EvalStep  # noqa: E402
from dense_eval_bench import CountOps  # noqa: E402

BATCH, BITS = 100, 4


def build(dev):
    config.args.bitW = config.args.abitW = BITS
    torch.manual_seed(0)
    net = digit.MNISTmodel_quant("org", BITS, BITS).to(dev)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
                m.running_mean.normal_(0.0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    return net.train()


def count_one_batch(ev, x, y):
    """{entry point or ATen operator: calls} of one eager batch"""
    lib = L.load()
    names = [n for t in ("SIGNATURES", "MOBILE_SIGNATURES", "K5CONV_SIGNATURES", "DIGIT_SIGNATURES") for n in getattr(L, t)]
    calls, saved = collections.Counter(), {n: getattr(lib, n) for n in names}
    for n in names:
        def wrapper(*a, _orig=saved[n], _n=n):
            calls[_n] += 1
            return _orig(*a)
        setattr(lib, n, wrapper)
    try:
        with ev:
            calls.clear()          # (begin() quantises the filters once per evaluation: not part of a batch)
            with CountOps() as mode:
                ev._eager_fallback(x, y)
            torch.cuda.synchronize()
    finally:
        for n, f in saved.items():
            setattr(lib, n, f)
    entry = {k: v for k, v in calls.items()
             if (k.endswith(("_fwd", "_metrics")) or "conv" in k) and not k.endswith(("_supported", "_form", "_bytes"))}
    return {"entry_points": dict(entry), "aten": dict(mode.ops), "launches": sum(entry.values()) + sum(mode.ops.values())}


def run_eval_step(ev, xs, ys, n):
    with ev:
        if ev._graph is None:
            ev.capture(xs[0], ys[0], warmup=1)
        for i in range(n):
            ev(xs[i % len(xs)], ys[i % len(ys)])
        return ev.result()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("digit_eval_bench: needs the GPU (no number is produced without one)")
    dev = torch.device("cuda:0")
    old = (config.args.bitW, config.args.abitW)
    try:
        base = build(dev)
        nets = {"composed": digit.use_hip_convs(copy.deepcopy(base)), "fused": digit.use_hip_convs(copy.deepcopy(base), eval_fused=True)}
        xs = [torch.randn(BATCH, 1, 28, 28, device=dev) for _ in range(4)]
        ys = [torch.randint(0, 10, (BATCH,), device=dev) for _ in range(4)]
        counts = {k: count_one_batch(EvalStep(net), xs[0], ys[0]) for k, net in nets.items()}
        evs = {k: EvalStep(net) for k, net in nets.items()}
        logits = {}
        for k, ev in evs.items():          # warm-up round (plans, allocator pools, the captures), not timed
            run_eval_step(ev, xs, ys, 8)
            with ev:
                logits[k] = ev(xs[0], ys[0]).clone()
        times = {k: [] for k in evs}
        for _ in range(a.rounds):
            for k, ev in evs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_eval_step(ev, xs, ys, a.batches)
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
    finally:
        config.args.bitW, config.args.abitW = old
    out = {k: {"us_per_batch": 1e6 * statistics.median(v) / a.batches, "best_us_per_batch": 1e6 * min(v) / a.batches,
               "worst_us_per_batch": 1e6 * max(v) / a.batches, "images_per_s": a.batches * BATCH / statistics.median(v),
               "one_batch": counts[k]} for k, v in times.items()}
    out["composed_over_fused"] = out["composed"]["us_per_batch"] / out["fused"]["us_per_batch"]
    out["max_abs_logit_difference"] = float((logits["composed"] - logits["fused"]).abs().max())
    out["max_abs_logit"] = float(logits["composed"].abs().max())
    out["batch"], out["bits"], out["batches"], out["rounds"] = BATCH, BITS, a.batches, a.rounds
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
