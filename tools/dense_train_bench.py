#!/usr/bin/env python
"""DenseNet-40 training without concatenations (`fuse_dense_train`: fused.DenseBlockFn on alignq_dense_train_*) against the paths it
replaces, in one visit.

  iteration  one whole eager densenet_40_quant training iteration (forward, cross-entropy, backward, SGD step) under
             use_hip_convs(model), the same with train_sites=True and the same with dense_train=True, run alternately, host clock to a
             synchronise; and torch.cuda.max_memory_allocated over one iteration of each (peak statistics reset in front of it)
  layers     every dense layer of the model as a block of ONE layer: the module under `fuse_train_sites` (BNQuantAnyFn, QConvK3Fn and
             the `cat`) against DenseBlockFn (the buffer, the copy of the input, launches (1) and (2); backward the copy of the gradient
             and launches (3) to (5)), forward and backward timed separately with device events around each eager call (an eager
             iteration's launch overheads included); the two forms alternate inside every round, the median over the rounds is kept

    python tools/dense_train_bench.py --out profiles/dense_train_bench.json
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
from alignq_amd import config, densenet, fused, paths  # noqa: E402
from alignq_amd.optimizer import SGD  # noqa: E402

CONFIGS = {"hip_convs": {}, "train_sites": {"train_sites": True}, "dense_train": {"dense_train": True}}


def bench_iteration(a, dev, res, dump):
    models = {}
    for name, kw in CONFIGS.items():
        torch.manual_seed(0)
        net = densenet.use_hip_convs(densenet.densenet_40_quant(a.bits, a.bits, "no_align").to(dev), **kw)
        models[name] = (net.train(), SGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=2e-4))
    gen = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(a.batch, 3, 32, 32, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)
    tgt = torch.randint(0, 10, (a.batch,), generator=gen).to(dev)

    def iteration(net, opt):
        opt.zero_grad()
        loss = F.cross_entropy(net(x), tgt)
        loss.backward()
        opt.step([], [], [], 1.0, 4.0)
        return loss
    times, first, peak = {k: [] for k in models}, {}, {}
    for k, (net, opt) in models.items():
        first[k] = float(iteration(net, opt))
        for _ in range(a.warmup):
            iteration(net, opt)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        iteration(net, opt)
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated(), held)
    for _ in range(a.rounds):
        for k, (net, opt) in models.items():
            t0 = time.perf_counter()
            for _ in range(a.iters):
                loss = iteration(net, opt)
            torch.cuda.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t0) / a.iters)
            assert bool(torch.isfinite(loss))
    res["iteration"] = {k: {"ms": round(statistics.median(v), 3), "ms_range": [round(min(v), 3), round(max(v), 3)],
                            "first_loss": first[k], "peak_MiB": round(peak[k][0] / 2 ** 20, 1),
                            "held_before_MiB": round(peak[k][1] / 2 ** 20, 1)} for k, v in times.items()}
    res["iteration"]["what"] = ("densenet_40_quant, eager forward + cross-entropy + backward + SGD step, host clock to a synchronise; "
                                "peak = torch.cuda.max_memory_allocated over one iteration, all three models resident")
    print(json.dumps(res["iteration"]), flush=True)
    dump()


def bench_layers(a, dev, res, dump):
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    c, side = 24, 32
    for stage in range(3):
        for i in range(12):
            cin = c + 12 * i
            torch.manual_seed(cin)
            block = torch.nn.Sequential(densenet.DenseBasicBlock("no_align", a.bits, a.bits, inplanes=cin, filters=cin, index=None))
            block = densenet.use_hip_convs(block.to(dev).train())
            paths.apply(block, fuse_train_sites=True)
            x = torch.randn(a.batch, cin, side, side, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            g = torch.randn(a.batch, cin + 12, side, side, device=dev).contiguous(memory_format=torch.channels_last)
            forms = {"train_sites": lambda: block(x), "dense_train": lambda: fused.dense_block_train(block, x)}
            assert forms["dense_train"]() is not None
            t = {k: {"fwd": [], "bwd": []} for k in forms}
            for rnd in range(a.warmup + a.rounds):
                for k, fn in forms.items():
                    fw = bw = 0.0
                    marks = []
                    for _ in range(a.reps):
                        e = (ev(), ev(), ev())
                        e[0].record(); y = fn(); e[1].record(); y.backward(g); e[2].record()
                        x.grad = None
                        block.zero_grad(set_to_none=True)
                        marks.append(e)
                    torch.cuda.synchronize()
                    for e in marks:
                        fw += e[0].elapsed_time(e[1]); bw += e[1].elapsed_time(e[2])
                    if rnd >= a.warmup:
                        t[k]["fwd"].append(1e3 * fw / a.reps); t[k]["bwd"].append(1e3 * bw / a.reps)
            row = {"P": a.batch * side * side, "CIN": cin, "COUT": 12}
            for k in forms:
                for d in ("fwd", "bwd"):
                    row[f"{k}_{d}_us"] = round(statistics.median(t[k][d]), 1)
                    row[f"{k}_{d}_us_range"] = [round(min(t[k][d]), 1), round(max(t[k][d]), 1)]
            row["fwd_ratio"] = round(row["train_sites_fwd_us"] / row["dense_train_fwd_us"], 2)
            row["bwd_ratio"] = round(row["train_sites_bwd_us"] / row["dense_train_bwd_us"], 2)
            res["layers"].append(row)
            print(json.dumps(row), flush=True)
            dump()
        c, side = c + 144, side // 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="eager calls per layer, form and round")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_train_bench: needs the GPU (no number is produced without one)")
    dev = torch.device("cuda:0")
    config.args.bitW = config.args.abitW = a.bits
    res = {"batch": a.batch, "bits": a.bits, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0), "layers": []}

    def dump():          # after every row: a run that is cut short leaves what it measured
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    bench_iteration(a, dev, res, dump)
    bench_layers(a, dev, res, dump)


if __name__ == "__main__":
    main()
