#!/usr/bin/env python
"""Training-mode quantiser sites at any width: the folded chain (fused.BNQuantAnyFn: alignq_bnq_any_fwd / _bwd, three launches each way)
against the composition the models run without `fuse_train_sites` (nn.BatchNorm2d on MIOpen, ActQuantFn, a separate ReLU / ReLU6).

  sites      every distinct (P, C, clamp) of MobileNet-V2 and DenseNet-40 at the given batch on 32 x 32 inputs, forward and backward timed
             separately with device events around each eager call (launch overheads of an eager iteration included: this is what a
             training iteration pays, not a kernel time); the two forms alternate inside every round, the median over the rounds is kept
  iteration  one whole eager DenseNet-40 training iteration (forward, cross-entropy, backward, SGD step) with the flag off and on, run
             alternately, host clock to a synchronise.  MobileNet-V2 has no such flag: its sites are timed above, its iteration is not.

    python tools/train_site_bench.py --out profiles/train_site_bench.json
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
from alignq_amd import config, densenet, fused, mobilenet  # noqa: E402
from alignq_amd.optimizer import SGD  # noqa: E402

CLAMP_NAME = {fused.CLAMP_NONE: "none", fused.CLAMP_RELU: "relu", fused.CLAMP_RELU6: "relu6"}


def mobilenet_sites(batch, side=32):
    """(P, C, clamp) of every site of mobilenet.MobileNetV2 in forward order"""
    out, s, cin = [(batch * side * side, 32, fused.CLAMP_RELU)], side, 32
    for expansion, cout, blocks, stride in mobilenet.MobileNetV2.cfg:
        for st in [stride] + [1] * (blocks - 1):
            planes = expansion * cin
            out.append((batch * s * s, planes, fused.CLAMP_RELU6))
            s = (s - 1) // st + 1
            out.append((batch * s * s, planes, fused.CLAMP_RELU6))
            out.append((batch * s * s, cout, fused.CLAMP_NONE))
            if st == 1:
                out.append((batch * s * s, cout, fused.CLAMP_RELU))
            cin = cout
    return out + [(batch * s * s, 1280, fused.CLAMP_RELU)]


def densenet_sites(batch, side=32, growth=12, n=12):
    """(P, C, clamp) of every site of densenet_40_quant: n dense layers per stage, then the transition's (or the head's) site"""
    out, c, s = [], 2 * growth, side
    for stage in range(3):
        out += [(batch * s * s, c + growth * i, fused.CLAMP_RELU) for i in range(n + 1)]
        c += growth * n
        s //= 2 if stage < 2 else 1
    return out


def bench_sites(a, dev, res, dump):
    sites = {}
    for model, lst in (("mobilenet_v2", mobilenet_sites(a.batch)), ("densenet_40", densenet_sites(a.batch))):
        for key in lst:
            sites.setdefault(key, {"models": set(), "count": 0})
            sites[key]["models"].add(model)
            sites[key]["count"] += 1
    act = A.activation_quantize_fn(a_bit=a.bits, stage="no_align")
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    for (P, C, clamp), info in sorted(sites.items(), key=lambda kv: (kv[0][1], -kv[0][0], kv[0][2])):
        side = 32
        while a.batch * side * side > P:
            side //= 2
        torch.manual_seed(C)
        bn = torch.nn.BatchNorm2d(C).to(dev).train()
        z = torch.randn(a.batch, C, side, side, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        g = torch.randn_like(z)
        tail = {fused.CLAMP_NONE: lambda t: t, fused.CLAMP_RELU: torch.relu, fused.CLAMP_RELU6: F.relu6}[clamp]
        forms = {"composition": lambda: tail(act(bn(z))), "folded": lambda: fused.bn_act_any(bn, act, z, clamp)}
        assert forms["folded"]() is not None
        t = {k: {"fwd": [], "bwd": []} for k in forms}
        for rnd in range(a.warmup + a.rounds):
            for k, fn in forms.items():
                fw = bw = 0.0
                marks = []
                for _ in range(a.reps):
                    e = (ev(), ev(), ev())
                    e[0].record(); y = fn(); e[1].record(); y.backward(g); e[2].record()
                    z.grad = None
                    marks.append(e)
                torch.cuda.synchronize()
                for e in marks:
                    fw += e[0].elapsed_time(e[1]); bw += e[1].elapsed_time(e[2])
                if rnd >= a.warmup:
                    t[k]["fwd"].append(1e3 * fw / a.reps); t[k]["bwd"].append(1e3 * bw / a.reps)
        row = {"P": P, "C": C, "clamp": CLAMP_NAME[clamp], "models": sorted(info["models"]), "sites": info["count"],
               "MB": round(P * C * 4 / 2 ** 20, 2)}
        for k in forms:
            for d in ("fwd", "bwd"):
                row[f"{k}_{d}_us"] = round(statistics.median(t[k][d]), 1)
                row[f"{k}_{d}_us_range"] = [round(min(t[k][d]), 1), round(max(t[k][d]), 1)]
        row["fwd_ratio"] = round(row["composition_fwd_us"] / row["folded_fwd_us"], 2)
        row["bwd_ratio"] = round(row["composition_bwd_us"] / row["folded_bwd_us"], 2)
        res["sites"].append(row)
        print(json.dumps(row), flush=True)
        dump()


def bench_iteration(a, dev, res, dump):
    models = {}
    for name in ("flag_off", "flag_on"):
        torch.manual_seed(0)
        net = densenet.use_hip_convs(densenet.densenet_40_quant(a.bits, a.bits, "no_align").to(dev), train_sites=name == "flag_on")
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
    times, first = {k: [] for k in models}, {}
    for k, (net, opt) in models.items():
        first[k] = float(iteration(net, opt))
        for _ in range(a.warmup):
            iteration(net, opt)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, (net, opt) in models.items():
            t0 = time.perf_counter()
            for _ in range(a.iters):
                loss = iteration(net, opt)
            torch.cuda.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t0) / a.iters)
            assert bool(torch.isfinite(loss))
    res["iteration"] = {k: {"ms": round(statistics.median(v), 3), "ms_range": [round(min(v), 3), round(max(v), 3)],
                            "first_loss": first[k]} for k, v in times.items()}
    res["iteration"]["what"] = "densenet_40_quant, eager forward + cross-entropy + backward + SGD step, host clock to a synchronise"
    print(json.dumps(res["iteration"]), flush=True)
    dump()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="eager calls per site, form and round")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_site_bench: needs the GPU (no number is produced without one)")
    dev = torch.device("cuda:0")
    config.args.bitW = config.args.abitW = a.bits
    res = {"batch": a.batch, "bits": a.bits, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0), "sites": []}

    def dump():          # after every row: a run that is cut short leaves what it measured
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    bench_iteration(a, dev, res, dump)
    bench_sites(a, dev, res, dump)


if __name__ == "__main__":
    main()
