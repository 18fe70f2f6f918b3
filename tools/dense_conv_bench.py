#!/usr/bin/env python3
"""The 3x3 kernels at any multiple of 4 channels (csrc/k3conv_kernels.hip) against what Conv2d_Q does without them, at every
distinct 3x3 dense-layer shape (C_in -> 12, H) of densenet_40_quant for 32x32 inputs at a batch of 128: C_in = 24 ... 156 at 32 x 32,
168 ... 300 at 16 x 16, 312 ... 444 at 8 x 8; and one whole eager training iteration of the model with the flag off and on.

Per shape and operation, two ways on the same channels-last tensors:
  hip   alignq_k3conv_fwd / _dgrad / _wgrad (the filter gradient with its slab reduction), the filter bins packed beforehand;
  base  F.conv2d / aten.convolution_backward with one output asked for (MIOpen, fp32).
Each is captured as a graph of REPS launches; the two graphs of an operation are replayed alternately for `--rounds` rounds after a
warm-up replay, device events around every five replays.  Median and range of the rounds, microseconds per launch.  `verdict` is
"slower" where the hip median exceeds the base median by more than the base's own range.  There is no decline list: the opt-in takes
every supported shape; the table says where that costs time.

The iteration: forward, cross-entropy, backward and the SGD step of densenet_40_quant at 4W/4A on one seeded batch, channels-last
parameters and `use_qconv` in both models, `use_qconv_pw` + `use_qconv_k3` (densenet.use_hip_convs) in one; the two are run alternately,
a host clock around `--iters` iterations that end in a device synchronise.

    python tools/dense_conv_bench.py --out profiles/dense_conv_bench.json
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
from alignq_amd import _lib as L  # noqa: E402
from alignq_amd import config, densenet, ops, paths  # noqa: E402
from alignq_amd.optimizer import SGD  # noqa: E402

REPS = 10


def shapes(side=32, depth=40, growth=12):
    """(C_in, C_out, H) of the dense layers in network order (compressionRate 1: a transition keeps the width)"""
    n, out, c, H = (depth - 4) // 3, [], 2 * growth, side
    for _ in range(3):
        for _ in range(n):
            out.append((c, growth, H))
            c += growth
        H //= 2
    return out


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    return g


def time_graphs(graphs, rounds):
    """{name: [microseconds per launch, one per round]}: the graphs replayed alternately, device events around five replays"""
    out = {k: [] for k in graphs}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                g.replay()
            e1.record()
            e1.synchronize()
            out[k].append(1e3 * e0.elapsed_time(e1) / (5 * REPS))
    return out


def bench_shapes(a, dev, res, dump):
    lib = L.load()
    cl = torch.channels_last
    g = torch.Generator(device="cpu").manual_seed(0)
    n = 2 ** a.bits - 1
    conv_args = (None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1)
    for cin, cout, H in shapes():
        B = a.batch
        geom = (B, H, H, cin, cout)
        assert lib.alignq_k3conv_supported(*geom) == 1, geom
        # what the layers see: ReLU of activation levels, quantised filter levels
        x = torch.clamp((2.0 * torch.randint(0, n + 1, (B, cin, H, H), generator=g) / n - 1.0) * 2.0, min=0.0).to(dev).contiguous(memory_format=cl)
        w = (torch.round(torch.tanh(torch.randn(cout, cin, 3, 3, generator=g)) * n) / n).to(dev).contiguous(memory_format=cl)
        dy = (torch.randn(B, cout, H, H, generator=g) * 1e-3).to(dev).contiguous(memory_format=cl)
        bins = ops.pack_filter_bins([w], a.bits)[0][0]
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
        ws = torch.empty(max(int(lib.alignq_k3conv_wgrad_ws_bytes(*geom)), 16), dtype=torch.uint8, device=dev)
        hip = {
            "fwd": lambda: L.check(lib.alignq_k3conv_fwd(L.ptr(x), L.ptr(bins), L.ptr(y), *geom, a.bits, L.stream_ptr()), "fwd"),
            "dgrad": lambda: L.check(lib.alignq_k3conv_dgrad(L.ptr(dy), L.ptr(bins), L.ptr(dx), *geom, a.bits, L.stream_ptr()), "dgrad"),
            "wgrad": lambda: L.check(lib.alignq_k3conv_wgrad(L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(ws), *geom, None, L.stream_ptr()), "wgrad"),
        }
        base = {
            "fwd": lambda: F.conv2d(x, w, None, 1, 1),
            "dgrad": lambda: torch.ops.aten.convolution_backward(dy, x, w, *conv_args, (True, False, False)),
            "wgrad": lambda: torch.ops.aten.convolution_backward(dy, x, w, *conv_args, (False, True, False)),
        }
        nbytes = {"fwd": 4 * (x.numel() + y.numel()) + 2 * w.numel(), "dgrad": 4 * (x.numel() + y.numel()) + 2 * w.numel(),
                  "wgrad": 4 * (x.numel() + y.numel() + w.numel())}
        row = {"CIN": cin, "COUT": cout, "H": H, "B": B, "n_slabs": int(len(ws) // (4 * 9 * cin * cout)), "ops": {}}
        for i, op in enumerate(("fwd", "dgrad", "wgrad")):
            t = time_graphs({"hip": graph_of(hip[op]), "base": graph_of(base[op])}, a.rounds)
            hm, bm = statistics.median(t["hip"]), statistics.median(t["base"])
            spread = max(t["base"]) - min(t["base"])
            row["ops"][op] = {"form": lib.alignq_k3conv_form(i, *geom),
                              "hip_us": hm, "hip_us_range": [min(t["hip"]), max(t["hip"])],
                              "base_us": bm, "base_us_range": [min(t["base"]), max(t["base"])],
                              "hip_over_base": hm / bm, "verdict": "slower" if hm > bm + spread else "not slower",
                              "algorithmic_bytes": nbytes[op], "hip_bytes_per_s": nbytes[op] / (hm * 1e-6)}
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
        dump()


def bench_iteration(a, dev, res, dump):
    config.args.bitW = config.args.abitW = a.bits
    cl = torch.channels_last
    models = {}
    for name in ("flag_off", "flag_on"):
        torch.manual_seed(0)
        net = densenet.densenet_40_quant(a.bits, a.bits, "no_align").to(dev)
        if name == "flag_on":
            net = densenet.use_hip_convs(net)
        else:
            net = net.to(memory_format=cl)
            paths.apply(net, use_qconv=True)
        models[name] = (net.train(), SGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=2e-4))
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(a.batch, 3, 32, 32, generator=g).to(dev).contiguous(memory_format=cl)
    t = torch.randint(0, 10, (a.batch,), generator=g).to(dev)

    def iteration(net, opt):
        opt.zero_grad()
        loss = F.cross_entropy(net(x), t)
        loss.backward()
        opt.step([], [], [], 1.0, 4.0)
        return loss
    times = {k: [] for k in models}
    for k, (net, opt) in models.items():
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
    res["iteration"] = {k: {"ms": statistics.median(v), "ms_range": [min(v), max(v)]} for k, v in times.items()}
    res["iteration"].update({"iters": a.iters, "warmup": a.warmup, "what": "eager forward + backward + SGD step, host clock to a synchronise"})
    print(json.dumps(res["iteration"]), flush=True)
    dump()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_conv_bench: needs the GPU (no number is produced without one)")
    dev = torch.device("cuda:0")
    res = {"batch": a.batch, "bits": a.bits, "rounds": a.rounds, "reps": REPS, "device": torch.cuda.get_device_name(0), "shapes": []}

    def dump():          # after every row: a run that is cut short leaves what it measured
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    bench_iteration(a, dev, res, dump)
    bench_shapes(a, dev, res, dump)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
