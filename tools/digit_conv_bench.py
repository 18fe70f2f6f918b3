#!/usr/bin/env python3
"""The 5x5 kernels (csrc/k5conv_kernels.hip) against what Conv2d_Q does without them, at the two layers of digit.MNISTmodel_quant for
28 x 28 inputs at a batch of 64: 3 -> 32 at 28 x 28 (image form: forward and filter gradient) and 32 -> 48 at 12 x 12 (body form: and
the data gradient); and one whole eager training iteration of the model (source batch + target batch) with the flags off and on.

Per layer and operation, two ways on the same channels-last tensors:
  hip   alignq_k5conv_fwd / _dgrad / _wgrad (the filter gradient with its slab reduction), the filter bins packed beforehand;
  base  F.conv2d with the bias / aten.convolution_backward with one output asked for (MIOpen, fp32).
Each is captured as a graph of REPS launches; the two graphs of an operation are replayed alternately for `--rounds` rounds after a
warm-up replay, device events around every 40 replays (400 launches: milliseconds per window).  Both sides' tensors stay resident in
cache across replays.  Median and range of the rounds, microseconds per launch.  `verdict` is
"slower" where the hip median exceeds the base median by more than the base's own range.  These layers are small (0.2 and 0.3 GFLOP
forward): a launch's fixed cost is a large share of every figure.

The iteration: digit.train_iteration at 4W/4A on one seeded pair of batches, flags off in one model (NCHW, every convolution on
MIOpen), digit.use_hip_convs in the other; the two are run alternately, a host clock around `--iters` iterations that end in a device
synchronise.

    python tools/digit_conv_bench.py --out profiles/digit_conv_bench.json
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
from alignq_amd import config, digit, ops  # noqa: E402
from alignq_amd.optimizer import SGD  # noqa: E402

REPS = 10
REPLAYS = 40          # per timed window: 400 launches, 3 - 25 ms
LAYERS = ((3, 32, 28), (32, 48, 12))          # (C_in, C_out, H) of feature[0] and feature[5]


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    return g


def time_graphs(graphs, rounds):
    """{name: [microseconds per launch, one per round]}: the graphs replayed alternately, device events around REPLAYS replays"""
    out = {k: [] for k in graphs}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPLAYS):
                g.replay()
            e1.record()
            e1.synchronize()
            out[k].append(1e3 * e0.elapsed_time(e1) / (REPLAYS * REPS))
    return out


def bench_layers(a, dev, res, dump):
    lib = L.load()
    cl = torch.channels_last
    g = torch.Generator(device="cpu").manual_seed(0)
    n = 2 ** a.bits - 1
    conv_args = (None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1)
    for cin, cout, H in LAYERS:
        B = a.batch
        geom = (B, H, H, cin, cout)
        x = torch.randn(B, cin, H, H, generator=g).to(dev).contiguous(memory_format=cl)
        w = (torch.round(torch.tanh(torch.randn(cout, cin, 5, 5, generator=g)) * n) / n).to(dev).contiguous(memory_format=cl)
        bias = torch.randn(cout, generator=g).to(dev)
        dy = (torch.randn(B, cout, H - 4, H - 4, generator=g) * 1e-3).to(dev).contiguous(memory_format=cl)
        bins = ops.pack_filter_bins([w], a.bits)[0][0]
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
        ws = torch.empty(max(int(lib.alignq_k5conv_wgrad_ws_bytes(*geom)), 16), dtype=torch.uint8, device=dev)
        hip = {
            "fwd": lambda: L.check(lib.alignq_k5conv_fwd(L.ptr(x), L.ptr(bins), L.ptr(bias), L.ptr(y), *geom, a.bits, L.stream_ptr()), "fwd"),
            "dgrad": lambda: L.check(lib.alignq_k5conv_dgrad(L.ptr(dy), L.ptr(bins), L.ptr(dx), *geom, a.bits, L.stream_ptr()), "dgrad"),
            "wgrad": lambda: L.check(lib.alignq_k5conv_wgrad(L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(ws), *geom, None, L.stream_ptr()), "wgrad"),
        }
        base = {
            "fwd": lambda: F.conv2d(x, w, bias),
            "dgrad": lambda: torch.ops.aten.convolution_backward(dy, x, w, *conv_args, (True, False, False)),
            "wgrad": lambda: torch.ops.aten.convolution_backward(dy, x, w, *conv_args, (False, True, False)),
        }
        flop = 2 * B * (H - 4) ** 2 * cout * 25 * cin
        nbytes = {"fwd": 4 * (x.numel() + y.numel()) + 2 * w.numel(), "dgrad": 4 * (x.numel() + y.numel()) + 2 * w.numel(),
                  "wgrad": 4 * (x.numel() + y.numel() + w.numel())}
        row = {"CIN": cin, "COUT": cout, "H": H, "B": B, "flop": flop, "n_slabs": int(len(ws) // (4 * 25 * cin * cout)), "ops": {}}
        for i, op in enumerate(("fwd", "dgrad", "wgrad")):
            if lib.alignq_k5conv_supported(i, *geom) != 1:          # the image form has no data gradient (nor does the model ask for one)
                continue
            t = time_graphs({"hip": graph_of(hip[op]), "base": graph_of(base[op])}, a.rounds)
            hm, bm = statistics.median(t["hip"]), statistics.median(t["base"])
            spread = max(t["base"]) - min(t["base"])
            row["ops"][op] = {"form": lib.alignq_k5conv_form(i, *geom),
                              "hip_us": hm, "hip_us_range": [min(t["hip"]), max(t["hip"])],
                              "base_us": bm, "base_us_range": [min(t["base"]), max(t["base"])],
                              "hip_over_base": hm / bm, "verdict": "slower" if hm > bm + spread else "not slower",
                              "algorithmic_bytes": nbytes[op], "hip_flop_per_s": flop / (hm * 1e-6)}
        res["layers"].append(row)
        print(json.dumps(row), flush=True)
        dump()


def bench_iteration(a, dev, res, dump):
    config.args.bitW = config.args.abitW = a.bits
    models = {}
    for name in ("flags_off", "flags_on"):
        torch.manual_seed(0)
        net = digit.MNISTmodel_quant("org", a.bits, a.bits).to(dev)
        if name == "flags_on":
            net = digit.use_hip_convs(net)
        models[name] = (net.train(), SGD(net.parameters(), lr=0.01, momentum=0.9))
    g = torch.Generator(device="cpu").manual_seed(1)
    src, tgt = torch.randn(a.batch, 1, 28, 28, generator=g).to(dev), torch.randn(a.batch, 3, 28, 28, generator=g).to(dev)
    labels = torch.randint(0, 10, (a.batch,), generator=g).to(dev)
    times = {k: [] for k in models}
    for k, (net, opt) in models.items():
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
    res["iteration"] = {k: {"ms": statistics.median(v), "ms_range": [min(v), max(v)]} for k, v in times.items()}
    res["iteration"].update({"iters": a.iters, "warmup": a.warmup,
                             "what": "eager source + target forward, three cross-entropies, backward, SGD step; host clock to a synchronise"})
    print(json.dumps(res["iteration"]), flush=True)
    dump()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers-only", action="store_true", help="skip the training iteration (A/B builds through ALIGNQ_SO)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("digit_conv_bench: needs the GPU (no number is produced without one)")
    dev = torch.device("cuda:0")
    res = {"batch": a.batch, "bits": a.bits, "rounds": a.rounds, "reps": REPS, "replays": REPLAYS, "library": L.SO_PATH if os.environ.get("ALIGNQ_SO") else "product", "device": torch.cuda.get_device_name(0), "layers": []}

    def dump():          # after every row: a run that is cut short leaves what it measured
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    if not a.layers_only:
        bench_iteration(a, dev, res, dump)
    bench_layers(a, dev, res, dump)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
