#!/usr/bin/env python3
"""The pointwise kernels (csrc/pointwise_kernels.hip) against what Conv2d_Q does without them, at every distinct 1x1 convolution
(C_in, C_out, H) of mobile_v2 for 32x32 inputs at the reference's batch of 100 that mobilenet.use_hip_convs(model, pointwise=True)
moves: the layers whose channel counts are not both multiples of 64 (those stay on alignq_qconv_*).

Per shape and operation, two ways on the same channels-last tensors:
  hip   alignq_pwconv_fwd / _dgrad / _wgrad (the filter gradient with its slab reduction), the filter bins packed beforehand;
  base  F.conv2d / aten.convolution_backward with one output asked for (MIOpen, fp32).
`wgrad_slabs` is the filter gradient's first launch alone (the slabs; the deferred form a fused.DeferredWgrads context uses, which
reduces every layer's slabs in one launch at the end of the backward), against the same base.
Each is captured as a graph of REPS launches; the two graphs of an operation are replayed alternately for `--rounds` rounds after a
warm-up replay, device events around every five replays.  Median and range of the rounds, microseconds per launch.  `verdict` is
"slower" where the hip median exceeds the base median by more than the base's own range.  There is no decline list: the opt-in takes
every supported shape; the table says where that costs time.

    python tools/pointwise_bench.py --out profiles/pointwise_bench.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alignq_amd import _lib as L  # noqa: E402
from alignq_amd import ops  # noqa: E402
from alignq_amd.mobilenet import MobileNetV2  # noqa: E402

REPS = 20


def shapes(side=32):
    """distinct (C_in, C_out, H) of the 1x1 convolutions the opt-in moves, in network order"""
    out, in_planes, H = [], 32, side
    for expansion, out_planes, num_blocks, stride in MobileNetV2.cfg:
        for s in [stride] + [1] * (num_blocks - 1):
            planes, Ho = expansion * in_planes, (H - 1) // s + 1
            layer = [(in_planes, planes, H), (planes, out_planes, Ho)] + ([(in_planes, out_planes, H)] if s == 1 else [])
            for key in layer:
                if (key[0] % 64 or key[1] % 64) and key not in out:
                    out.append(key)
            in_planes, H = out_planes, Ho
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointwise_bench: needs the GPU (no number is produced without one)")
    dev = torch.device("cuda:0")
    lib = L.load()
    cl = torch.channels_last
    g = torch.Generator(device="cpu").manual_seed(0)
    n = 2 ** a.bits - 1
    res = {"batch": a.batch, "bits": a.bits, "rounds": a.rounds, "reps": REPS, "device": torch.cuda.get_device_name(0), "shapes": []}
    conv_args = (None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1)
    for cin, cout, H in shapes():
        B, M = a.batch, a.batch * H * H
        assert lib.alignq_pwconv_supported(M, cin, cout) == 1, (cin, cout, H)
        # what the layers see: ReLU6 of activation levels (or a sum of two), quantised filter levels
        x = torch.clamp((2.0 * torch.randint(0, n + 1, (B, cin, H, H), generator=g) / n - 1.0) * 2.0, 0.0, 6.0).to(dev).contiguous(memory_format=cl)
        w = (torch.round(torch.tanh(torch.randn(cout, cin, 1, 1, generator=g)) * n) / n).to(dev).contiguous(memory_format=cl)
        dy = (torch.randn(B, cout, H, H, generator=g) * 1e-3).to(dev).contiguous(memory_format=cl)
        bins = ops.pack_filter_bins([w], a.bits)[0][0]
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
        ws = torch.empty(max(int(lib.alignq_pwconv_wgrad_ws_bytes(M, cin, cout)), 16), dtype=torch.uint8, device=dev)
        hip = {
            "fwd": lambda: L.check(lib.alignq_pwconv_fwd(L.ptr(x), L.ptr(bins), L.ptr(y), M, cin, cout, a.bits, L.stream_ptr()), "fwd"),
            "dgrad": lambda: L.check(lib.alignq_pwconv_dgrad(L.ptr(dy), L.ptr(bins), L.ptr(dx), M, cin, cout, a.bits, L.stream_ptr()), "dgrad"),
            "wgrad": lambda: L.check(lib.alignq_pwconv_wgrad(L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(ws), M, cin, cout, None, L.stream_ptr()), "wgrad"),
        }
        base = {
            "fwd": lambda: F.conv2d(x, w),
            "dgrad": lambda: torch.ops.aten.convolution_backward(dy, x, w, *conv_args, (True, False, False)),
            "wgrad": lambda: torch.ops.aten.convolution_backward(dy, x, w, *conv_args, (False, True, False)),
        }
        nbytes = {"fwd": 4 * (x.numel() + y.numel()) + 2 * w.numel(), "dgrad": 4 * (x.numel() + y.numel()) + 2 * w.numel(),
                  "wgrad": 4 * (x.numel() + y.numel() + w.numel())}
        row = {"CIN": cin, "COUT": cout, "H": H, "M": M, "ops": {}}
        ns = ctypes.c_int(0)
        hip["wgrad_slabs"] = lambda: L.check(lib.alignq_pwconv_wgrad(L.ptr(x), L.ptr(dy), None, L.ptr(ws), M, cin, cout, ctypes.byref(ns),
                                                                    L.stream_ptr()), "wgrad")
        base["wgrad_slabs"] = base["wgrad"]
        nbytes["wgrad_slabs"] = nbytes["wgrad"]
        for op in ("fwd", "dgrad", "wgrad", "wgrad_slabs"):
            t = time_graphs({"hip": graph_of(hip[op]), "base": graph_of(base[op])}, a.rounds)
            hm, bm = statistics.median(t["hip"]), statistics.median(t["base"])
            spread = max(t["base"]) - min(t["base"])
            row["ops"][op] = {"form": lib.alignq_pwconv_form({"fwd": 0, "dgrad": 1, "wgrad": 2, "wgrad_slabs": 2}[op], M, cin, cout),
                              "hip_us": hm, "hip_us_range": [min(t["hip"]), max(t["hip"])],
                              "base_us": bm, "base_us_range": [min(t["base"]), max(t["base"])],
                              "hip_over_base": hm / bm, "verdict": "slower" if hm > bm + spread else "not slower",
                              "algorithmic_bytes": nbytes[op], "hip_bytes_per_s": nbytes[op] / (hm * 1e-6)}
        row["n_slabs"] = ns.value
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
