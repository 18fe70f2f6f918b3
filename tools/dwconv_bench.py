#!/usr/bin/env python3
"""The depthwise 3x3 kernels (csrc/dwconv_kernels.hip) against what Conv2d_Q did before them, at every distinct depthwise
(C, H, stride) of mobile_v2 for 32x32 inputs at the reference's batch of 100 (utils/options.py:60).

Per shape, forward + data gradient + filter gradient two ways on the same channels-last tensors:
  hip   ops.QConvDwFn and torch.autograd.grad through it;
  base  F.conv2d(..., groups=C) and torch.autograd.grad through it (MIOpen: the path Conv2d_Q took for groups != 1).
Both paths are warmed, timed with device events over `--reps` calls, and ALTERNATE inside one process for `--rounds` rounds, so that
the baseline's own spread (max - min over the rounds) is known.  `verdict` is "slower" where the hip median exceeds the base median
by more than that spread: such a shape has to leave alignq_dwconv3x3_supported.

Per launch (the three exports called directly) the algorithmic bytes over time: one read of the input, one write of the output, the
filter, and for the filter gradient both reads.  This is bytes/s of the launch, NOT a share of the HBM peak: most of these tensors
fit the 256 MiB memory-side cache.

    python tools/dwconv_bench.py --out profiles/dwconv_bench.json
"""
import argparse
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


def shapes(side=32):
    """distinct (C, H, stride) of the depthwise convolutions, in network order"""
    out, in_planes, H = [], 32, side
    for expansion, out_planes, num_blocks, stride in MobileNetV2.cfg:
        for s in [stride] + [1] * (num_blocks - 1):
            key = (expansion * in_planes, H, s)
            if key not in out:
                out.append(key)
            in_planes, H = out_planes, (H - 1) // s + 1
    return out


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per call


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = L.load()
    cl = torch.channels_last
    g = torch.Generator(device="cpu").manual_seed(0)
    res = {"batch": a.batch, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0), "shapes": []}
    for C, H, s in shapes():
        B, Ho = a.batch, (H - 1) // s + 1
        assert lib.alignq_dwconv3x3_supported(B, H, H, C, s) == 1, (C, H, s)
        # what the layers see: ReLU6 of 4-bit activation levels, 4-bit filter levels
        x = torch.clamp((2.0 * torch.randint(0, 16, (B, C, H, H), generator=g) / 15.0 - 1.0) * 2.0, 0.0, 6.0)
        x = x.to(dev).contiguous(memory_format=cl).requires_grad_(True)
        w = (2.0 * torch.randint(0, 16, (C, 1, 3, 3), generator=g) / 15.0 - 1.0).to(dev).requires_grad_(True)
        dy = torch.randn(B, C, Ho, Ho, generator=g).to(dev).contiguous(memory_format=cl)

        def hip():
            torch.autograd.grad(ops.QConvDwFn.apply(x, w, s), (x, w), dy)

        def base():
            torch.autograd.grad(F.conv2d(x, w, None, s, 1, 1, C), (x, w), dy)

        for _ in range(a.warmup):
            hip()
            base()
        torch.cuda.synchronize()
        t_hip, t_base = [], []
        for _ in range(a.rounds):
            t_hip.append(timed(hip, a.reps))
            t_base.append(timed(base, a.reps))
        # the three launches alone
        xd, yd, dx, dw = x.detach(), torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
        ws = torch.empty(int(lib.alignq_dwconv3x3_wgrad_ws_bytes(B, H, H, C, s)), dtype=torch.uint8, device=dev)
        tail = (B, H, H, C, s)
        launches = {
            "fwd": lambda: lib.alignq_dwconv3x3_nhwc_fwd(xd.data_ptr(), w.data_ptr(), yd.data_ptr(), *tail, L.stream_ptr()),
            "dgrad": lambda: lib.alignq_dwconv3x3_nhwc_dgrad(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), *tail, L.stream_ptr()),
            "wgrad": lambda: lib.alignq_dwconv3x3_nhwc_wgrad(xd.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), *tail,
                                                             L.stream_ptr()),
        }
        nbytes = {"fwd": 4 * (x.numel() + dy.numel() + w.numel()), "dgrad": 4 * (x.numel() + dy.numel() + w.numel()),
                  "wgrad": 4 * (x.numel() + dy.numel() + w.numel())}
        per = {}
        for name, fn in launches.items():
            for _ in range(a.warmup):
                assert fn() == 0
            us = [timed(fn, a.reps) for _ in range(a.rounds)]
            per[name] = {"us": summary(us), "algorithmic_bytes": nbytes[name],
                         "bytes_per_s": nbytes[name] / (statistics.median(us) * 1e-6)}
        hs, bs = summary(t_hip), summary(t_base)
        spread = bs["max"] - bs["min"]
        row = {"C": C, "H": H, "stride": s, "hip_us": hs, "base_us": bs, "base_spread_us": spread,
               "hip_over_base": hs["median"] / bs["median"],
               "verdict": "slower" if hs["median"] > bs["median"] + spread else "not slower", "launches": per}
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
