#!/usr/bin/env python
"""MobileNet-V2 (SVHN, the full cfg) evaluation at eval_batch_size = 100: images/s of a whole evaluation (begin(), the batches,
result()) and, per depthwise shape of the network, the fused depthwise + site launch against the two launches it replaces.
Prints one JSON line; --out also writes it to a file.

    python tools/mobilenet_eval_bench.py [--batches 100] [--rounds 5] [--out profiles/mobilenet_eval_bench.json]

Whole evaluation, four paths timed in interleaved rounds in one process (median, best and the spread of the rounds reported):
  model_eval          the reference's test() on this repository's modules: eval mode, no_grad, channels-last, use_qconv,
                      F.cross_entropy + topk accuracy with their host reads per batch;
  eval_step_composed  captured EvalStep with every site the `model.eval()` composition - mobilenet.py's folded route switched off,
                      which is EvalStep(mobile_v2(...)) as it stood before the folded sites existed: the baseline;
  eval_step_folded    captured EvalStep with the folded sites (alignq_site_eval_fwd, alignq_site_eval_twin_fwd,
                      alignq_dwconv3x3_site_eval_fwd);
  eval_step_pointwise the same on a copy of the model with mobilenet.use_hip_convs(model, pointwise=True): the 1x1 convolutions whose
                      channel counts are no multiples of 64 on alignq_pwconv_fwd instead of MIOpen, their bins packed once in begin().
Per depthwise shape (C, H_in, stride) of the network at batch 100: a graph of REPS fused launches against a graph of REPS
(alignq_dwconv3x3_nhwc_fwd, alignq_site_eval_fwd) pairs, replayed alternately; microseconds per site."""
import argparse
import copy
import ctypes
import json
import os
import statistics
import sys
import time
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alignq_amd import _lib as L  # noqa: E402
from alignq_amd import config, fused  # noqa: E402
from alignq_amd import mobilenet as M  # noqa: E402
from alignq_amd.eval_step import EvalStep  # noqa: E402

BATCH, BITS, REPS = 100, 4, 20


def build(dev):
    config.args.bitW = config.args.abitW = BITS
    torch.manual_seed(0)
    net = M.use_hip_convs(M.mobile_v2(BITS, BITS, "no_align").to(dev))
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0.0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    return net.train()


def accuracy(output, target, topk=(1, 5)):
    """utils/common.py:84-98"""
    maxk = max(topk)
    _, pred = output.topk(maxk, 1, True, True)
    correct = pred.t().eq(target.view(1, -1).expand_as(pred.t()))
    return [correct[:k].reshape(-1).float().sum(0).mul_(100.0 / target.size(0)) for k in topk]


def run_model_eval(net, xs, ys, n):
    net.eval()
    loss = p1 = p5 = 0.0
    with torch.no_grad():
        for i in range(n):
            out = net(xs[i % len(xs)])
            y = ys[i % len(ys)]
            loss += F.cross_entropy(out, y).item()
            a1, a5 = accuracy(out, y)
            p1 += a1.item()
            p5 += a5.item()
    net.train()
    return loss / n, p1 / n, p5 / n


class composed_sites:
    """mobilenet.py sees eval_active() == False: both forwards take the module composition, the code path before the folded route"""

    def __enter__(self):
        self.saved = M.fused
        M.fused = types.SimpleNamespace(eval_active=lambda: False)

    def __exit__(self, *exc):
        M.fused = self.saved
        return False


def run_eval_step(ev, xs, ys, n, composed):
    with ev:
        if ev._graph is None:
            if composed:
                with composed_sites():
                    ev.capture(xs[0], ys[0], warmup=1)
            else:
                ev.capture(xs[0], ys[0], warmup=1)
        for i in range(n):
            ev(xs[i % len(xs)], ys[i % len(ys)])
        return ev.result()


def whole_evaluation(dev, batches, rounds):
    net = build(dev)
    xs = [torch.randn(BATCH, 3, 32, 32, device=dev).contiguous(memory_format=torch.channels_last) for _ in range(4)]
    ys = [torch.randint(0, 10, (BATCH,), device=dev) for _ in range(4)]
    ev_c, ev_f = EvalStep(net), EvalStep(net)
    ev_p = EvalStep(M.use_hip_convs(copy.deepcopy(net), pointwise=True))
    paths = {"model_eval": lambda: run_model_eval(net, xs, ys, batches),
             "eval_step_composed": lambda: run_eval_step(ev_c, xs, ys, batches, True),
             "eval_step_folded": lambda: run_eval_step(ev_f, xs, ys, batches, False),
             "eval_step_pointwise": lambda: run_eval_step(ev_p, xs, ys, batches, False)}
    for f in paths.values():          # warm-up round (plans, allocator pools, the captures), not timed
        f()
    times, results = {k: [] for k in paths}, {}
    for _ in range(rounds):
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[k] = f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    n_img = batches * BATCH
    rec = {k: {"images_per_s": n_img / statistics.median(v), "best_images_per_s": n_img / min(v),
               "worst_images_per_s": n_img / max(v), "ms_per_batch": 1e3 * statistics.median(v) / batches,
               "rounds_ms_per_batch": [1e3 * t / batches for t in v]} for k, v in times.items()}
    rec["folded_over_composed"] = rec["eval_step_folded"]["images_per_s"] / rec["eval_step_composed"]["images_per_s"]
    rec["folded_over_model_eval"] = rec["eval_step_folded"]["images_per_s"] / rec["model_eval"]["images_per_s"]
    rec["pointwise_over_folded"] = rec["eval_step_pointwise"]["images_per_s"] / rec["eval_step_folded"]["images_per_s"]
    rec["prec1"] = {k: float(v[1]) for k, v in results.items()}
    rec["batch"], rec["bits"], rec["batches"] = BATCH, BITS, batches
    return rec


def depthwise_shapes():
    """(C, H_in, stride) of every depthwise convolution of the full network at 32x32 inputs, in order, without repeats"""
    shapes, planes, side = [], 32, 32
    for expansion, out_planes, num_blocks, stride in M.MobileNetV2.cfg:
        for s in [stride] + [1] * (num_blocks - 1):
            shape = (expansion * planes, side, s)
            if shape not in shapes:
                shapes.append(shape)
            side, planes = (side - 1) // s + 1, out_planes
    return shapes


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    return g


def time_graphs(graphs, rounds):
    """{name: [microseconds per repetition, one per round]}: the graphs replayed alternately, device events around each replay"""
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


def depthwise_sites(dev, rounds):
    lib = L.load()
    r, formula, k = float(config.args.act_range), L.FORMULA_CDF, BITS
    recs = []
    for C, H, s in depthwise_shapes():
        Ho = (H - 1) // s + 1
        x = torch.relu(torch.randn(BATCH, C, H, H, device=dev)).contiguous(memory_format=torch.channels_last)
        w = (2.0 * torch.randint(0, 16, (C, 1, 3, 3), device=dev) / 15.0 - 1.0).float()
        g, b, m = (torch.randn(C, device=dev) * 0.3 + o for o in (1.0, 0.0, 0.1))
        v = torch.rand(C, device=dev) + 0.5
        mid = torch.empty(BATCH, C, Ho, Ho, device=dev).contiguous(memory_format=torch.channels_last)
        y1, y2 = torch.empty_like(mid), torch.empty_like(mid)
        site_f = L.EvalSite(None, L.ptr(g), L.ptr(b), L.ptr(m), L.ptr(v), 1e-5, k, fused.CLAMP_RELU6)
        site_2 = L.EvalSite(L.ptr(mid), L.ptr(g), L.ptr(b), L.ptr(m), L.ptr(v), 1e-5, k, fused.CLAMP_RELU6)

        def one_launch():
            L.check(lib.alignq_dwconv3x3_site_eval_fwd(L.ptr(x), L.ptr(w), ctypes.byref(site_f), BATCH, H, H, C, s, r, formula, L.ptr(y1),
                                                       L.stream_ptr()), "alignq_dwconv3x3_site_eval_fwd")

        def two_launches():
            L.check(lib.alignq_dwconv3x3_nhwc_fwd(L.ptr(x), L.ptr(w), L.ptr(mid), BATCH, H, H, C, s, L.stream_ptr()), "alignq_dwconv3x3_nhwc_fwd")
            L.check(lib.alignq_site_eval_fwd(ctypes.byref(site_2), BATCH * Ho * Ho, C, r, formula, None, L.ptr(y2), L.stream_ptr()),
                    "alignq_site_eval_fwd")
        graphs = {"fused": graph_of(one_launch), "two_launches": graph_of(two_launches)}
        torch.cuda.synchronize()
        assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))
        t = time_graphs(graphs, rounds)
        med = {kk: statistics.median(vv) for kk, vv in t.items()}
        recs.append({"C": C, "H_in": H, "stride": s, "out_MB": y1.numel() * 4 / 1e6, "fused_us": med["fused"],
                     "two_launches_us": med["two_launches"], "fused_us_range": [min(t["fused"]), max(t["fused"])],
                     "two_launches_us_range": [min(t["two_launches"]), max(t["two_launches"])],
                     "two_over_fused": med["two_launches"] / med["fused"]})
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mobilenet_eval_bench: needs the GPU (no number is produced without one)")
    dev = torch.device("cuda:0")
    old = (config.args.bitW, config.args.abitW, config.args.train_batch_size)
    try:
        out = {"evaluation": whole_evaluation(dev, a.batches, a.rounds), "depthwise_sites": depthwise_sites(dev, a.rounds)}
    finally:
        config.args.bitW, config.args.abitW, config.args.train_batch_size = old
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
