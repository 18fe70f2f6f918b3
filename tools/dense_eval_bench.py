#!/usr/bin/env python
"""DenseNet-40 (CIFAR-10) evaluation at eval_batch_size = 100 through EvalStep, with `fuse_dense_eval` off and on, on the same
commit; and each of the 36 dense-layer shapes of the network as one fused launch against the launches it replaces.
Prints one JSON line; --out also writes it to a file.

    python tools/dense_eval_bench.py [--batches 50] [--rounds 7] [--out profiles/dense_eval_bench.json]

Whole evaluation, two paths timed in interleaved rounds in one process (median, best and worst round reported), each a captured
EvalStep replayed `batches` times between device synchronisations:
  composed   densenet.use_hip_convs(model): per dense layer batch-norm, quantiser, ReLU, alignq_k3conv_fwd and torch.cat;
  fused      densenet.use_hip_convs(model, dense_eval=True): DenseNet._forward_eval, one alignq_dense_layer_eval_fwd per dense layer
             into one buffer per block, the transitions' pools written into the next buffer.
Per path also what one eager batch issues: the calls of this library's entry points and the ATen operators that launch work (views,
allocations and metadata operators left out), counted by a dispatch mode - the launch counts the two paths are compared by.
Per dense-layer shape (CIN, H) at batch 100: a graph of REPS fused launches (in place in a (B, CIN + 12, H, H) buffer) against a graph of
REPS (alignq_site_eval_fwd, alignq_k3conv_fwd, torch.cat) triples, replayed alternately, device events around each group of replays;
microseconds per layer, medians over the rounds.  Both forms are checked to give the same bits before they are timed."""
import argparse
import collections
import copy
import ctypes
import json
import os
import statistics
import sys
import time

import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alignq_amd import _lib as L  # noqa: E402
from alignq_amd import config, fused, ops  # noqa: E402
from alignq_amd import densenet as D  # noqa: E402
from alignq_amd.eval_step import EvalStep  # noqa: E402

BATCH, BITS, REPS, GROWTH = 100, 4, 10, 12
CL = torch.channels_last
# ATen operators that launch nothing: views, allocations, metadata
NO_LAUNCH = ("view", "reshape", "as_strided", "empty", "detach", "alias", "t.default", "transpose", "permute", "expand", "slice", "select",
             "squeeze", "unsqueeze", "_unsafe_view", "is_", "size", "stride", "sym_", "_local_scalar", "lift_fresh", "resize_", "narrow",
             "set_", "_to_copy_meta", "contiguous")


class CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = collections.Counter()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func).replace("aten.", "")
        if not any(name.startswith(p) for p in NO_LAUNCH):
            self.ops[name] += 1
        return func(*args, **(kwargs or {}))


def build(dev):
    config.args.bitW = config.args.abitW = BITS
    torch.manual_seed(0)
    net = D.densenet_40_quant(BITS, BITS, "no_align").to(dev)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0.0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    return net.train()


def count_one_batch(ev, x, y):
    """{entry point or ATen operator: calls} of one eager batch"""
    lib = L.load()
    names = list(L.SIGNATURES) + list(L.MOBILE_SIGNATURES) + list(L.POINTWISE_SIGNATURES) + list(L.K3CONV_SIGNATURES) + list(L.DENSE_SIGNATURES)
    calls, saved = collections.Counter(), {}
    for n in names:
        saved[n] = getattr(lib, n)

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
    # the entry points that launch: forwards, convolutions, the metrics; the `*_supported` / `*_form` queries launch nothing
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


def whole_evaluation(dev, batches, rounds):
    base = build(dev)
    nets = {"composed": D.use_hip_convs(copy.deepcopy(base)), "fused": D.use_hip_convs(copy.deepcopy(base), dense_eval=True)}
    xs = [torch.randn(BATCH, 3, 32, 32, device=dev).contiguous(memory_format=CL) for _ in range(4)]
    ys = [torch.randint(0, 10, (BATCH,), device=dev) for _ in range(4)]
    counts = {k: count_one_batch(EvalStep(net), xs[0], ys[0]) for k, net in nets.items()}
    evs = {k: EvalStep(net) for k, net in nets.items()}
    logits = {}
    for k, ev in evs.items():          # warm-up round (plans, allocator pools, the captures), not timed
        run_eval_step(ev, xs, ys, 4)
        with ev:
            logits[k] = ev(xs[0], ys[0]).clone()
    times, results = {k: [] for k in evs}, {}
    for _ in range(rounds):
        for k, ev in evs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[k] = run_eval_step(ev, xs, ys, batches)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    n_img = batches * BATCH
    rec = {k: {"ms_per_batch": 1e3 * statistics.median(v) / batches, "best_ms_per_batch": 1e3 * min(v) / batches,
               "worst_ms_per_batch": 1e3 * max(v) / batches, "images_per_s": n_img / statistics.median(v),
               "rounds_ms_per_batch": [1e3 * t / batches for t in v], "one_batch": counts[k]} for k, v in times.items()}
    rec["composed_over_fused"] = rec["composed"]["ms_per_batch"] / rec["fused"]["ms_per_batch"]
    rec["max_abs_logit_difference"] = float((logits["composed"] - logits["fused"]).abs().max())
    rec["max_abs_logit"] = float(logits["composed"].abs().max())
    rec["prec1"] = {k: float(v[1]) for k, v in results.items()}
    rec["batch"], rec["bits"], rec["batches"], rec["rounds"] = BATCH, BITS, batches, rounds
    return rec


def dense_shapes():
    """(CIN, H) of the 36 dense layers of DenseNet-40 at 32x32 inputs (compressionRate 1), in order"""
    shapes, cin, side = [], 2 * GROWTH, 32
    for _ in range(3):
        for _ in range(12):
            shapes.append((cin, side))
            cin += GROWTH
        side //= 2
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
    """{name: [microseconds per repetition, one per round]}: the graphs replayed alternately, device events around each group"""
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


def dense_layers(dev, rounds):
    lib = L.load()
    r, formula, k = float(config.args.act_range), L.FORMULA_CDF, BITS
    n = 2 ** BITS - 1
    recs = []
    for cin, H in dense_shapes():
        C_end = cin + GROWTH
        buf = torch.randn(BATCH, C_end, H, H, device=dev).contiguous(memory_format=CL)
        x = buf[:, :cin].contiguous(memory_format=CL)
        wq = (torch.round(torch.tanh(torch.randn(GROWTH, cin, 3, 3, device=dev)) * n) / n).contiguous(memory_format=CL)
        bins = ops.pack_filter_bins([wq], BITS)[0][0]
        g, b, m = (torch.randn(cin, device=dev) * 0.3 + o for o in (1.0, 0.0, 0.1))
        v = torch.rand(cin, device=dev) + 0.5
        tmp = torch.empty_like(x)
        y = torch.empty(BATCH, GROWTH, H, H, device=dev).contiguous(memory_format=CL)
        held = {}
        site_f = L.DenseSite(L.ptr(g), L.ptr(b), L.ptr(m), L.ptr(v), 1e-5, k, fused.CLAMP_RELU)
        site_2 = L.EvalSite(L.ptr(x), L.ptr(g), L.ptr(b), L.ptr(m), L.ptr(v), 1e-5, k, fused.CLAMP_RELU)

        def one_launch():
            p = buf.data_ptr()
            L.check(lib.alignq_dense_layer_eval_fwd(p, C_end, p + 4 * cin, C_end, ctypes.byref(site_f), L.ptr(bins), BATCH, H, H, cin, GROWTH,
                                                    BITS, r, formula, L.stream_ptr()), "alignq_dense_layer_eval_fwd")

        def replaced():
            L.check(lib.alignq_site_eval_fwd(ctypes.byref(site_2), BATCH * H * H, cin, r, formula, None, L.ptr(tmp), L.stream_ptr()),
                    "alignq_site_eval_fwd")
            L.check(lib.alignq_k3conv_fwd(L.ptr(tmp), L.ptr(bins), L.ptr(y), BATCH, H, H, cin, GROWTH, BITS, L.stream_ptr()),
                    "alignq_k3conv_fwd")
            held["cat"] = torch.cat((x, y), 1)

        def site_conv():
            L.check(lib.alignq_site_eval_fwd(ctypes.byref(site_2), BATCH * H * H, cin, r, formula, None, L.ptr(tmp), L.stream_ptr()),
                    "alignq_site_eval_fwd")
            L.check(lib.alignq_k3conv_fwd(L.ptr(tmp), L.ptr(bins), L.ptr(y), BATCH, H, H, cin, GROWTH, BITS, L.stream_ptr()),
                    "alignq_k3conv_fwd")
        graphs = {"fused": graph_of(one_launch), "replaced": graph_of(replaced), "site_conv": graph_of(site_conv)}
        for gr in graphs.values():          # (the tensors a capture allocates hold values only after a replay)
            gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf.view(torch.int32), held["cat"].view(torch.int32))
        t = time_graphs(graphs, rounds)
        med = {kk: statistics.median(vv) for kk, vv in t.items()}
        recs.append({"CIN": cin, "H": H, "fused_us": med["fused"], "site_conv_cat_us": med["replaced"], "site_conv_us": med["site_conv"],
                     "fused_us_range": [min(t["fused"]), max(t["fused"])],
                     "site_conv_cat_us_range": [min(t["replaced"]), max(t["replaced"])],
                     "replaced_over_fused": med["replaced"] / med["fused"], "site_conv_over_fused": med["site_conv"] / med["fused"]})
        del graphs, held
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_eval_bench: needs the GPU (no number is produced without one)")
    dev = torch.device("cuda:0")
    old = (config.args.bitW, config.args.abitW)
    try:
        layers = dense_layers(dev, a.rounds)
        out = {"evaluation": whole_evaluation(dev, a.batches, a.rounds), "dense_layers": layers,
               "dense_layers_sum_us": {k: sum(rec[k] for rec in layers) for k in ("fused_us", "site_conv_cat_us", "site_conv_us")}}
    finally:
        config.args.bitW, config.args.abitW = old
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
