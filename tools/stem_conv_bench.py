#!/usr/bin/env python3
"""The 3x3 image-form kernels (csrc/k3image_kernels.hip) against what Conv2d_Q does without them, at the two 3-channel stems of the
reference trees - DenseNet-40's conv1 (3 -> 24) and MobileNet-V2's (3 -> 32) - for 32 x 32 inputs at a batch of 128; and DenseNet-40's
captured evaluation at eval_batch_size = 100 with the stem on MIOpen (densenet.use_hip_convs(model, dense_eval=True)) and in the first
block's buffer (stem=True).

Per stem and operation, two ways on the same channels-last tensors:
  hip   alignq_k3image_fwd / _wgrad (the filter gradient with its slab reduction), the filter bins packed beforehand;
  base  F.conv2d / aten.convolution_backward with the filter gradient asked for (MIOpen, fp32).
Each is captured as a graph of REPS launches; the two graphs of an operation are replayed alternately for `--rounds` rounds after a
warm-up replay, device events around every REPLAYS replays.  Both sides' tensors stay resident in cache across replays.  Median and range
of the rounds, microseconds per launch.  `verdict` is "SLOWER" where the hip median exceeds the base median by more than the base's own
range.  The evaluation: the two EvalSteps captured and replayed `--batches` times between device synchronisations, in interleaved
rounds, a host clock around each; per path also what one eager batch issues (this library's launching entry points and the ATen
operators that launch work, tools/dense_eval_bench.py's count).

    python tools/stem_conv_bench.py --out profiles/stem_conv_bench.json
"""
import argparse
import collections
import copy
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dense_eval_bench as DB  # noqa: E402
from alignq_amd import _lib as L  # noqa: E402
from alignq_amd import config, ops  # noqa: E402
from alignq_amd import densenet as D  # noqa: E402
from alignq_amd.eval_step import EvalStep  # noqa: E402

REPS = 10
REPLAYS = 40
STEMS = (24, 32)          # C_out of DenseNet-40's and MobileNet-V2's conv1
CL = torch.channels_last


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


def bench_stems(a, dev, res, dump):
    lib = L.load()
    g = torch.Generator(device="cpu").manual_seed(0)
    n = 2 ** a.bits - 1
    conv_args = (None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1)
    B, H = a.batch, 32
    for cout in STEMS:
        geom = (B, H, H, cout)
        x = torch.randn(B, 3, H, H, generator=g).to(dev).contiguous(memory_format=CL)
        w = (torch.round(torch.tanh(torch.randn(cout, 3, 3, 3, generator=g)) * n) / n).to(dev).contiguous(memory_format=CL)
        dy = (torch.randn(B, cout, H, H, generator=g) * 1e-3).to(dev).contiguous(memory_format=CL)
        bins = ops.pack_filter_bins([w], a.bits)[0][0]
        y, dw = torch.empty_like(dy), torch.empty_like(w)
        ws = torch.empty(max(int(lib.alignq_k3image_wgrad_ws_bytes(*geom)), 16), dtype=torch.uint8, device=dev)
        hip = {
            "fwd": lambda: L.check(lib.alignq_k3image_fwd(L.ptr(x), L.ptr(bins), L.ptr(y), *geom, cout, a.bits, L.stream_ptr()), "fwd"),
            "wgrad": lambda: L.check(lib.alignq_k3image_wgrad(L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(ws), *geom, None, L.stream_ptr()), "wgrad"),
        }
        base = {
            "fwd": lambda: F.conv2d(x, w, None, 1, 1),
            "wgrad": lambda: torch.ops.aten.convolution_backward(dy, x, w, *conv_args, (False, True, False)),
        }
        flop = 2 * B * H * H * cout * 27
        nbytes = {"fwd": 4 * (x.numel() + y.numel()) + 2 * w.numel(), "wgrad": 4 * (x.numel() + y.numel() + w.numel())}
        row = {"COUT": cout, "H": H, "B": B, "flop": flop, "n_slabs": int(len(ws) // (4 * 27 * cout)), "ops": {}}
        for i, op in enumerate(("fwd", "wgrad")):
            t = time_graphs({"hip": graph_of(hip[op]), "base": graph_of(base[op])}, a.rounds)
            hm, bm = statistics.median(t["hip"]), statistics.median(t["base"])
            spread = max(t["base"]) - min(t["base"])
            row["ops"][op] = {"form": lib.alignq_k3image_form(i, *geom),
                              "hip_us": hm, "hip_us_range": [min(t["hip"]), max(t["hip"])],
                              "base_us": bm, "base_us_range": [min(t["base"]), max(t["base"])],
                              "hip_over_base": hm / bm, "verdict": "SLOWER" if hm > bm + spread else "not slower",
                              "algorithmic_bytes": nbytes[op], "hip_bytes_per_s": nbytes[op] / (hm * 1e-6)}
        res["stems"].append(row)
        print(json.dumps(row), flush=True)
        dump()


def count_one_batch(ev, x, y):
    """tools/dense_eval_bench.py's count of one eager batch, with this family's entry points among the names"""
    lib = L.load()
    calls, saved = collections.Counter(), {}
    for table in (L.SIGNATURES, L.MOBILE_SIGNATURES, L.POINTWISE_SIGNATURES, L.K3CONV_SIGNATURES, L.DENSE_SIGNATURES, L.K3IMAGE_SIGNATURES):
        for name in table:
            saved[name] = getattr(lib, name)

            def wrapper(*args, _orig=saved[name], _n=name):
                calls[_n] += 1
                return _orig(*args)
            setattr(lib, name, wrapper)
    try:
        with ev:
            calls.clear()          # (begin() quantises the filters once per evaluation: not part of a batch)
            with DB.CountOps() as mode:
                ev._eager_fallback(x, y)
            torch.cuda.synchronize()
    finally:
        for name, f in saved.items():
            setattr(lib, name, f)
    entry = {k: v for k, v in calls.items()
             if (k.endswith(("_fwd", "_metrics")) or "conv" in k) and not k.endswith(("_supported", "_form", "_bytes"))}
    return {"entry_points": dict(entry), "aten": dict(mode.ops), "launches": sum(entry.values()) + sum(mode.ops.values())}


def bench_evaluation(a, dev, res, dump):
    base = DB.build(dev)
    nets = {"stem_miopen": D.use_hip_convs(copy.deepcopy(base), dense_eval=True),
            "stem_hip": D.use_hip_convs(copy.deepcopy(base), dense_eval=True, stem=True)}
    xs = [torch.randn(DB.BATCH, 3, 32, 32, device=dev).contiguous(memory_format=CL) for _ in range(4)]
    ys = [torch.randint(0, 10, (DB.BATCH,), device=dev) for _ in range(4)]
    counts = {k: count_one_batch(EvalStep(net), xs[0], ys[0]) for k, net in nets.items()}
    evs = {k: EvalStep(net) for k, net in nets.items()}
    logits = {}
    for k, ev in evs.items():          # warm-up round (plans, allocator pools, the captures), not timed
        DB.run_eval_step(ev, xs, ys, 4)
        with ev:
            logits[k] = ev(xs[0], ys[0]).clone()
    times = {k: [] for k in evs}
    for _ in range(a.rounds):
        for k, ev in evs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            DB.run_eval_step(ev, xs, ys, a.batches)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    rec = {k: {"ms_per_batch": 1e3 * statistics.median(v) / a.batches,
               "ms_per_batch_range": [1e3 * min(v) / a.batches, 1e3 * max(v) / a.batches], "one_batch": counts[k]} for k, v in times.items()}
    hm, bm = rec["stem_hip"]["ms_per_batch"], rec["stem_miopen"]["ms_per_batch"]
    spread = rec["stem_miopen"]["ms_per_batch_range"][1] - rec["stem_miopen"]["ms_per_batch_range"][0]
    rec.update({"hip_over_miopen": hm / bm, "verdict": "SLOWER" if hm > bm + spread else "not slower",
                "max_abs_logit_difference": float((logits["stem_hip"] - logits["stem_miopen"]).abs().max()),
                "max_abs_logit": float(logits["stem_miopen"].abs().max()), "batch": DB.BATCH, "batches": a.batches})
    res["evaluation"] = rec
    print(json.dumps(rec), flush=True)
    dump()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--stems-only", action="store_true", help="skip the evaluation (A/B builds through ALIGNQ_SO)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stem_conv_bench: needs the GPU (no number is produced without one)")
    dev = torch.device("cuda:0")
    res = {"batch": a.batch, "bits": a.bits, "rounds": a.rounds, "reps": REPS, "replays": REPLAYS,
           "library": L.SO_PATH if os.environ.get("ALIGNQ_SO") else "product", "device": torch.cuda.get_device_name(0), "stems": []}

    def dump():          # after every row: a run that is cut short leaves what it measured
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    old = (config.args.bitW, config.args.abitW)
    try:
        bench_stems(a, dev, res, dump)
        if not a.stems_only:
            bench_evaluation(a, dev, res, dump)
    finally:
        config.args.bitW, config.args.abitW = old
    print(json.dumps(res))


if __name__ == "__main__":
    main()
