#!/usr/bin/env python
"""File sizes of a packed k-bit checkpoint (export.PackedModel.save) against the dense `torch.save(state_dict())`, and the time of
EvalStep.begin() from the packed codes (alignq_weight_unpack_multi) against begin() from the fp32 filters
(fused.prequantize_weights: statistics, erf, rounding, then the bins pass), in the same process and run.  Prints one JSON line.

    python tools/packed_eval_bench.py [--configs r20_admm,r20_cdf,r50_dann] [--rounds 5] [--reps 20] [--out FILE]

begin() is timed as wall time around begin() + synchronize (it is host work plus a handful of launches; end() is outside the
timed span), `reps` times per round, the two paths interleaved round by round; the median over all rounds, the fastest and the
slowest round's median (the run-to-run spread) are reported."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alignq_amd import config, export  # noqa: E402
from alignq_amd.eval_step import EvalStep  # noqa: E402

CONFIGS = {"r20_admm": ("admm", 8), "r20_cdf": ("cdf", 8), "r50_dann": ("dann", 8)}


def build(kind, bits, dev):
    config.args.bitW = config.args.abitW = bits
    torch.manual_seed(0)
    if kind == "dann":
        from alignq_amd.resnet_office import resnet50_dann
        config.args.train_batch_size = 28
        return resnet50_dann(bits, bits).to(dev)
    from alignq_amd.resnet import resnet20_quant
    config.args.train_batch_size = 128
    return resnet20_quant(bits, bits, tree=kind).to(dev)


def time_begin(ev, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.begin()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
        ev.end()
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"rounds": a.rounds, "reps": a.reps, "configs": {}}
    for name in a.configs.split(","):
        kind, bits = CONFIGS[name]
        net = build(kind, bits, dev)
        pk = export.pack_model(net)
        with tempfile.TemporaryDirectory() as tmp:
            dense_path, packed_path = os.path.join(tmp, "dense.pt"), os.path.join(tmp, "packed.alignq")
            torch.save(net.state_dict(), dense_path)
            pk.save(packed_path)
            sizes = {"dense_file_bytes": os.path.getsize(dense_path), "packed_file_bytes": os.path.getsize(packed_path)}
            pk = export.PackedModel.load(packed_path)
        sizes.update(packed_nbytes=pk.nbytes(), dense_nbytes=pk.dense_nbytes(),
                     filters=len(pk.filters), filter_elements=sum(pk._numel(f) for f in pk.filters.values()))
        paths = {"begin_fp32": EvalStep(net), "begin_packed": EvalStep(net, weights=pk)}
        for ev in paths.values():
            time_begin(ev, 3)                     # warm-up: allocations, the first unpack's buffers
        meds = {k: [] for k in paths}
        for _ in range(a.rounds):
            for k, ev in paths.items():
                meds[k].append(time_begin(ev, a.reps))
        rec = dict(sizes)
        for k, v in meds.items():
            rec[k + "_us"] = {"median": 1e6 * statistics.median(v), "min": 1e6 * min(v), "max": 1e6 * max(v)}
        rec["packed_over_fp32"] = rec["begin_packed_us"]["median"] / rec["begin_fp32_us"]["median"]
        rec["file_ratio"] = sizes["packed_file_bytes"] / sizes["dense_file_bytes"]
        res["configs"][name] = rec
        del net, paths, pk
        torch.cuda.empty_cache()
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = 128
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
