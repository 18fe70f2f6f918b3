#!/usr/bin/env python
"""What following the reference's schedules costs a captured step, by value (the graph is captured again) and with the
hyper-parameters in device memory (alignq_amd/schedule.py: one graph, a table walked inside it).  ONE variant per process, one
JSON line each:

    office_parent   resnet50_dann, 28 + 28 images of 224 x 224, channels-last: every epoch new_epoch -> one eager iteration ->
                    re-capture -> replays (dann_office/main.py:321-328 with kernel arguments by value; alpha frozen)
    office_device   the same step with device_hyper=True and an office_dann table: every epoch is replays only, alpha per
                    iteration (dann_office/main.py:346-348) included
    cifar_parent    ResNet-20 8W/8A, batch 128: replays, set_lr(lr / 10) (a re-capture), replays
    cifar_device    the same with device_hyper=True: set_lr is one 16-byte copy

Per variant: wall time per epoch, the time per epoch spent outside replays (new_epoch + eager iteration + capture, or set_lr),
and the steady-state time per replayed step; every window ends in a device synchronise.  One process per variant, each under
its own time limit, chained so that a failure ends the chain; the parent variant three times for the run-to-run spread:

    timeout -k 10 280 python tools/schedule_bench.py --variant office_parent && \\
    timeout -k 10 280 python tools/schedule_bench.py --variant office_device && \\
    timeout -k 10 280 python tools/schedule_bench.py --variant office_parent && \\
    timeout -k 10 280 python tools/schedule_bench.py --variant office_parent && \\
    timeout -k 10 120 python tools/schedule_bench.py --variant cifar_parent && \\
    timeout -k 10 120 python tools/schedule_bench.py --variant cifar_device
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alignq_amd import config, schedule  # noqa: E402


def now():
    torch.cuda.synchronize()
    return time.perf_counter()


def office(a, device_hyper, dev):
    from alignq_amd.resnet_office import resnet50_dann
    from alignq_amd.train_step import OfficeTrainStep
    B, lr, num_epochs = a.batch, 0.004, 200                    # (200 epochs: the reference's default, the rate of epoch 0 exists)
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = config.args.eval_batch_size = B
    gen = torch.Generator().manual_seed(0)
    xs = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    xt = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    ys = torch.randint(0, 31, (B,), generator=gen).to(dev)
    torch.manual_seed(0)
    step = OfficeTrainStep(resnet50_dann(8, 8).to(dev).train(), lr=lr, alpha=0.5, channels_last=True, device_hyper=device_hyper)
    if device_hyper:
        step.set_schedule(schedule.office_dann(lr, num_epochs, a.iters))
    step.capture(xs, ys, xt, warmup=3)
    if device_hyper:
        step.seek(0)
    sx = step.static_inputs()
    for _ in range(10):
        step(*sx)
    if device_hyper:
        step.seek(0)
    graphs, epochs = {id(step._graph)}, []
    for epoch in range(a.epochs):
        t0 = now()
        step.new_epoch(epoch, num_epochs, lr)
        replays = a.iters
        if not device_hyper:
            step(*sx)                       # the eager first iteration of the epoch, and the capture behind it
            replays -= 1
        t1 = now()
        for _ in range(replays):
            step(*step.static_inputs())
        t2 = now()
        graphs.add(id(step._graph))
        epochs.append(dict(epoch_s=t2 - t0, outside_replays_s=t1 - t0, ms_per_replay=1e3 * (t2 - t1) / replays))
    out = summary(epochs)
    out.update(graphs_seen=len(graphs), batch=B, iters=a.iters)
    if device_hyper:
        out["hyper"] = step.current_hyper()
    return out


def cifar(a, device_hyper, dev):
    from alignq_amd.resnet import resnet20_quant
    from alignq_amd.train_step import TrainStep
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = 128
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(128, 3, 32, 32, generator=gen).to(dev)
    y = torch.randint(0, 10, (128,), generator=gen).to(dev)
    torch.manual_seed(0)
    step = TrainStep(resnet20_quant(8, 8).to(dev).train(), lr=0.04, channels_last=True, device_hyper=device_hyper)
    step.capture(x, y, warmup=3)
    n = a.cifar_iters
    for _ in range(200):
        step(*step.static_inputs())
    epochs, lr = [], 0.04
    for epoch in range(a.epochs):
        lr = lr / 10
        t0 = now()
        step.set_lr(lr)
        t1 = now()
        for _ in range(n):
            step(*step.static_inputs())
        t2 = now()
        epochs.append(dict(epoch_s=t2 - t0, outside_replays_s=t1 - t0, ms_per_replay=1e3 * (t2 - t1) / n))
    out = summary(epochs)
    out.update(batch=128, iters=n)
    return out


def summary(epochs):
    return dict(epoch_s=statistics.median(e["epoch_s"] for e in epochs),
                outside_replays_s=statistics.median(e["outside_replays_s"] for e in epochs),
                ms_per_replay=statistics.median(e["ms_per_replay"] for e in epochs),
                best_ms_per_replay=min(e["ms_per_replay"] for e in epochs), epochs=epochs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", required=True, choices=["office_parent", "office_device", "cifar_parent", "cifar_device"])
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100, help="iterations per Office epoch (Office-31: on the order of a hundred)")
    ap.add_argument("--batch", type=int, default=28)
    ap.add_argument("--cifar-iters", type=int, default=391, help="iterations per CIFAR epoch (50000 / 128)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "schedule_bench needs the GPU"
    dev = torch.device("cuda:0")
    kind, mode = a.variant.split("_")
    out = (office if kind == "office" else cifar)(a, mode == "device", dev)
    out["variant"] = a.variant
    print(json.dumps(out))


if __name__ == "__main__":
    main()
