#!/usr/bin/env python
"""What an ITERATION of configuration 5 costs with the input pipeline in it (ResNet-50-DANN 8W/8A, 28 source + 28 target images
of 224 x 224; synthetic Amazon -> Webcam sizes: 2 817 and 795 images stored as 256 x 256 bytes, the reference's loaders without
drop_last, walked as dann_office/main.py:340-343 zips them: 28 full iterations and one of 28 + 11 per epoch).  Prints one JSON line.

    python tools/office_epoch_bench.py [--source 2817] [--target 795] [--batch 28] [--rounds 5] [--limit 240]

Forms, each one warm epoch and then `--rounds` timed epochs in ONE process, each form under its own time limit (SIGALRM: a form
that overruns ends the process):
  bare      (a) the captured step replayed on static batches (what bench.py --model resnet50_dann times)
  in_graph  (b) the pair loader inside the step's graph (set_producer(PairLoader)): an iteration is one replay
  host      (c) what a user had to do before: RandomCrop(224) + flip + ToTensor + Normalize vectorised in torch on the host
            (16 threads) on the resized bytes, a pinned double-buffered copy into static_inputs(), replay
ms_per_iteration is the time of the epoch's full iterations / their number (device synchronised at both ends); the short last
iteration (eager fallback in every form but `bare`) is timed with the epoch only."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alignq_amd import config, data as D  # noqa: E402
from alignq_amd.resnet_office import resnet50_dann  # noqa: E402
from alignq_amd.train_step import OfficeTrainStep  # noqa: E402

SIDE, CROP = D.OFFICE_SIDE, D.OFFICE_CROP


class HostDomain:
    """The reference's train transforms of one domain, batched, in torch on the host; double-buffered pinned staging."""

    def __init__(self, images, labels, batch, seed):
        self.images, self.labels, self.batch = torch.from_numpy(images), torch.from_numpy(labels), batch
        self.mean, self.std = torch.tensor(D.IMAGENET_MEAN).view(1, 1, 1, 3), torch.tensor(D.IMAGENET_STD).view(1, 1, 1, 3)
        self.gen = torch.Generator().manual_seed(seed)
        self.pin_x = [torch.empty(batch, CROP, CROP, 3).pin_memory() for _ in range(2)]
        self.pin_y = [torch.empty(batch, dtype=torch.int64).pin_memory() for _ in range(2)]
        self.free = [torch.cuda.Event(), torch.cuda.Event()]
        self.turn = 0
        self.ar = torch.arange(CROP)

    def begin_epoch(self):
        self.perm = torch.randperm(len(self.images), generator=self.gen)

    def batch_into(self, k, sx, sy):
        idx = self.perm[k * self.batch:(k + 1) * self.batch]
        b = len(idx)
        dy = torch.randint(0, SIDE - CROP + 1, (b,), generator=self.gen)
        dx = torch.randint(0, SIDE - CROP + 1, (b,), generator=self.gen)
        f = torch.rand(b, generator=self.gen) < 0.5
        rows = dy[:, None] + self.ar
        cols = dx[:, None] + torch.where(f[:, None], CROP - 1 - self.ar, self.ar)
        crop = self.images[idx[:, None, None], rows[:, :, None], cols[:, None, :]]
        slot = self.turn
        self.turn ^= 1
        self.free[slot].synchronize()                        # the copy that last read this staging buffer has finished
        px, py = self.pin_x[slot][:b], self.pin_y[slot][:b]
        torch.div(crop.to(torch.float32), 255, out=px)
        px.sub_(self.mean).div_(self.std)
        py.copy_(self.labels[idx])
        if b == sx.shape[0]:
            sx.permute(0, 2, 3, 1).copy_(px, non_blocking=True)       # channels-last storage: the same memory order
            if sy is not None:
                sy.copy_(py, non_blocking=True)
            self.free[slot].record()
            return sx, sy
        x, y = px.permute(0, 3, 1, 2).to(sx.device, non_blocking=True), py.to(sx.device, non_blocking=True)
        self.free[slot].record()
        return x, y


def synthetic(n, classes, rng):
    """n images of SIDE x SIDE random bytes drawn from a pool of 256 distinct ones (the kernel's work does not depend on content)"""
    pool = rng.integers(0, 256, (256, SIDE, SIDE, 3), dtype=np.uint8)
    return pool[rng.integers(0, len(pool), n)], rng.integers(0, classes, n).astype(np.int64)


def timed_epoch(full, run_full, run_last):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(full):
        run_full(k)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    run_last()
    torch.cuda.synchronize()
    return t1 - t0, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", type=int, default=2817)
    ap.add_argument("--target", type=int, default=795)
    ap.add_argument("--batch", type=int, default=28)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds each form may take")
    ap.add_argument("--host-threads", type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "office_epoch_bench needs the GPU"
    torch.set_num_threads(a.host_threads)
    dev = torch.device("cuda:0")
    B = a.batch
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = config.args.eval_batch_size = B
    rng = np.random.default_rng(0)
    sets = [synthetic(a.source, 31, rng), synthetic(a.target, 31, rng)]
    src = D.DeviceLoader(D.DeviceImages.office(*sets[0], train=True, device=dev), B, seed=0, channels_last=True)
    tgt = D.DeviceLoader(D.DeviceImages.office(*sets[1], train=True, device=dev), B, seed=1, channels_last=True)
    pair = D.PairLoader(src, tgt, "zip")
    sizes = pair.iterations()
    full = sum(1 for s in sizes if s == (B, B))
    short = len(sizes) - full
    hosts = [HostDomain(*sets[0], B, 0), HostDomain(*sets[1], B, 1)]
    torch.manual_seed(0)
    step = OfficeTrainStep(resnet50_dann(8, 8).to(dev).train(), lr=0.004, channels_last=True)
    first = pair.peek()
    step.capture(*first, warmup=2)
    sxs, sys_, sxt = step.static_inputs()

    def form_bare():
        return timed_epoch(full, lambda k: step(sxs, sys_, sxt), lambda: None)

    def host_batch(k):
        xs, ys = hosts[0].batch_into(k, sxs, sys_)
        xt, _ = hosts[1].batch_into(k, sxt, None)
        return xs, ys, xt

    def form_host():
        for h in hosts:
            h.begin_epoch()
        return timed_epoch(full, lambda k: step(*host_batch(k)), lambda: short and step(*host_batch(full)))

    def form_in_graph():
        pair.begin_epoch(form_in_graph.epoch)
        form_in_graph.epoch += 1
        return timed_epoch(full, lambda k: step.next(), lambda: short and step.next())
    form_in_graph.epoch = 0

    def overrun(signum, frame):
        raise SystemExit("office_epoch_bench: a form exceeded its time limit of %d s" % a.limit)
    signal.signal(signal.SIGALRM, overrun)

    def measure(name, form):
        signal.alarm(a.limit)
        form()                                               # the warm epoch
        runs = [form() for _ in range(a.rounds)]
        signal.alarm(0)
        t_full = statistics.median(r[0] for r in runs)
        t_all = statistics.median(r[1] for r in runs)
        imgs = 2 * full * B if name == "bare" else sum(s + t for s, t in sizes)
        return {"ms_per_iteration": 1e3 * t_full / full, "best_ms_per_iteration": 1e3 * min(r[0] for r in runs) / full,
                "images_per_s": imgs / t_all, "epoch_s": t_all}

    out = {"source": a.source, "target": a.target, "batch": B, "full_iterations": full, "short_iterations": short,
           "rounds": a.rounds, "host_threads": a.host_threads, "set_bytes": int(src.images.images.numel() + tgt.images.images.numel())}
    out["bare"] = measure("bare", form_bare)
    out["host"] = measure("host", form_host)
    out["bare_again"] = measure("bare", form_bare)           # the spread of the yardstick inside this process
    step.set_producer(pair)
    step.capture(*first, warmup=0)
    out["in_graph"] = measure("in_graph", form_in_graph)
    out["in_graph_minus_bare_us"] = 1e3 * (out["in_graph"]["ms_per_iteration"] - min(out["bare"]["ms_per_iteration"],
                                                                                    out["bare_again"]["ms_per_iteration"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
