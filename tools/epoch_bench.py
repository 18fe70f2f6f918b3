#!/usr/bin/env python
"""What an EPOCH of the headline workload costs with the input pipeline in it (ResNet-20 8W/8A CDF+ADMM, batch 128, a synthetic
50 000-image uint8 set: 390 batches of 128 and one of 80, the reference's loader without drop_last).  Prints one JSON line.

    python tools/epoch_bench.py [--images 50000] [--batch 128] [--rounds 3] [--limit 240]

Forms, each one warm epoch and then `--rounds` timed epochs in ONE process, each form under its own time limit (SIGALRM: a form
that overruns ends the process):
  bare      the captured step replayed on a static batch (what bench.py times), 390 replays
  host      what a user had to do before alignq_amd.data: RandomCrop(32, 4) + flip + ToTensor + Normalize in torch on the host
            (16 threads), a pinned copy into static_inputs(), replay
  eager     DeviceLoader.fill(*static_inputs()) in front of each replay
  in_graph  the loader inside the step's graph (set_producer): an epoch is 390 replays + the short batch
ms_per_step is the time of the 390 full batches / 390 (device synchronised at both ends); images_per_s counts the whole epoch,
the short last batch (eager fallback in every form) included."""
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
from alignq_amd.resnet import resnet20_quant  # noqa: E402
from alignq_amd.train_step import TrainStep  # noqa: E402


class HostPipeline:
    """The reference's transforms, batched, in torch on the host; double-buffered pinned staging into the step's input buffers."""

    def __init__(self, images, labels, batch, mean, std, seed):
        self.images, self.labels, self.batch = torch.from_numpy(images), torch.from_numpy(labels), batch
        self.mean, self.std = torch.tensor(mean).view(1, 1, 1, 3), torch.tensor(std).view(1, 1, 1, 3)
        self.gen = torch.Generator().manual_seed(seed)
        self.pin_x = [torch.empty(batch, 32, 32, 3).pin_memory() for _ in range(2)]
        self.pin_y = [torch.empty(batch, dtype=torch.int64).pin_memory() for _ in range(2)]
        self.free = [torch.cuda.Event(), torch.cuda.Event()]
        self.turn = 0
        self.ar = torch.arange(32)

    def begin_epoch(self):
        self.perm = torch.randperm(len(self.images), generator=self.gen)

    def batch_into(self, k, sx, sy):
        idx = self.perm[k * self.batch:(k + 1) * self.batch]
        b = len(idx)
        padded = torch.nn.functional.pad(self.images[idx], (0, 0, 4, 4, 4, 4))
        dy = torch.randint(0, 9, (b,), generator=self.gen)
        dx = torch.randint(0, 9, (b,), generator=self.gen)
        f = torch.rand(b, generator=self.gen) < 0.5
        rows = dy[:, None] + self.ar
        cols = dx[:, None] + torch.where(f[:, None], 31 - self.ar, self.ar)
        crop = padded[torch.arange(b)[:, None, None], rows[:, :, None], cols[:, None, :]]
        slot = self.turn
        self.turn ^= 1
        self.free[slot].synchronize()                        # the copy that last read this staging buffer has finished
        px, py = self.pin_x[slot][:b], self.pin_y[slot][:b]
        torch.div(crop.to(torch.float32), 255, out=px)
        px.sub_(self.mean).div_(self.std)
        py.copy_(self.labels[idx])
        if b == sx.shape[0]:
            sx.permute(0, 2, 3, 1).copy_(px, non_blocking=True)       # channels-last storage: the same memory order
            sy.copy_(py, non_blocking=True)
            self.free[slot].record()
            return sx, sy
        x, y = px.permute(0, 3, 1, 2).to(sx.device, non_blocking=True), py.to(sx.device, non_blocking=True)
        self.free[slot].record()
        return x, y


def timed_epoch(full_batches, run_full, run_last):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(full_batches):
        run_full(k)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    run_last()
    torch.cuda.synchronize()
    return t1 - t0, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=50000)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds each form may take")
    ap.add_argument("--host-threads", type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "epoch_bench needs the GPU"
    torch.set_num_threads(a.host_threads)
    dev = torch.device("cuda:0")
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = a.batch
    n, B = a.images, a.batch
    full, short = n // B, n % B
    rng = np.random.default_rng(0)
    images = rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8)
    labels = rng.integers(0, 10, n).astype(np.int64)
    ds = D.DeviceImages.preset("cifar10_train", images, labels, dev)
    loader = D.DeviceLoader(ds, B, seed=0)
    host = HostPipeline(images, labels, B, D.CIFAR10_MEAN, D.CIFAR10_STD, 0)
    torch.manual_seed(0)
    step = TrainStep(resnet20_quant(8, 8).to(dev).train(), lr=0.04, channels_last=True)
    x0, y0 = loader.peek()
    step.capture(x0, y0, warmup=3)
    sx, sy = step.static_inputs()

    def form_bare():
        return timed_epoch(full, lambda k: step(sx, sy), lambda: None)

    def form_host():
        host.begin_epoch()
        return timed_epoch(full, lambda k: step(*host.batch_into(k, sx, sy)),
                           lambda: short and step(*host.batch_into(full, sx, sy)))

    def form_eager():
        loader.begin_epoch(form_eager.epoch)
        form_eager.epoch += 1

        def one(k):
            loader.fill(sx, sy)
            step(sx, sy)
        return timed_epoch(full, one, lambda: short and step(*loader.next_batch()))
    form_eager.epoch = 0

    def form_in_graph():
        loader.begin_epoch(form_in_graph.epoch)
        form_in_graph.epoch += 1
        return timed_epoch(full, lambda k: step.next(), lambda: short and step.next())
    form_in_graph.epoch = 100

    def overrun(signum, frame):
        raise SystemExit("epoch_bench: a form exceeded its time limit of %d s" % a.limit)
    signal.signal(signal.SIGALRM, overrun)

    def measure(name, form):
        signal.alarm(a.limit)
        form()                                               # the warm epoch
        runs = [form() for _ in range(a.rounds)]
        signal.alarm(0)
        t_full = statistics.median(r[0] for r in runs)
        t_all = statistics.median(r[1] for r in runs)
        imgs = full * B if name == "bare" else n
        return {"ms_per_step": 1e3 * t_full / full, "best_ms_per_step": 1e3 * min(r[0] for r in runs) / full,
                "images_per_s": imgs / t_all, "epoch_s": t_all}

    out = {"images": n, "batch": B, "full_batches": full, "last_batch": short, "rounds": a.rounds, "host_threads": a.host_threads}
    out["bare"] = measure("bare", form_bare)
    out["eager"] = measure("eager", form_eager)
    out["host"] = measure("host", form_host)
    out["bare_again"] = measure("bare", form_bare)           # the spread of the yardstick inside this process
    step.set_producer(loader)
    step.capture(x0, y0, warmup=0)
    out["in_graph"] = measure("in_graph", form_in_graph)
    out["in_graph_minus_bare_us"] = 1e3 * (out["in_graph"]["ms_per_step"] - min(out["bare"]["ms_per_step"],
                                                                               out["bare_again"]["ms_per_step"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
