"""Captured DSAN step at full size (resnet50_dsan, B + B images of 224 x 224, channels-last, Conv2d_Q on the GEMM kernels, the
dual traversal): capture(warmup=2), then --steps replays with a new lambd each, timed with device events.  Prints one line
`dsan ms_per_step <t>`.  Under `rocprofv3 --kernel-trace --stats -- python tools/dsan_step.py` the statistics list the LMMD
launches (lmmd_l2_kernel, lmmd_fwd_finish_kernel, lmmd_bwd_kernel) beside the backbone's."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    from alignq_amd import config
    from alignq_amd.resnet_office import resnet50_dsan
    from alignq_amd.train_step import DSANTrainStep, dsan_lambd
    dev = torch.device("cuda:0")
    config.args.bitW = config.args.abitW = 8
    config.args.train_batch_size = config.args.eval_batch_size = a.batch
    torch.manual_seed(0)
    xs = torch.randn(a.batch, 3, 224, 224, device=dev)
    xt = torch.randn(a.batch, 3, 224, 224, device=dev)
    ys = torch.randint(0, 31, (a.batch,), device=dev)
    step = DSANTrainStep(resnet50_dsan(8, 8).to(dev).train(), lr=4e-5, channels_last=True)
    step.capture(xs, ys, xt, warmup=2, lambd=dsan_lambd(0, 20, 100))
    for i in range(3):
        step(xs, ys, xt, dsan_lambd(i, 20, 100))
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(a.steps):
        out = step(xs, ys, xt, dsan_lambd(3 + i, 20, 100))
    t1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(out[1]).all()
    print("dsan ms_per_step %.3f loss %.4f loss_mmd %.4f" % (t0.elapsed_time(t1) / a.steps, float(out[1]), float(out[2])))


if __name__ == "__main__":
    main()
