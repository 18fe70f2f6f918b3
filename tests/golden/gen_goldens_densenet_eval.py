#!/usr/bin/env python3
"""Golden-vector generator for DenseNet's evaluation pass (cdf_alignment/dense-cifar-10: main.py's test(), model/densenet.py,
utils/common.py's accuracy), with the recipe of gen_goldens_mobilenet_eval.py and the model of gen_goldens_densenet.py: the
reference's own modules on CPU at densenet_init.REDUCED (depth 10: two layers per dense block), densenet_init_, 8W/8A, 32x32 inputs,
batch 8.  Writes

  G22 g22_densenet_eval.npz
    three training-mode forwards on seeded batches (the running statistics leave (0, 1)), then net.eval() and test()'s forward on a
    fresh seeded batch: every batch-norm buffer, the evaluation input, the reference's logits, CrossEntropyLoss, and Prec@1 / Prec@5
    from the reference's utils.accuracy for the stored targets, as percentages and as counts.

  The targets are CHOSEN from the reference's logits as G20's are (gen_goldens_mobilenet_eval._choose): rows cycle through top-1 hit,
  top-5-only hit and miss, each target's logit as far as possible from the logits at the rank-1 and rank-5 boundaries.  The input seed
  is searched until every row's distance is at least MARGIN_FRACTION of the row's logit range; `min_margin` is the smallest distance of
  the batch: an implementation whose logits stay within min_margin / 2 of the reference's ranks every row the same way.

  Tensors and numbers only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_goldens_densenet_eval.py
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import gen_goldens as G  # noqa: E402
import gen_goldens_densenet as GD  # noqa: E402
from gen_goldens_mobilenet_eval import MARGIN_FRACTION, _choose  # noqa: E402

BATCH, SIDE, BITS = 8, 32, 8
TRAIN_SEEDS = (2201, 2202, 2203)
EVAL_SEED0 = 2300


def gen():
    import torch
    from densenet_init import REDUCED, densenet_init_
    torch.manual_seed(0)
    q, args, m = GD._enter(BITS)
    accuracy = importlib.import_module("utils.common").accuracy
    assert args.bitW == BITS and args.abitW == BITS and float(args.act_range) == 2.0
    net = densenet_init_(m.DenseNet(BITS, BITS, args.stage, **REDUCED))
    net.train()
    for seed in TRAIN_SEEDS:
        out = net(torch.randn(BATCH, 3, SIDE, SIDE, generator=torch.Generator().manual_seed(seed)))
        assert torch.isfinite(out).all()
    net.eval()
    buffers = {k: G._np(v) for k, v in net.state_dict().items()
               if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    assert all(int(v) == len(TRAIN_SEEDS) for k, v in buffers.items() if k.endswith("num_batches_tracked"))
    assert max(float(np.abs(v).max()) for k, v in buffers.items() if k.endswith("running_mean")) > 0.0

    found = None
    for seed in range(EVAL_SEED0, EVAL_SEED0 + 500):
        x = torch.randn(BATCH, 3, SIDE, SIDE, generator=torch.Generator().manual_seed(seed))
        with torch.no_grad():
            logits = net(x)
        lg = G._np(logits)
        if not np.isfinite(lg).all():
            continue
        picks = [_choose(lg[i], i % 3) for i in range(BATCH)]
        if all(mg >= MARGIN_FRACTION * float(lg[i].max() - lg[i].min()) for i, (_, mg) in enumerate(picks)):
            found = (seed, x, logits, lg, picks)
            break
    assert found is not None, "no input seed gives every row its margin"
    seed, x, logits, lg, picks = found
    targets = torch.tensor([t for t, _ in picks], dtype=torch.int64)
    min_margin = min(mg for _, mg in picks)
    with torch.no_grad():
        ce = torch.nn.CrossEntropyLoss()(logits, targets)
        prec1, prec5 = accuracy(logits, targets, topk=(1, 5))
    n1 = sum(1 for i in range(BATCH) if i % 3 == 0)
    n5 = sum(1 for i in range(BATCH) if i % 3 != 2)
    assert round(float(prec1[0]) * BATCH / 100.0) == n1 and round(float(prec5[0]) * BATCH / 100.0) == n5
    print("seed", seed, "min_margin", min_margin, "ce", float(ce), "prec1", float(prec1[0]), "prec5", float(prec5[0]),
          "max |logit|", float(np.abs(lg).max()))
    out = {"stage": np.array(str(args.stage)), "act_range": np.array(float(args.act_range)), "bits": np.array(BITS),
           "batch": np.array(BATCH), "depth": np.array(REDUCED["depth"]), "compression": np.array(REDUCED["compressionRate"]),
           "eval_seed": np.array(seed), "x": G._np(x), "logits": lg, "targets": G._np(targets), "ce": np.array(float(ce)),
           "prec1": np.array(float(prec1[0])), "prec5": np.array(float(prec5[0])), "n_top1": np.array(n1), "n_top5": np.array(n5),
           "min_margin": np.array(min_margin), "margin_fraction": np.array(MARGIN_FRACTION),
           "buffer_names": np.array(list(buffers.keys()))}
    out.update({"buf_" + k: v for k, v in buffers.items()})
    G._save("g22_densenet_eval", **out)
    size = os.path.getsize(os.path.join(HERE, "g22_densenet_eval.npz"))
    assert size < 1000000, size
    print("bytes", size)


if __name__ == "__main__":
    gen()
