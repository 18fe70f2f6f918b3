"""Seeded inputs and NumPy restatements shared by the evaluation fixtures' generator (gen_goldens_eval.py, reference side) and
the tests (test_eval_cpu.py, test_gpu_eval.py): G17 / G18 store no inputs, only what the reference computed from these.
Values come from torch's CPU generator (stable across machines for one torch build, like det_init.py)."""
import numpy as np
import torch

# G17: one site per tree.  [B, C, H, W]: 6144 elements = one and a half tiles of the kernel (4 x 256 float4), B = 6 is a short batch
SITE_SHAPE = {"admm": (6, 16, 8, 8), "cdf": (6, 16, 8, 8), "office": (6, 64, 4, 4)}
SITE_SEED = {"admm": 1701, "cdf": 1702, "office": 1703}
SITE_KS = (2, 4, 8)
BN_EPS = 1e-5

# G18: whole networks.  (batch, image side, classes, bits, training-mode forwards before the evaluation)
NET = {"admm": (100, 32, 10, 8, 2), "cdf": (100, 32, 10, 8, 2), "office": (28, 64, 31, 8, 2)}
NET_SEED = {"admm": 1801, "cdf": 1802, "office": 1803}
MARGIN = 1e-3


def site_inputs(tree):
    """z (the convolution's output), the shortcut, and the batch-norm's vectors with running statistics away from (0, 1)"""
    B, C, H, W = SITE_SHAPE[tree]
    g = torch.Generator().manual_seed(SITE_SEED[tree])
    z = torch.randn(B, C, H, W, generator=g) * 1.5 + 0.3
    res = torch.randn(B, C, H, W, generator=g)
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = torch.randn(C, generator=g) * 0.3
    mean = torch.randn(C, generator=g) * 0.5 + 0.2
    var = 0.3 + 2.0 * torch.rand(C, generator=g)
    return z, res, gamma, beta, mean, var


def site_bn(tree):
    """an eval-mode nn.BatchNorm2d holding site_inputs' vectors"""
    _, _, gamma, beta, mean, var = site_inputs(tree)
    bn = torch.nn.BatchNorm2d(gamma.numel(), eps=BN_EPS)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(mean); bn.running_var.copy_(var)
    return bn.eval()


def net_inputs(tree, target_seed=None):
    """(training batches [n, B, 3, S, S], evaluation batch [B, 3, S, S], targets [B] or None)"""
    B, S, classes, _, n_train = NET[tree]
    g = torch.Generator().manual_seed(NET_SEED[tree])
    xtr = torch.randn(n_train, B, 3, S, S, generator=g)
    xev = torch.randn(B, 3, S, S, generator=g) * 1.1 + 0.05
    y = None
    if target_seed is not None:
        y = torch.randint(0, classes, (B,), generator=torch.Generator().manual_seed(int(target_seed)))
    return xtr, xev, y


def levels(xq, k, r, tree):
    """the integer level index behind a quantiser output (float64 arithmetic on the stored fp32 value)"""
    n = 2 ** k - 1
    xq = np.asarray(xq, dtype=np.float64)
    if tree == "cdf":
        return np.rint((xq / r + 1.0) * 0.5 * n).astype(np.int64)
    return np.rint(xq * n).astype(np.int64)


def margins(logits, target):
    """per row: distance of the target's logit to its top-1 boundary (the largest other logit) and to its top-5 boundary (the
    fifth-largest other logit)"""
    lg = np.asarray(logits, dtype=np.float64)
    out = np.empty((lg.shape[0], 2))
    for i, (row, t) in enumerate(zip(lg, target)):
        others = np.sort(np.delete(row, int(t)))[::-1]
        out[i] = abs(row[int(t)] - others[0]), abs(row[int(t)] - others[4])
    return out


def ab_numpy(gamma, beta, mean, var, eps):
    """include/alignq.h: s = sqrt(var + eps); a = gamma / s; b = beta - (a * mean), fp32, each operation rounded on its own"""
    f = np.float32
    s = np.sqrt((var.astype(f) + f(eps)).astype(f)).astype(f)
    a = (gamma.astype(f) / s).astype(f)
    b = (beta.astype(f) - (a * mean.astype(f)).astype(f)).astype(f)
    return a, b


def metrics_numpy(logits, target):
    """(sum ce, top-1, top-5, rows) as include/alignq.h states them for alignq_eval_metrics, in float64 from the fp32 logits"""
    lg = np.asarray(logits).astype(np.float64)
    K = lg.shape[1]
    ce, n1, n5 = 0.0, 0, 0
    for row, t in zip(lg, target):
        if not (0 <= t < K):
            continue
        m = np.nanmax(row)
        ce += m + np.log(np.sum(np.exp(row - m))) - row[t]
        if np.isnan(row).any():
            continue
        rank = int(np.sum(row > row[t]))
        n1 += rank < 1
        n5 += rank < 5
    return ce, int(n1), int(n5), len(target)
