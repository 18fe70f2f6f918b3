"""DSAN on the MI355X: the HIP LMMD (alignq_lmmd_fwd / _bwd through alignq_amd.mmd) against the reference's own values
(fixture G15) and the eager restatement (tests/test_dsan_cpu.py), run to run bit-identical; the tiny DSAN's two iterations
against fixture G16 through the plain and the channels-last dual path; the full-size captured DSAN step replayed bit for bit
against eager iterations with a different lambd in each."""
import os
import sys

import numpy as np
import pytest
import torch

from tests.conftest import load_golden
from tests.test_dsan_cpu import G15_NAMES, g15_case, run_restated

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from det_init import det_init_, sample  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    from alignq_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def cu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def npy(t):
    return t.detach().cpu().numpy()


def hip_lmmd(dev, xs, xt, ys, p, kernel_mul=2.0, kernel_num=5, fix_sigma=None, g=1.0, pair=False):
    from alignq_amd import mmd
    if pair:
        x = cu(np.concatenate([xs, xt]), dev).requires_grad_(True)
        loss = mmd.lmmd_pair(x, cu(ys, dev), cu(p, dev), kernel_mul, kernel_num, fix_sigma)
        (loss * g).backward()
        B = xs.shape[0]
        return npy(loss), npy(x.grad[:B]), npy(x.grad[B:])
    s, t = cu(xs, dev).requires_grad_(True), cu(xt, dev).requires_grad_(True)
    loss = mmd.lmmd(s, t, cu(ys, dev), cu(p, dev), kernel_mul, kernel_num, fix_sigma)
    assert loss.shape == (1,)
    (loss * g).backward()
    return npy(loss), npy(s.grad), npy(t.grad)


@pytest.mark.parametrize("ci", range(len(G15_NAMES)), ids=G15_NAMES)
def test_hip_lmmd_matches_reference_fixture(dev, ci):
    g = load_golden("g15_lmmd")
    c = g15_case(g, ci)
    loss, ds, dt = hip_lmmd(dev, c["xs"], c["xt"], c["ys"], c["p"], c["kernel_mul"], c["kernel_num"], c["fix_sigma"])
    ref = float(g[f"loss_{ci}"][0])
    if G15_NAMES[ci] in ("no_common", "identical"):
        # the NaN guard (bandwidth 0) and m = 0: loss 0 and exact zero gradients
        assert loss[0] == 0.0 and ref == 0.0
        assert not ds.any() and not dt.any() and np.isfinite(ds).all() and np.isfinite(dt).all()
    else:
        assert abs(float(loss[0]) - ref) <= 1e-5 * abs(ref), (float(loss[0]), ref)
        for got, key in ((ds, "ds"), (dt, "dt")):
            want = g[f"{key}_{ci}"]
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-5 * np.abs(want).max(), err_msg=key)
    # the dual path's form (both halves of one tensor, one gradient buffer) computes the same bits
    lp, dsp, dtp = hip_lmmd(dev, c["xs"], c["xt"], c["ys"], c["p"], c["kernel_mul"], c["kernel_num"], c["fix_sigma"], pair=True)
    assert np.array_equal(lp, loss) and np.array_equal(dsp, ds) and np.array_equal(dtp, dt)


@pytest.mark.parametrize("D", [256, 2048])
@pytest.mark.parametrize("B", [2, 7, 28, 32, 64])
def test_hip_lmmd_sweep_against_restatement(dev, B, D):
    rng = np.random.default_rng(1000 * B + D)
    C = 31
    xs = (rng.standard_normal((B, D)) * 0.7 + 0.05).astype(np.float32)
    xt = (rng.standard_normal((B, D)) * 1.2 - 0.1).astype(np.float32)
    ys = rng.integers(0, C, B).astype(np.int64)
    logits = rng.standard_normal((B, C)) * 2.0
    logits[0, ys[0]] += 10.0                                  # at least one class in common
    p = np.exp(logits - logits.max(1, keepdims=True))
    p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    gscale = 0.37                                             # the upstream gradient, read from device memory
    loss, ds, dt = hip_lmmd(dev, xs, xt, ys, p, g=gscale)
    ref, rds, rdt = run_restated(dict(xs=xs, xt=xt, ys=ys, p=p, kernel_mul=2.0, kernel_num=5, fix_sigma=None), torch.float64)
    assert ref[0] != 0.0
    assert abs(float(loss[0]) - ref[0]) <= 1e-5 * abs(ref[0]), (float(loss[0]), ref[0])
    np.testing.assert_allclose(ds, gscale * rds, rtol=0, atol=1e-5 * np.abs(gscale * rds).max())
    np.testing.assert_allclose(dt, gscale * rdt, rtol=0, atol=1e-5 * np.abs(gscale * rdt).max())


def test_hip_lmmd_is_bit_reproducible(dev):
    g = load_golden("g15_lmmd")
    for ci in (0, 2):
        c = g15_case(g, ci)
        a = hip_lmmd(dev, c["xs"], c["xt"], c["ys"], c["p"])
        b = hip_lmmd(dev, c["xs"], c["xt"], c["ys"], c["p"])
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_hip_lmmd_out_of_range_labels_join_no_class(dev):
    """A source label outside [0, C) adds to no class count and to no weight: the same as dropping its one-hot row."""
    g = load_golden("g15_lmmd")
    c = g15_case(g, 0)
    ys = c["ys"].copy()
    ys[3], ys[5] = 31, -4
    loss, ds, dt = hip_lmmd(dev, c["xs"], c["xt"], ys, c["p"])
    ref, rds, rdt = run_restated(dict(c, ys=ys), torch.float64)
    assert abs(float(loss[0]) - ref[0]) <= 1e-5 * abs(ref[0])
    np.testing.assert_allclose(ds, rds, rtol=0, atol=1e-5 * np.abs(rds).max())


def full_state(model, step, admms):
    """Everything an iteration leaves behind, by name (as tests/test_gpu_round6.py collects it)."""
    st = {}
    for n_, p in model.named_parameters():
        st["param:" + n_] = npy(p)
    for n_, b in model.named_buffers():
        st["buffer:" + n_] = npy(b)
    names = {id(p): n_ for n_, p in model.named_parameters()}
    for p, s in step.optimizer_t.state.items():
        if s.get("momentum_buffer") is not None:
            st["momentum:" + names[id(p)]] = npy(s["momentum_buffer"])
    for i, a in enumerate(admms):
        if a.D is not None:
            st["D:%d" % i] = npy(a.D)
    return st


def same_bits(a, b):
    """Equal as fp32 values (+0 == -0) with NaNs in the same places."""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def differing(sa, sb):
    assert set(sa) == set(sb), sorted(set(sa) ^ set(sb))
    return [(k, int(np.count_nonzero(sa[k] != sb[k])), sa[k].size) for k in sa if not same_bits(sa[k], sb[k])]


def _tiny_dsan(stage):
    from alignq_amd.resnet_office import DSAN, Bottleneck, ResNet
    return DSAN(lambda w, a, s: ResNet(w, a, s, Bottleneck, [1, 1, 1, 1], width_per_group=8), 4, 4, stage)


@pytest.mark.parametrize("channels_last,fuse_relu,dual", [(False, False, False), (True, True, True)])
def test_office_tiny_dsan_two_iterations_vs_reference(dev, channels_last, fuse_relu, dual):
    """DSANTrainStep on the tiny DSAN of fixture G16 (the reference's own modules through main.py:386-478, the LMMD over the
    bottlenecked features), two iterations with new_epoch between them and a different lambd each; the bars of the G10 test
    (tests/test_gpu_round2.py): whole-network values at 4-bit bin-flip scale, the two heads' updates by direction and size."""
    from alignq_amd import config
    from alignq_amd.train_step import DSANTrainStep
    g = load_golden("g16_office_tiny_dsan")
    g10 = load_golden(str(g["inputs"]))
    config.args.bitW = config.args.abitW = 4
    config.args.train_batch_size = config.args.eval_batch_size = 6
    try:
        torch.manual_seed(0)
        net = _tiny_dsan(str(g["stage"]))
        assert [n for n, _ in net.named_parameters()] == list(g["names"])
        det_init_(net)
        net = net.to(dev).train()
        step = DSANTrainStep(net, lr=float(g["lr"]), channels_last=channels_last, fuse_relu=fuse_relu, dual=dual)
        assert step.dual == dual
        named = list(net.named_parameters())
        init_state = {n: p.detach().clone() for n, p in named}
        prev = None
        for it, epoch in enumerate((1, 2)):
            rate = step.new_epoch(epoch, int(g["num_epochs"]), float(g["lr"]))
            assert abs(rate - float(g[f"rate_{it}"])) < 1e-12
            s_pred, loss, loss_mmd = step(cu(g10["xs"][it], dev), cu(g["ys"][it], dev), cu(g10["xt"][it], dev),
                                          float(g["lambd"][it]))
            torch.cuda.synchronize()
            if it == 0:
                np.testing.assert_allclose(npy(s_pred), g["s_pred_0"], atol=0.2)
            np.testing.assert_allclose(npy(loss_mmd), g[f"loss_mmd_{it}"], rtol=2e-2)
            np.testing.assert_allclose(npy(loss), g[f"loss_{it}"], rtol=2e-2)
            for bi, b in enumerate(step.blocks):
                d = np.abs(npy(b.admm0.D) - g[f"D_{it}_{bi}"]).max()
                assert d < (6e-3, 3e-2)[it], (it, bi, d)                               # the TARGET pass's D
            for j, (n, p) in enumerate(named):
                ref, got = g[f"after_{it}/{j}"], npy(sample(p))
                tol = (6e-3, 2e-2)[it] if ("alterD" in n or "gamma" in n) else (2.5e-3, 8e-3)[it]
                np.testing.assert_allclose(got, ref, atol=tol, err_msg=n)
            for j, (n, p) in enumerate(named):
                if not (n.startswith("bottle") or n.startswith("cls_fc")) or p.dim() != 2:
                    continue
                prev_ref = g[f"after_{it - 1}/{j}"] if it else npy(sample(init_state[n]))
                prev_got = prev[n] if it else npy(sample(init_state[n]))
                d_ref, d_got = g[f"after_{it}/{j}"] - prev_ref, npy(sample(p)) - prev_got
                cos = float((d_ref * d_got).sum() / (np.linalg.norm(d_ref) * np.linalg.norm(d_got) + 1e-30))
                ratio = float(np.linalg.norm(d_got) / (np.linalg.norm(d_ref) + 1e-30))
                assert cos > (0.99, 0.8)[it] and abs(ratio - 1.0) < (0.05, 0.3)[it], (n, it, cos, ratio)
                buf = npy(sample(step.optimizer_t.state[p]["momentum_buffer"]))
                rb = float(np.linalg.norm(buf) / (np.linalg.norm(g[f"buf_{it}/{j}"]) + 1e-30))
                assert abs(rb - 1.0) < (0.05, 0.3)[it], (n, it, rb)
            prev = {n: npy(sample(p)) for n, p in named}
    finally:
        config.args.bitW = config.args.abitW = 8
        config.args.train_batch_size, config.args.eval_batch_size = 128, 100


def test_captured_dsan_step_replays_eager_bit_for_bit(dev):
    """resnet50_dsan at full size (32 + 32 images of 224 x 224, channels-last, Conv2d_Q on the GEMM kernels, the dual
    traversal): four eager iterations against capture(warmup=2) + two replays, lambd different in each replayed iteration (the
    device scalar is refilled before each replay).  Every parameter, buffer, momentum buffer and ADMM.D bit for bit except the
    stem's (behind torch's max-pool backward, atomic adds: compared to rounding as in test_gpu_round6).  The capture itself
    shows that the step, the LMMD included, never synchronises with the host."""
    from alignq_amd import config
    from alignq_amd.resnet_office import resnet50_dsan
    from alignq_amd.train_step import DSANTrainStep, dsan_lambd
    old = (config.args.bitW, config.args.abitW, config.args.train_batch_size, config.args.eval_batch_size)
    config.args.bitW = config.args.abitW = 8
    B = 32
    config.args.train_batch_size = config.args.eval_batch_size = B
    try:
        gen = torch.Generator().manual_seed(12)
        xs = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
        xt = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
        ys = torch.randint(0, 31, (B,), generator=gen).to(dev)
        lambds = [dsan_lambd(i, 20, 100) for i in (40, 40, 41, 97)]     # the warm-up iterations share one value
        assert len(set(lambds[1:])) == 3

        def make():
            return det_init_(resnet50_dsan(8, 8)).to(dev).train()
        m1, m2 = make(), make()
        s1 = DSANTrainStep(m1, lr=4e-5, channels_last=True)
        s2 = DSANTrainStep(m2, lr=4e-5, channels_last=True)
        assert s1.dual and s1.qconv
        for lam in lambds:
            o1 = s1(xs, ys, xt, lam)
        s2.capture(xs, ys, xt, warmup=2, lambd=lambds[0])
        assert s2._graph is not None and s2._graph2 is None
        for lam in lambds[2:]:
            o2 = s2(xs, ys, xt, lam)
        torch.cuda.synchronize()
        assert torch.isfinite(o1[1]).all() and torch.isfinite(o2[1]).all()
        st1 = full_state(m1, s1, [b.admm0 for b in s1.blocks])
        st2 = full_state(m2, s2, [b.admm0 for b in s2.blocks])
        stem = ("feature_layers.conv1.", "feature_layers.bn1.")
        for key in [k for k in st1 if k.split(":", 1)[1].startswith(stem)]:
            np.testing.assert_allclose(st1[key], st2[key], rtol=1e-5, atol=1e-7 * float(np.abs(st1[key]).max()) + 1e-12, err_msg=key)
            st1.pop(key), st2.pop(key)
        bad = differing(st1, st2)
        for a, b in zip(o1, o2):
            assert same_bits(npy(a), npy(b)), (npy(a).ravel()[:4], npy(b).ravel()[:4])
        assert not bad, "graph replay differs from eager in %d tensors, first: %s" % (len(bad), bad[:6])
    finally:
        config.args.bitW, config.args.abitW, config.args.train_batch_size, config.args.eval_batch_size = old
